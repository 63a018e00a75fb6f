"""Guarded, poisoned and repeated launches: a test-side allocator for the op wrappers.

The plan tests compare every kernel with an fp64 reference, but three kinds of error pass them: a read of memory nobody
initialised (the caching allocator hands a wrapper the block its previous, identical launch just filled with the right
values), a store outside the tensor (it lands in allocator slack), and a run-to-run difference.  This harness makes all
three visible without a reference:

  * `Guard(pattern)` owns a proxy that takes the place of the module global `torch` in the wrapper modules
    (`with guard.installed(ops, ops_bwd): ...`).  The proxy forwards every attribute to the real torch except `empty`,
    `empty_like`, `empty_strided` -- which return a view into a larger uint8 buffer filled with ONE byte pattern, GUARD
    bytes in front of the view and GUARD behind it, the interior carrying the same pattern -- and `zeros`, `zeros_like`,
    `full`, which get the same guards and keep their own fill.  0xFF reads as NaN in bf16 / fp16 / fp32 and as -1 in
    integers, 0x7B as a large finite value in all three float types and a large positive integer.
  * `guard.place(t)` copies an input's whole storage into a guarded buffer once per storage and returns the view of the
    same size, stride and offset (q / k / v stay slices of one fused buffer); `guard.inout(t)` does the same for a tensor
    the op writes (out= with accumulate, dx_add, gradient slices).
  * `guard.verify()` (after the device is idle) checks every guard byte of every buffer and that every placed input's
    storage is byte-equal to the original.  The guard holds a reference to every buffer until then: the wrappers drop
    their scratch while the kernel is still running.
  * `check_launches(modules, call)` runs `call(run)` three times -- plain, under 0xFF, under 0x7B -- and requires
    everything it returns to be bit-equal across the three and both verifications to pass.  An element never written
    differs between the two patterns; a read of uninitialised scratch or past an input is NaN in one run and something
    else in the other; a race shows as a difference.  There is no tolerance.  On a device the two pattern launches also
    fill every CU's LDS with the same byte in front of every launching library call (tests/lds_poison.py), so the same
    bit-equality covers LDS a kernel reads without having written it; lds=False leaves LDS alone.

A torn store begins right behind the tensor's end, so the first guard bytes catch it; GUARD is a multiple of 512, so the
view keeps the alignment the allocator gives.  A store that lands further away cannot be caught by a guard of any size.
Eager launches only: inside a graph capture the fills would become graph nodes.

Every allocation records the chain of function names of the calling module that asked for it, innermost first
(("_gemm_launch", "_gemm_call", "linear")): `owner` is the first public name of the chain.
"""
import contextlib
import sys

import torch as _torch

GUARD = 1 << 20
PATTERNS = (0xFF, 0x7B)


class GuardError(AssertionError):
    pass


def _numel(size):
    n = 1
    for d in size:
        n *= int(d)
    return n


def _size_of(args):
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(int(d) for d in args[0])
    return tuple(int(d) for d in args)


def _bytes_of_storage(t):
    """uint8 view of t's whole storage."""
    st = t.untyped_storage()
    return _torch.empty(0, dtype=_torch.uint8, device=t.device).set_(st, 0, (st.nbytes(),), (1,))


def _chain(depth=2):
    """Function names of the frames of the file that called the proxy, innermost first."""
    f = sys._getframe(depth)
    fname, names = f.f_code.co_filename, []
    while f is not None and f.f_code.co_filename == fname:
        if not f.f_code.co_name.startswith("<"):
            names.append(f.f_code.co_name)
        f = f.f_back
    return tuple(names) or ("<module>",)


class _Buf:
    __slots__ = ("raw", "nbytes", "chain", "orig", "orig_bytes", "kind")

    @property
    def owner(self):
        return next((n for n in self.chain if not n.startswith("_")), self.chain[0])

    @property
    def lo(self):
        return self.raw.data_ptr() + GUARD

    def describe(self):
        return f"buffer of {self.nbytes} bytes {self.kind} by {self.owner} (call chain {' <- '.join(self.chain)})"


class _TorchProxy:
    """Stands in for the module global `torch`: everything is the real torch's except the allocating calls."""

    def __init__(self, guard):
        object.__setattr__(self, "_guard", guard)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch proxy is read-only")

    # ---- pattern-filled
    def empty(self, *size, dtype=None, device=None, **kw):
        if kw:      # pinned host staging buffers and the like are not kernel outputs: the real call
            return _torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._guard._alloc(_size_of(size), None, dtype, device, None, _chain())

    def empty_like(self, t, dtype=None, device=None, **kw):
        if kw:
            return _torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._guard._alloc(tuple(t.shape), None, dtype or t.dtype, device or t.device, None, _chain())

    def empty_strided(self, size, stride, dtype=None, device=None, **kw):
        if kw:
            return _torch.empty_strided(size, stride, dtype=dtype, device=device, **kw)
        return self._guard._alloc(tuple(size), tuple(stride), dtype, device, None, _chain())

    # ---- guarded, own fill
    def zeros(self, *size, dtype=None, device=None, **kw):
        if kw:
            return _torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._guard._alloc(_size_of(size), None, dtype, device, 0, _chain())

    def zeros_like(self, t, dtype=None, device=None, **kw):
        if kw:
            return _torch.zeros_like(t, dtype=dtype, device=device, **kw)
        return self._guard._alloc(tuple(t.shape), None, dtype or t.dtype, device or t.device, 0, _chain())

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if kw:
            return _torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:
            dtype = _torch.full((), fill_value).dtype
        return self._guard._alloc(tuple(size), None, dtype, device, fill_value, _chain())


class Plain:
    """The unguarded launch of check_launches: the same surface as Guard, the real allocator."""
    pattern = None

    def empty(self, *size, dtype=None, device=None):
        return _torch.empty(*size, dtype=dtype, device=device)

    def full(self, size, fill_value, dtype=None, device=None):
        return _torch.full(size, fill_value, dtype=dtype, device=device)

    def place(self, t):
        return t

    def inout(self, t):
        """A fresh copy of t's whole storage, t's view of it."""
        if t is None:
            return None
        raw = _bytes_of_storage(t).clone()
        return _torch.empty(0, dtype=t.dtype, device=t.device).set_(raw.untyped_storage(), t.storage_offset(), t.shape, t.stride())


class Guard:
    def __init__(self, pattern):
        assert 0 <= pattern <= 255
        self.pattern = pattern
        self.bufs = []
        self._placed = {}
        self.torch = _TorchProxy(self)

    # ---- allocation
    def _raw(self, nbytes, device, chain, kind):
        b = _Buf()
        b.raw = _torch.empty(GUARD + nbytes + GUARD, dtype=_torch.uint8, device=device)
        b.raw.fill_(self.pattern)
        b.nbytes, b.chain, b.kind, b.orig, b.orig_bytes = nbytes, chain, kind, None, None
        self.bufs.append(b)
        return b

    def _alloc(self, size, stride, dtype, device, fill, chain):
        dtype = dtype or _torch.get_default_dtype()
        device = _torch.device(device) if device is not None else _torch.device("cpu")
        if device.type == "cuda" and device.index is None:
            device = _torch.device("cuda", _torch.cuda.current_device())
        if stride is None:
            stride, acc = [], 1
            for d in reversed(size):
                stride.insert(0, acc)
                acc *= max(int(d), 1)
        n = _numel(size)
        extent = 0 if n == 0 else 1 + sum((int(d) - 1) * int(s) for d, s in zip(size, stride))
        esz = _torch.empty(0, dtype=dtype).element_size()
        b = self._raw(extent * esz, device, chain, "allocated")
        t = _torch.empty(0, dtype=dtype, device=device).set_(b.raw.untyped_storage(), GUARD // esz, size, tuple(stride))
        if fill is not None:
            t.fill_(fill)
        return t

    def empty(self, *size, dtype=None, device=None):
        """An output the test itself hands to the op (lse=, out=): allocated like a wrapper's torch.empty."""
        return self._alloc(_size_of(size), None, dtype, device, None, _chain())

    def full(self, size, fill_value, dtype=None, device=None):
        return self._alloc(tuple(size), None, dtype, device, fill_value, _chain())

    def _place(self, t, inout):
        if t is None:
            return None
        key = t.untyped_storage().data_ptr()
        b = self._placed.get(key)
        if b is None:
            src = _bytes_of_storage(t)
            b = self._raw(src.numel(), t.device, _chain(3), "placed")
            b.raw[GUARD:GUARD + src.numel()].copy_(src)
            b.orig, b.orig_bytes = t, src.clone()       # t keeps the storage, and with it the key, alive
            self._placed[key] = b
        if inout:
            b.orig_bytes, b.kind = None, "placed (in/out)"
        return _torch.empty(0, dtype=t.dtype, device=t.device).set_(b.raw.untyped_storage(),
                                                                     GUARD // t.element_size() + t.storage_offset(), t.shape, t.stride())

    def place(self, t):
        """t's view of a guarded copy of its whole storage (one copy per storage); verify() requires the copy to stay
        byte-equal to the original, unless the storage is also handed over as an in/out tensor."""
        return self._place(t, False)

    def inout(self, t):
        """place() for a tensor the op writes: guarded, not compared with the original."""
        return self._place(t, True)

    @contextlib.contextmanager
    def installed(self, *modules):
        saved = [(m, m.__dict__["torch"]) for m in modules]
        for m, _ in saved:
            m.torch = self.torch
        try:
            yield self
        finally:
            for m, real in saved:
                m.torch = real

    # ---- checks
    def names(self):
        return {n for b in self.bufs for n in b.chain}

    def owner_of(self, t):
        """The buffer whose interior holds t's first byte, or None."""
        p = t.data_ptr()
        for b in self.bufs:
            if b.lo <= p < b.lo + max(b.nbytes, 1) and b.raw.device == t.device:
                return b
        return None

    def verify(self):
        """Every guard byte intact, every placed input unchanged; GuardError names each offender's wrapper."""
        if not self.bufs:
            return
        flags = []
        for b in self.bufs:
            front = (b.raw[:GUARD] != self.pattern).any()
            back = (b.raw[GUARD + b.nbytes:] != self.pattern).any()
            changed = (b.raw[GUARD:GUARD + b.nbytes] != b.orig_bytes).any() if b.orig_bytes is not None else front & False
            flags.append(_torch.stack([front, back, changed]))
        by_dev = {}                  # one transfer per device, not one per buffer
        for i, f in enumerate(flags):
            by_dev.setdefault(f.device, []).append(i)
        bad = {}
        for idx in by_dev.values():
            for row, i in zip(_torch.stack([flags[i] for i in idx]).cpu().tolist(), idx):
                if any(row):
                    bad[i] = row
        if not bad:
            return
        msgs = []
        for i, (front, back, changed) in sorted(bad.items()):
            b = self.bufs[i]
            if front:
                at = int((b.raw[:GUARD] != self.pattern).nonzero()[-1])
                msgs.append(f"store in front (last damaged guard byte -{GUARD - at}) of the {b.describe()}")
            if back:
                at = int((b.raw[GUARD + b.nbytes:] != self.pattern).nonzero()[0])
                msgs.append(f"store past the end (first damaged guard byte +{at}) of the {b.describe()}")
            if changed:
                at = int((b.raw[GUARD:GUARD + b.nbytes] != b.orig_bytes).nonzero()[0])
                msgs.append(f"input modified at byte {at}: {b.describe()}")
        raise GuardError(f"pattern 0x{self.pattern:02X}: " + "; ".join(msgs))


# ------------------------------------------------------------------------------------------------ three launches

def flatten(out):
    """Every tensor of what an op returned, in a fixed order: tensors, sequences, dicts (by key); the fused GroupNorm sums
    a conv attaches to its output (`_gn_stats`) count as returned."""
    if out is None:
        return []
    if isinstance(out, _torch.Tensor):
        st = getattr(out, "_gn_stats", None)
        return [out] + ([st[0]] if st is not None else [])
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in flatten(out[k])]
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in flatten(o)]
    return []


def bits(t):
    """A private copy of t's bytes, logical order."""
    c = t.detach().contiguous()
    if c.dtype == _torch.bool:
        c = c.to(_torch.uint8)
    return c.reshape(-1).view(_torch.uint8).clone()


def _sync():
    if _torch.cuda.is_available() and _torch.cuda.is_initialized():
        _torch.cuda.synchronize()


class _Differs(Exception):
    """A result of a pattern run is not the plain run's: the message, before anyone knows which pattern caused it."""


def _pattern_run(modules, call, p, lds_pattern, lds, ref, shapes):
    """One guarded launch under memory pattern p, LDS filled with the byte lds_pattern in front of every library call (None:
    LDS left alone).  Returns (names recorded, entry points poisoned); GuardError from verify(), _Differs from the comparison."""
    g = Guard(p)
    poisoned = set()
    with contextlib.ExitStack() as stack:
        if lds_pattern is not None:
            proxy = stack.enter_context(lds(lds_pattern))
            poisoned = proxy.poisoned
        stack.enter_context(g.installed(*modules))
        res = flatten(call(g))
    _sync()
    g.verify()
    got = [(tuple(t.shape), t.dtype) for t in res]
    if got != shapes:
        raise GuardError(f"pattern 0x{p:02X}: the launch returned {got}, the plain one {shapes}")
    for i, (t, r) in enumerate(zip(res, ref)):
        b = bits(t)
        if not _torch.equal(b, r):
            ne = (b != r).nonzero()
            esz = t.element_size()
            buf = g.owner_of(t)
            what = buf.describe() if buf is not None else "tensor the guard did not allocate"
            raise _Differs(f"result {i} {shapes[i]} differs from the plain launch in {ne.numel()} byte(s), "
                           f"first at element {int(ne[0]) // esz}, last at element {int(ne[-1]) // esz}: {what}")
    return g.names(), set(poisoned)


def _lds_installer(lds):
    """lds=True: tests/lds_poison.installed, where there is a device to poison; a callable: that context manager."""
    if lds is True:
        if not _torch.cuda.is_available():
            return None
        import lds_poison
        return lds_poison.installed
    return lds or None


def check_launches(modules, call, declared=(), patterns=PATTERNS, lds=True):
    """call(run) three times: run = Plain(), then a Guard per pattern installed in `modules`.  call places its inputs
    (run.place / run.inout), allocates the outputs it hands over (run.empty) and returns every tensor that is a result.
    GuardError unless the results are bit-equal across the three launches, both verifications pass and every name in
    `declared` appears in a call chain of the recorded allocations -- or, for a name that begins with `dfw_`, among the
    library entry points that were preceded by an LDS fill.  Returns the names recorded, those entry points included.

    lds (default on, where there is a device): in the two pattern launches every launching entry point of the library is
    also preceded by a fill of every CU's LDS with the same byte (tests/lds_poison.py: 0xFF is NaN in the three float types
    and -1 in integers, 0x7B large and finite), so the bit-equality covers what a kernel reads from LDS without having
    written it.  The plain launch stays plain.  An entry point that launches several kernels gets the fill in front of its
    first one only.  When a result differs, the launch is repeated under the same memory pattern with LDS zero-filled: if
    that one is bit-equal, the error says that LDS is the cause and names the entry points poisoned.  lds=False: memory
    only; a callable `lds(pattern)`: that context manager in place of lds_poison.installed."""
    install = _lds_installer(lds)
    run = Plain()
    res = flatten(call(run))
    _sync()
    ref = [bits(t) for t in res]
    shapes = [(tuple(t.shape), t.dtype) for t in res]
    del res
    names = set()
    for p in patterns:
        try:
            recorded, poisoned = _pattern_run(modules, call, p, p if install else None, install, ref, shapes)
            if install and not poisoned:
                raise GuardError(f"pattern 0x{p:02X}: no library call of this case was preceded by an LDS fill: it does not fetch "
                                 "the handle through diffews_amd._lib.lib() (lds=False for a case that launches nothing)")
            names |= poisoned
        except _Differs as e:
            if not install:
                raise GuardError(f"pattern 0x{p:02X}: {e}") from None
            try:
                _, poisoned = _pattern_run(modules, call, p, 0x00, install, ref, shapes)
            except (_Differs, GuardError):
                raise GuardError(f"pattern 0x{p:02X} (in memory and in LDS; the difference stays with LDS zero-filled, so it is "
                                 f"not the LDS pattern's): {e}") from None
            raise GuardError(f"LDS pattern 0x{p:02X} (word 0x{p * 0x01010101:08X} in every CU's LDS in front of "
                             f"{', '.join(sorted(poisoned)) or 'no entry point'}): {e}; the same launch under memory pattern "
                             f"0x{p:02X} with LDS zero-filled is bit-equal to the plain one: a kernel of these entry points "
                             "reads LDS it has not written, no allocation is involved") from None
        names |= recorded
    missing = set(declared) - names
    if missing:
        raise GuardError(f"no allocation was recorded for {sorted(missing)}; recorded: {sorted(names)}")
    return names
