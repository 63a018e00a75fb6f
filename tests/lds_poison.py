"""LDS poison: what tests/launch_guard.py does for the allocator, for the 160 KiB of LDS on every CU.

LDS is not cleared between the dispatches of one process, so a workgroup starts on what the previous kernel on its CU left
behind.  The kernels multiply rows "zero-filled by the buffer bounds check", `0 x V` rows behind masked keys, sum staging
tiles and read LDS tables other threads initialise; in the plan tests the neighbour is another float kernel on seeded randn
data and every leftover is finite and plausible, in the product it is an integer kernel that leaves -1 words (NaN in bf16,
fp16 and fp32).  This module fills every CU's LDS with ONE word immediately before a library call:

  * `tests/lds_poison.hip` (built here with the hipcc and the architecture flag of diffews_amd/build.py into a cache
    directory keyed by the source hash, loaded with ctypes AFTER torch so that it binds torch's HIP runtime -- see
    `_lib.lib()`; nothing is compiled at import) has `fill(word)`, `probe(word)` and three planted defects.
  * `LibProxy` wraps the ctypes handle `_lib.lib()` returns.  Every attribute is forwarded unchanged; a call of a LAUNCHING
    entry point -- a function of include/diffews_hip.h that takes a `dfw_stream_t`, the list is parsed from the header -- is
    preceded by a `fill` on `torch.cuda.current_stream()`.  `*_workspace_bytes`, `*_kernel_name`, `dfw_configure` and the
    like are not.  Nothing is issued while the stream is capturing (the fill would become a graph node).  The proxy keeps
    the set of entry points it poisoned.
  * `installed(pattern)` swaps `diffews_amd._lib.lib` for a function that returns the proxy and restores it on exit.  ops,
    ops_bwd, unet, vae, pipeline, train and input_pipeline fetch the handle through `L.lib()` at every call, so the one swap
    covers them all.

Limit: an entry point that launches several kernels (zero + main, split-K + reduce, the four launches of the native routes)
gets the fill in front of its FIRST kernel only; the later ones see what their predecessor left, as in production.

GRID_MULTIPLE and STAY_TICKS are the values at which one fill reached every CU of an idle MI355X
(profiles/lds_poison.md); tests/test_lds_poison_gpu.py holds that as a condition.
"""
import contextlib
import ctypes as C
import hashlib
import os
import re
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(HERE, "lds_poison.hip")
HEADER = os.path.join(ROOT, "include", "diffews_hip.h")

THREADS = 256
LDS_WORDS = 160 * 1024 // 4
GRID_MULTIPLE = 4          # workgroups per CU in one fill
STAY_TICKS = 500           # s_memrealtime ticks (10 ns) a workgroup stays after writing: 5 us
PATTERNS = (0xFF, 0x7B)
PLANTED = ("lds_planted_zero_times", "lds_planted_histogram", "lds_planted_staging")

_vp, _i32, _u32 = C.c_void_p, C.c_int32, C.c_uint32
_SYMBOLS = {
    "lds_poison_fill": (_i32, [_u32, _i32, _i32, _vp, _vp]),
    "lds_poison_probe": (_i32, [_u32, _i32, _i32, _vp, _vp, _vp]),
    "lds_poison_words": (_i32, []),
    "lds_planted_zero_times": (_i32, [_vp, _vp, _i32, _vp]),
    "lds_planted_histogram": (_i32, [_vp, _vp, _i32, _vp]),
    "lds_planted_staging": (_i32, [_vp, _vp, _i32, _vp]),
}


def word_of(pattern):
    """The byte pattern repeated into a 32-bit word (0xFF -> 0xFFFFFFFF)."""
    assert 0 <= pattern <= 255
    return pattern * 0x01010101


# ------------------------------------------------------------------------------------------------ which entry points launch

def launching_from_header(path=HEADER):
    """Names of the functions the header declares with a `dfw_stream_t` parameter, in order of declaration."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    names = []
    for m in re.finditer(r"\b(dfw_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        if re.search(r"\bdfw_stream_t\b", m.group(2)):
            names.append(m.group(1))
    return names


_LAUNCHING = None


def launching():
    global _LAUNCHING
    if _LAUNCHING is None:
        _LAUNCHING = frozenset(launching_from_header())
    return _LAUNCHING


# ------------------------------------------------------------------------------------------------ build and load

def _flags():
    from diffews_amd import build as B
    return [f for f in B.FLAGS if f.startswith("--offload-arch=")] + ["-O3", "-std=c++17", "-fPIC", "-shared"]


def cache_dir():
    return os.environ.get("DFW_TEST_CACHE") or os.path.join(tempfile.gettempdir(), f"diffews_amd_tests_{os.getuid()}")


def build(out_dir=None):
    """Compile tests/lds_poison.hip (once per source hash) and return the shared object's path."""
    flags = _flags()
    with open(SOURCE, "rb") as f:
        key = hashlib.sha256(" ".join(flags).encode() + b"\0" + f.read()).hexdigest()[:16]
    out_dir = out_dir or cache_dir()
    so = os.path.join(out_dir, f"lds_poison_{key}.so")
    if os.path.isfile(so):
        return so
    os.makedirs(out_dir, exist_ok=True)
    tmp = f"{so}.{os.getpid()}.tmp"
    cmd = [os.environ.get("HIPCC", "hipcc"), *flags, "-o", tmp, SOURCE]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {SOURCE}:\n{r.stdout}")
    os.replace(tmp, so)
    return so


_handle = None


def handle():
    """The ctypes handle of the poisoner, built on first use and loaded after torch."""
    global _handle
    if _handle is None:
        so = build()
        import torch  # noqa: F401      (first: the poisoner must bind torch's HIP runtime, as _lib.lib() explains)
        h = C.CDLL(so)
        for name, (res, args) in _SYMBOLS.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        assert h.lds_poison_words() == LDS_WORDS
        _handle = h
    return _handle


# ------------------------------------------------------------------------------------------------ fill and probe

def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _capturing():
    import torch
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def cu_count():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: HIP error {rc}")


def fill(word, where=None, multiple=GRID_MULTIPLE, ticks=STAY_TICKS):
    """Write `word` to all LDS of every CU, on the current stream.  `where`: an int32 tensor [multiple * CUs, 2] that
    receives (XCC id, hardware id) of every workgroup."""
    grid = multiple * cu_count()
    assert where is None or (where.numel() == 2 * grid and where.element_size() == 4 and where.is_contiguous())
    _check(handle().lds_poison_fill(word, grid, ticks, where.data_ptr() if where is not None else None, _stream()), "lds_poison_fill")


def probe(word, multiple=GRID_MULTIPLE, ticks=STAY_TICKS):
    """(counts [grid] of LDS words equal to `word` per workgroup, where [grid, 2]) as device tensors, current stream."""
    import torch
    grid = multiple * cu_count()
    counts = torch.zeros(grid, dtype=torch.int32, device="cuda")
    where = torch.zeros(grid, 2, dtype=torch.int32, device="cuda")
    _check(handle().lds_poison_probe(word, grid, ticks, counts.data_ptr(), where.data_ptr(), _stream()), "lds_poison_probe")
    return counts, where


def cus_of(where):
    """The distinct CUs of a `where` array: (XCC id, shader engine / array / CU bits 8..15 of the hardware id)."""
    w = where.cpu().tolist()
    return {(int(x) & 0xF, (int(h) >> 8) & 0xFF) for x, h in w}


# ------------------------------------------------------------------------------------------------ the proxy

class LibProxy:
    """Stands in for the ctypes handle: every attribute is the handle's, a call of a launching entry point is preceded by
    `fill(word)`.  `fill` and `capturing` are injectable so that the order of events can be tested on a fake handle."""

    def __init__(self, real, word, names=None, fill=fill, capturing=_capturing):
        d = self.__dict__
        d["_real"], d["_word"], d["_fill"], d["_capturing"] = real, word, fill, capturing
        d["_names"] = frozenset(launching() if names is None else names)
        d["poisoned"] = set()

    def __setattr__(self, name, value):
        raise AttributeError("the library proxy is read-only")

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._names:
            return fn

        def poisoned_call(*args):
            if not self._capturing():
                self._fill(self._word)
                self.poisoned.add(name)
            return fn(*args)

        poisoned_call.__name__ = name
        return poisoned_call


@contextlib.contextmanager
def installed(pattern, real=None, names=None, **kw):
    """`diffews_amd._lib.lib` returns a LibProxy (byte `pattern` repeated into the word) until the block ends; yields the
    proxy.  `real` / `names`: another handle and its launching names (the planted defects)."""
    from diffews_amd import _lib
    proxy = LibProxy(_lib.lib() if real is None else real, word_of(pattern), names, **kw)
    saved = _lib.lib
    _lib.lib = lambda: proxy
    try:
        yield proxy
    finally:
        _lib.lib = saved


# ------------------------------------------------------------------------------------------------ the measurement

def measure(repetitions=10):
    """Prints what profiles/lds_poison.md records: distinct CUs per fill over grid multiples and stays, the time of one
    fill, and the share of probe workgroups that find all their words after a fill, per pattern."""
    import statistics

    import torch
    handle()
    cus = cu_count()
    print(f"{torch.cuda.get_device_name(0)}, {cus} CUs")
    for multiple in (1, 2, 4, 8):
        for ticks in (0, 100, 500, 2000):
            seen = []
            for _ in range(5):
                where = torch.full((multiple * cus, 2), -1, dtype=torch.int32, device="cuda")
                fill(word_of(0x7B), where=where, multiple=multiple, ticks=ticks)
                torch.cuda.synchronize()
                seen.append(len(cus_of(where)))
            print(f"coverage: {multiple} workgroups per CU, stay {ticks / 100:g} us: distinct CUs over 5 fills {seen}")
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(100):
        fill(0)
    t1.record()
    torch.cuda.synchronize()
    print(f"one fill (GRID_MULTIPLE {GRID_MULTIPLE}, STAY_TICKS {STAY_TICKS}): {t0.elapsed_time(t1) * 10:.1f} us")
    for pattern in PATTERNS:
        shares = []
        for _ in range(repetitions):
            fill(word_of(pattern))
            counts, _ = probe(word_of(pattern))
            torch.cuda.synchronize()
            shares.append(float((counts == LDS_WORDS).double().mean()))
        print(f"persistence 0x{pattern:02X}: share of probe workgroups with all {LDS_WORDS} words: min {min(shares):.4f} "
              f"median {statistics.median(shares):.4f} max {max(shares):.4f}")
    fill(word_of(0xFF))
    a = torch.randn(4096, 4096, device="cuda", dtype=torch.bfloat16)
    a @ a
    counts, _ = probe(word_of(0xFF))
    torch.cuda.synchronize()
    print(f"with a torch 4096^3 bf16 matmul between fill and probe: share of words still 0xFF {float(counts.double().mean()) / LDS_WORDS:.4f}")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    measure()
