"""Host-side op wrappers: torch tensors (device memory + current stream only) -> C-ABI calls.

Every function launches hand-written gfx950 kernels from libdiffews_hip.so on
`torch.cuda.current_stream()`; nothing here computes with PyTorch.  Activations are NHWC
(`[B, H, W, C]` or `[rows, C]`) in the engine storage dtype (bf16 or fp16).

The library checks scalars and the extents it is told; what it cannot know -- a tensor's dtype, layout, extent and
device -- is refused here, by one checker (`_Args`, shared with ops_bwd.py) and never by `assert`, so `python -O` changes
nothing.  Every tensor whose address reaches the library goes through it: dtype, layout (contiguous, or a unit last
stride where a wrapper takes row-strided views) and extent (the last element the kernel addresses through the pointer
lies inside the tensor).  A refusal is ValueError("<wrapper>: <argument> ..."); only _dt, _f32 and _rowbias keep their
TypeError.  The device rule comes last, after every shape and dtype refusal and before the stream is asked for: all
tensors of a call lie on ONE cuda device (workspaces are allocated there), the documented host mirrors (tab_host,
table_host, planes_host) on the host.  Whether that device is the current one is not checked.
"""
import ctypes as C
import os
import math

import torch

from . import _lib as L

_DT = {torch.bfloat16: L.BF16, torch.float16: L.F16}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"engine storage dtype must be bfloat16 or float16, got {t.dtype}")


def _f32(t, name):
    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous float32 tensor")
    return t


class _Args:
    """The argument checker of one wrapper call: `arg = _Args("wrapper")`, then arg(name, t, ...) per tensor,
    arg.need(condition, message) per relation between scalars and arg.device() last.  Every refusal is
    ValueError(f"{wrapper}: {name} ...").  Nothing here allocates."""
    __slots__ = ("fn", "dev", "first", "off")

    def __init__(self, fn):
        self.fn, self.dev, self.first, self.off = fn, None, None, None

    def need(self, ok, message, *values):
        """message.format(*values) is the refusal: formatted only when it is raised (sizes print as tuples)."""
        if not ok:
            raise ValueError(f"{self.fn}: " + message.format(*(tuple(v) if isinstance(v, torch.Size) else v for v in values)))

    def __call__(self, name, t, dtype=None, shape=None, dim=None, dense=True, elems=None, extent=None, host=False):
        """t's address, unless t is refused: `dtype` is one dtype, a tuple of them or None (the storage dtypes, left to
        _dt); `shape` the exact shape, `dim` the number of dimensions, `elems` the number of elements; dense=False takes
        any view with a unit last stride instead of a contiguous tensor; `extent` is the number of elements the kernel
        addresses from t's first one, which t must span.  host=True: a host mirror.  The device is only noted here."""
        ok = (dtype is None or t.dtype == dtype or (type(dtype) is tuple and t.dtype in dtype)) \
            and (shape is None or t.shape == shape) and (dim is None or t.dim() == dim) \
            and (elems is None or t.numel() == elems) and (t.is_contiguous() if dense else t.dim() > 0 and t.stride(-1) == 1)
        if ok and extent is not None:
            ok = extent <= (t.numel() if dense else _span(t))
        if not ok:
            kinds = " or ".join(str(d) for d in (dtype if type(dtype) is tuple else (dtype or "bfloat16 / float16",)))
            want = (("shape", shape and tuple(shape)), ("dimensions", dim), ("elements", elems), ("extent", extent))
            raise ValueError(f"{self.fn}: {name} must be a {'contiguous' if dense else 'unit-last-stride'} {kinds} tensor"
                             + "".join(f", {k} {v}" for k, v in want if v is not None)
                             + f"; got {t.dtype} {tuple(t.shape)} with strides {t.stride()}")
        d = t.device
        if host:
            if d.type != "cpu" and self.off is None:
                self.off = f"the host mirror {name} lies on {d}"
        elif self.dev is None:
            self.dev, self.first = d, name
        elif d != self.dev and self.off is None:
            self.off = f"{name} lies on {d}, {self.first} on {self.dev}"
        return t.data_ptr()

    def f32(self, name, t, n):
        """An optional fp32 vector of at least n elements (_f32 and its TypeError first): its address, None for None."""
        return None if t is None else self(name, _f32(t, name), torch.float32, extent=n)

    def device(self):
        """The last refusal of a wrapper: the device rule of the module docstring."""
        if self.off is None and self.dev is not None and self.dev.type != "cuda":
            self.off = f"{self.first} lies on {self.dev}"
        if self.off is not None:
            raise ValueError(f"{self.fn}: all tensors must be device tensors on one cuda device, host mirrors on the host; "
                             + self.off)


def _span(t):
    """Elements from t's first to its last one, in memory: what a kernel may address through t's pointer."""
    return 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride())) if t.numel() else 0


def _rowbias(arg, a, rb, imgs, N):
    """rowbias [imgs, N] fp32, rows may be strided (a column slice of a wider buffer)."""
    if rb is None:
        return
    if rb.dtype != torch.float32 or rb.dim() != 2 or rb.stride(1) != 1:
        raise TypeError("rowbias must be float32 [imgs, N] with unit column stride")
    arg.need(rb.shape[0] >= imgs and rb.shape[1] == N, "rowbias must be [{}, {}], got {}", imgs, N, rb.shape)
    a.rowbias, a.ld_rowbias = arg("rowbias", rb, torch.float32, dense=False), rb.stride(0)


# Optional per-launch timing hook (bench.py roofline leg): when set, every GEMM launch is bracketed
# by events on the launch stream and reported as hook(kernel_name, flops, start_event, end_event).
gemm_hook = None


def _gemm_call(a, device):
    lib = L.lib()
    if gemm_hook is not None:
        buf = C.create_string_buffer(64)
        L.check(lib.dfw_gemm_kernel_name(C.byref(a), buf, 64), "dfw_gemm_kernel_name")
        _timed(buf.value.decode(), 2.0 * a.M * a.N * a.K * max(1, a.batch),
               (a.M, a.N, a.K, a.taps, a.stride, a.ups, a.splitk, max(1, a.batch)), lambda: _gemm_launch(lib, a, device))
        return
    _gemm_launch(lib, a, device)


def _gemm_launch(lib, a, device):
    nbytes = lib.dfw_gemm_workspace_bytes(C.byref(a))   # 0 unless the plan uses split-K
    if nbytes:
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    L.check(lib.dfw_gemm(C.byref(a), _stream()), "dfw_gemm")
    return


def linear(x, w, bias=None, residual=None, rowbias=None, rows_per_img=0, act=L.ACT_NONE, geglu=False,
           out=None, out_f32=False, out_scale=1.0, splitk=None, colscale=None):
    """y[M, N] = epi(x[M, K] @ w[N, K]^T).  x may be a row-strided view ([M, K] with stride (ld, 1)).
    colscale = (n, s): output columns < n (a multiple of 64) are multiplied by s in fp32 before rounding."""
    arg = _Args("linear")
    arg("x", x, dim=2, dense=False)
    M, K = x.shape
    arg("w", w, x.dtype, dim=2)
    N = w.shape[0]
    arg.need(w.shape[1] == K, "w must be [N, {}] for x {}, got {}", K, x.shape, w.shape)
    n_out = N // 2 if geglu else N
    if out is None:
        out = torch.empty(M, n_out, dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    a = L.GemmArgs()
    a.A, a.W, a.C = x.data_ptr(), w.data_ptr(), arg("out", out, (x.dtype, torch.float32), (M, n_out), dense=False)
    a.bias = arg.f32("bias", bias, N)
    _rowbias(arg, a, rowbias, -(-M // rows_per_img) if rows_per_img else 1, N)
    if residual is not None:
        a.residual, a.ldr = arg("residual", residual, (x.dtype, torch.float32), (M, N), dense=False), residual.stride(0)
        a.residual_f32 = int(residual.dtype == torch.float32)   # the fp32 residual stream
    a.a_elems = (M - 1) * x.stride(0) + K
    a.w_elems = w.numel()
    a.M, a.N, a.K, a.lda, a.ldc = M, N, K, x.stride(0), out.stride(0)
    a.taps, a.Cin = 1, K
    a.rows_per_img = rows_per_img
    a.out_scale, a.act, a.geglu = out_scale, act, int(geglu)
    a.out_mode = L.OUT_F32 if out.dtype == torch.float32 else L.OUT_T
    a.splitk = 0 if splitk is None else splitk   # 0: the library plans tile + split-K
    a.batch, a.dtype = 1, _dt(x)
    if colscale is not None:
        a.colscale_n, a.colscale = int(colscale[0]), float(colscale[1])
    arg.device()
    _gemm_call(a, x.device)
    return out


def bmm_nt(x, w, out_f32=False, out_scale=1.0):
    """Batched y[b] = x[b] @ w[b]^T for contiguous x [Bt, M, K], w [Bt, N, K]."""
    arg = _Args("bmm_nt")
    arg("x", x, dim=3)
    Bt, M, K = x.shape
    arg("w", w, x.dtype, dim=3)
    N = w.shape[1]
    arg.need(w.shape[0] == Bt and w.shape[2] == K, "w must be [{}, N, {}], got {}", Bt, K, w.shape)
    out = torch.empty(Bt, M, N, dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    a = L.GemmArgs()
    a.A, a.W, a.C = x.data_ptr(), w.data_ptr(), out.data_ptr()
    a.a_elems, a.w_elems = M * K, N * K
    a.M, a.N, a.K, a.lda, a.ldc = M, N, K, K, N
    a.taps, a.Cin = 1, K
    a.out_scale = out_scale
    a.out_mode = L.OUT_F32 if out_f32 else L.OUT_T
    a.splitk, a.batch = 1, Bt
    a.strideA, a.strideW, a.strideC = M * K, N * K, M * N
    a.dtype = _dt(x)
    arg.device()
    _gemm_call(a, x.device)
    return out


def conv3x3(x, w, cout, bias=None, stride=1, pad=1, ups=False, rowbias=None, residual=None,
            out_nchw_f32=False, out_scale=1.0, splitk=None, gn_groups=0, gn_in=None, act=L.ACT_NONE,
            out_f32=False, w_blk=None):
    """3x3 conv on NHWC x [B, H, W, Cin] with w packed [Cout, 9*Cin] (ky, kx, cin order).
    w_blk: optional blocked copy of w (packing.block_conv3x3: [9][Cin/32][Cout][32]) for the kernels that stage W per
    (tap, 32-channel chunk): their LDS-DMA then fetches whole cache lines (dfw_gemm_args.W_blocked).
    pad = top/left zero padding (bottom/right come from bounds checks: pad=0,stride=2 is the VAE
    encoder's F.pad(0,1,0,1) + conv(stride 2, padding 0)); ups fuses nearest-2x upsampling.
    gn_in = (gamma, beta, groups, eps, silu): the conv's input is GroupNorm(+SiLU) of x, applied by dfw_groupnorm first
    (ResnetBlock2D's norm + nonlinearity + conv as one call; a kernel that normalised its input patch in LDS instead was
    built in rounds 1-3, never beat pass + conv, and is gone: DESIGN.md section 3).
    out_f32: NHWC fp32 output, and `residual` may be fp32 -- the fp32 residual stream (x + branch summed and stored
    in fp32; the conv's operands stay 16-bit)."""
    arg = _Args("conv3x3")
    arg("x", x, dim=4)
    B, Hi, Wi, Cin = x.shape
    if gn_in is not None:
        x = groupnorm(x, *gn_in, out_dtype=w.dtype)
    arg("w", w, x.dtype, (cout, 9 * Cin))
    if ups:
        arg.need(stride == 1 and pad == 1, "ups goes with stride 1 and pad 1, got stride {} and pad {}", stride, pad)
        Ho, Wo = 2 * Hi, 2 * Wi
    elif stride == 1:
        Ho, Wo = Hi, Wi
    else:
        Ho, Wo = (Hi + 2 * pad - 3) // stride + 1 if pad else Hi // 2, (Wi + 2 * pad - 3) // stride + 1 if pad else Wi // 2
    M = B * Ho * Wo
    if out_nchw_f32:
        out = torch.empty(B, cout, Ho, Wo, dtype=torch.float32, device=x.device)
    else:
        out = torch.empty(B, Ho, Wo, cout, dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    a = L.GemmArgs()
    a.A, a.W, a.C = x.data_ptr(), w.data_ptr(), out.data_ptr()
    if w_blk is not None:
        arg.need(Cin % 32 == 0, "w_blk needs Cin a multiple of 32, got {}", Cin)
        a.W_blocked = arg("w_blk", w_blk, w.dtype, elems=w.numel())
    a.bias = arg.f32("bias", bias, cout)
    _rowbias(arg, a, rowbias, B, cout)
    if residual is not None:
        a.residual, a.ldr = arg("residual", residual, (x.dtype, torch.float32), elems=M * cout), cout
        a.residual_f32 = int(residual.dtype == torch.float32)
    a.a_elems, a.w_elems = x.numel(), w.numel()
    a.M, a.N, a.K, a.lda, a.ldc = M, cout, 9 * Cin, Cin, cout
    a.taps, a.Cin, a.Hi, a.Wi, a.Ho, a.Wo = 9, Cin, Hi, Wi, Ho, Wo
    a.stride, a.pad, a.ups = stride, pad, int(ups)
    a.rows_per_img = Ho * Wo
    a.out_scale, a.act = out_scale, act
    a.out_mode = L.OUT_NCHW_F32 if out_nchw_f32 else (L.OUT_F32 if out_f32 else L.OUT_T)
    a.splitk = 0 if splitk is None else splitk
    a.batch, a.dtype = 1, _dt(x)
    stats = None
    arg.device()
    if gn_groups and not out_nchw_f32:
        # fused GroupNorm statistics of the output, when the planned kernel supports them
        a.gn_groups = gn_groups
        chunks = L.lib().dfw_gemm_gn_chunks(C.byref(a))
        if chunks > 0:
            part = torch.empty(B, chunks, gn_groups, 2, dtype=torch.float32, device=x.device)
            a.gn_partial = part.data_ptr()
            stats = (part, chunks, gn_groups)
    _gemm_call(a, x.device)
    if stats is not None:
        out._gn_stats = stats   # consumed by groupnorm(out, ...) -- valid while `out` is not modified
    return out


def _timed(name, flops, shape, call):
    """call() bracketed by two events on the launch stream and reported as gemm_hook(name, flops, start, end, shape)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    gemm_hook(name, flops, e0, e1, shape)


def _fsa_args(arg, q, k, v, out, heads):
    """(FsaArgs with the q / k / v / out fields and the dtype filled, out): q / k / v [B, N, heads*64] views with unit
    channel stride, `out` [B, N, heads*64] with dense rows, allocated when None."""
    arg("q", q, dim=3, dense=False)
    B, N, Cq = q.shape
    arg.need(Cq == heads * 64, "q must be [B, N, {}] for {} heads, got {}", heads * 64, heads, q.shape)
    arg("k", k, q.dtype, dim=3, dense=False)
    arg.need(k.shape[0] == B and k.shape[2] == Cq, "k must be [{}, keys, {}], got {}", B, Cq, k.shape)
    arg("v", v, q.dtype, k.shape, dense=False)
    if out is None:
        out = torch.empty(B, N, Cq, dtype=q.dtype, device=q.device)
    arg("out", out, q.dtype, (B, N, Cq), dense=False)
    arg.need(out.stride(1) == Cq, "out must have dense rows (stride {}), got strides {}", Cq, out.stride())
    a = L.FsaArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.batch, a.heads, a.n_q, a.n_kv = B, heads, N, k.shape[1]
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(1), k.stride(1), v.stride(1), Cq
    a.q_bs, a.k_bs, a.v_bs, a.o_bs = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.dtype = _dt(q)
    return a, out


def _fsa_bank(arg, a, q, k_bank, v_bank, nshot, images, count):
    """The bank fields of an FsaArgs from _fsa_args: k_bank / v_bank [images, Nb, heads*64] views in q's dtype, `images`
    of them (None: any number), which `count` words in the refusal."""
    arg.need(k_bank is not None and v_bank is not None, "a bank launch (nshot > 0) needs k_bank and v_bank")
    arg("k_bank", k_bank, q.dtype, dim=3, dense=False)
    arg.need(k_bank.shape[2] == q.shape[2], "k_bank must be [images, Nb, {}], got {}", q.shape[2], k_bank.shape)
    arg.need(images is None or k_bank.shape[0] == images, "k_bank must hold {} images ({}), got {}", images, count, k_bank.shape[0])
    arg("v_bank", v_bank, q.dtype, k_bank.shape, dense=False)
    a.k_bank, a.v_bank = k_bank.data_ptr(), v_bank.data_ptr()
    a.n_bank, a.nshot = k_bank.shape[1], nshot
    a.ldkb, a.ldvb, a.kb_bs, a.vb_bs = k_bank.stride(1), v_bank.stride(1), k_bank.stride(0), v_bank.stride(0)


def _fsa_launch(a, q, nbytes, call, keys):
    """call() with `nbytes` of key-split scratch behind a.workspace; keys() -- the keys the launch's B * n_q query rows read
    in all -- is evaluated for the hook only (bench.py roofline leg: QK^T + PV flops of this launch)."""
    if nbytes:
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    if gemm_hook is None:
        return call()
    n = keys()
    _timed("fsa_attention", 4.0 * a.heads * 64 * a.n_q * n, (a.batch, a.heads, a.n_q, n), call)


def fsa_attention(q, k, v, heads, k_bank=None, v_bank=None, nshot=0, scale=None, out=None, n_plain=0,
                  q_prescaled=False, lse=None, key_split=True, bank_shared=False, _group=0, _shots=None):
    """KV-fusion self-attention.  q/k/v: [B, N, heads*64] views (token stride = stride(1));
    k_bank/v_bank: [(B-n_plain)*nshot, Nb, heads*64] views written by the support pass.
    n_plain: the first n_plain batch entries ignore the bank (lock-step [support ; query] launch).
    q_prescaled: q already carries scale * log2(e) (linear(..., colscale=(C, FSA_QSCALE))).
    key_split: let the library split the bank readers' key range over several workgroups when that balances the launch
    (many shots; needs a scratch buffer, allocated here).
    bank_shared: k_bank/v_bank hold ONE support set, [nshot, Nb, heads*64], and every batch entry attends over
    [own ; that set] (a prepared SupportBank read by a batch of queries) -- same kernel, same key order as the bank
    repeated B times."""
    arg = _Args("fsa_attention")
    a, out = _fsa_args(arg, q, k, v, out, heads)
    B, N = q.shape[:2]
    if nshot:
        arg.need(n_plain == 0 or not (bank_shared or _group), "a shared bank or a stack of sets takes no plain entries, got n_plain {}", n_plain)
        arg.need(not (bank_shared and _group), "bank_shared does not go with a stack of sets")
        arg.need(not _group or B % _group == 0, "the batch of {} is not a multiple of the group of {}", B, _group)
        if _shots is not None:      # fsa_attention_ragged: nshot is max(shots)
            arg.need(_group, "a shot count per set needs a group")
            shots_c = (C.c_int32 * len(_shots))(*_shots)
            images, count = sum(_shots), "the sum of shots"
        elif _group:      # fsa_attention_sets
            images, count = (B // _group) * nshot, "nshot for each of the B // group sets"
        elif bank_shared:
            images, count = nshot, "nshot, one shared set"
        else:
            images, count = (B - n_plain) * nshot, "nshot for each of the B - n_plain entries"
        _fsa_bank(arg, a, q, k_bank, v_bank, nshot, images, count)
        a.bank_shared = int(bool(bank_shared))
    elif bank_shared:
        raise ValueError("bank_shared needs a bank (nshot > 0)")
    a.scale = scale if scale is not None else 64 ** -0.5
    a.n_plain, a.q_prescaled = n_plain, int(bool(q_prescaled))
    if lse is not None:   # training: per-row log2-sum-exp2 for the backward
        a.lse = arg("lse", lse, torch.float32, (B, heads, N))
    arg.device()
    if _shots is not None:
        call = lambda: _fsa_ragged_call(a, shots_c, len(_shots), _group)
        nbytes = L.lib().dfw_fsa_ragged_workspace_bytes(C.byref(a), shots_c, len(_shots), _group) if key_split else 0
    else:
        call = (lambda: _fsa_sets_call(a, _group)) if _group else (lambda: _fsa_call(a))
        nbytes = L.lib().dfw_fsa_workspace_bytes(C.byref(a)) if (nshot >= 2 and key_split) else 0   # key split of the bank readers (many shots)
    if _shots is not None:
        keys = lambda: B * k.shape[1] + _group * sum(_shots) * k_bank.shape[1]
    else:
        keys = lambda: n_plain * k.shape[1] + (B - n_plain) * (k.shape[1] + (nshot * k_bank.shape[1] if nshot else 0))
    _fsa_launch(a, q, nbytes, call, keys)
    return out


def _fsa_call(a):
    L.check(L.lib().dfw_fsa_attention(C.byref(a), _stream()), "dfw_fsa_attention")


def _fsa_sets_call(a, group):
    L.check(L.lib().dfw_fsa_attention_sets(C.byref(a), group, _stream()), "dfw_fsa_attention_sets")


def fsa_attention_sets(q, k, v, heads, k_bank, v_bank, nshot, group, scale=None, out=None, q_prescaled=False,
                       lse=None, key_split=True):
    """KV-fusion self-attention of a class-major batch against a STACK of support sets: q/k/v [B, N, heads*64],
    k_bank/v_bank [(B // group) * nshot, Nb, heads*64]; entries [j*group, (j+1)*group) attend over [own ; set j]
    (bank image = (entry // group) * nshot + shot).  Same kernel, plan and workspace as fsa_attention on the bank
    materialised per entry; group == 1 is that launch, group == B with one set reads like bank_shared."""
    if not nshot or nshot < 1 or group < 1:
        raise ValueError("fsa_attention_sets needs a bank (nshot >= 1) and group >= 1")
    return fsa_attention(q, k, v, heads, k_bank, v_bank, nshot=nshot, scale=scale, out=out, q_prescaled=q_prescaled,
                         lse=lse, key_split=key_split, _group=int(group))


def _fsa_ragged_call(a, shots, nsets, group):
    L.check(L.lib().dfw_fsa_attention_ragged(C.byref(a), shots, nsets, group, _stream()), "dfw_fsa_attention_ragged")


def fsa_attention_ragged(q, k, v, heads, k_bank, v_bank, shots, group, scale=None, out=None, q_prescaled=False,
                         lse=None, key_split=True):
    """fsa_attention_sets with a shot count per set: `shots` a sequence of B // group counts (each >= 1), k_bank/v_bank
    [sum(shots), Nb, heads*64] with the sets packed set-major; entries [j*group, (j+1)*group) attend over
    [own ; the shots[j] images of set j].  Per set the kernel arithmetic, key order and tile sequence of fsa_attention on
    that set's slice with bank_shared=True; with all counts equal it is fsa_attention_sets bit for bit.  The key split
    never exceeds 1 + min(shots)."""
    shots = [int(s) for s in shots]
    if group < 1 or not shots or min(shots) < 1:
        raise ValueError("fsa_attention_ragged needs group >= 1 and a count >= 1 for every set")
    if len(shots) * int(group) != q.shape[0]:
        raise ValueError(f"{len(shots)} sets of {group} entries are not the batch of {q.shape[0]}")
    return fsa_attention(q, k, v, heads, k_bank, v_bank, nshot=max(shots), scale=scale, out=out, q_prescaled=q_prescaled,
                         lse=lse, key_split=key_split, _group=int(group), _shots=shots)


def _fsa_routed_call(a, table, table_host, nbank, min_shots):
    L.check(L.lib().dfw_fsa_attention_routed(C.byref(a), table, table_host, nbank, min_shots, _stream()),
            "dfw_fsa_attention_routed")


def fsa_attention_routed(q, k, v, heads, k_bank, v_bank, table, table_host, max_shots, min_shots, q_prescaled=False,
                         key_split=True, out=None):
    """KV-fusion self-attention of a batch in which every entry reads a support set of its own out of a STACK of bank
    images: q/k/v [B, N, heads*64], k_bank/v_bank [nbank, Nb, heads*64], `table` a DEVICE int32 [B, 2] tensor whose row e =
    (first image, shots) of entry e -- entry e attends over [own ; images first_e .. first_e + shots_e - 1].  The kernel
    reads the table when it runs: under stream capture one graph serves every table written into the same tensor.
    `table_host` is its int32 host mirror, validated by the library before the launch (every count within
    [min_shots, max_shots], every set inside the stack).  The launch plan and workspace depend on the shapes, max_shots
    and min_shots only; the key split never exceeds 1 + min_shots.  Per entry the kernel arithmetic, key order and tile
    sequence of fsa_attention on that set's slice with bank_shared=True."""
    arg = _Args("fsa_attention_routed")
    a, out = _fsa_args(arg, q, k, v, out, heads)
    B = q.shape[0]
    host = C.cast(arg("table_host", table_host, torch.int32, (B, 2), host=True), C.POINTER(C.c_int32))
    arg("table", table, torch.int32, (B, 2))
    _fsa_bank(arg, a, q, k_bank, v_bank, int(max_shots), None, None)
    a.scale, a.q_prescaled = 64 ** -0.5, int(bool(q_prescaled))
    nbank, min_shots = int(k_bank.shape[0]), int(min_shots)
    arg.device()
    nbytes = L.lib().dfw_fsa_routed_workspace_bytes(C.byref(a), nbank, min_shots) if key_split else 0
    _fsa_launch(a, q, nbytes, lambda: _fsa_routed_call(a, table.data_ptr(), host, nbank, min_shots),
                lambda: B * k.shape[1] + int(table_host[:, 1].sum()) * k_bank.shape[1])
    return out


def zeros(shape, dtype, device="cuda"):
    """torch.zeros whose fill is a library kernel (capture-safe: no memset node).  Sizes are padded to 16 bytes."""
    n = 1
    for d in shape:
        n *= int(d)
    esz = torch.empty(0, dtype=dtype).element_size()
    pad = (-(n * esz)) % 16 // esz if (n * esz) % 16 else 0
    buf = torch.empty(n + pad, dtype=dtype, device=device)
    L.check(L.lib().dfw_zero(buf.data_ptr(), (n + pad) * esz, _stream()), "dfw_zero")
    return buf[:n].view(*shape)


def split_storage(x, dtype):
    """fp32 x -> (hi, lo) in `dtype` with hi + lo = x to ~2^-22 relative (fp16): see linear_stream / conv3x3_stream."""
    arg = _Args("split_storage")
    arg("x", x, torch.float32)
    arg.need(x.numel() % 8 == 0, "x must hold a multiple of 8 elements, got {}", x.numel())
    arg.device()
    hi = torch.empty(x.shape, dtype=dtype, device=x.device)
    lo = torch.empty(x.shape, dtype=dtype, device=x.device)
    L.check(L.lib().dfw_split_f32(x.data_ptr(), hi.data_ptr(), lo.data_ptr(), x.numel(), _DT[dtype], _stream()), "dfw_split_f32")
    return hi, lo


def linear_stream(x, w, bias=None, residual=None):
    """Linear whose INPUT is the residual stream (ResnetBlock2D.conv_shortcut).  16-bit stream: plain linear.  fp32 stream:
    x is fed as two 16-bit operands (hi, lo = split_storage(x)); the second GEMM adds onto the first through the fp32 residual
    epilogue, so the stream's 16-bit rounding never enters the fp32 result."""
    if x.dtype != torch.float32:
        return linear(x, w, bias=bias, residual=residual)
    hi, lo = split_storage(x, w.dtype)
    y = linear(hi, w, bias=bias, residual=residual, out_f32=True)
    return linear(lo, w, residual=y, out_f32=True)


def conv3x3_stream(x, w, cout, bias=None, lo=True, w_up2x=None, **kw):
    """conv3x3 whose INPUT is the residual stream (Downsample2D / Upsample2D convs): as linear_stream.
    w_up2x (with ups=True): the folded pack of w (packing.fold_up2x).  A 16-bit stream then takes conv3x3_up2x where the
    library accepts the shape (Hi, Wi multiples of 16, Cin and Cout of 64) and UP2X_FOLD is on; the fp32 stream, small maps
    and every other caller run the unfolded conv below, unchanged.
    lo=False: the fp32 stream is fed as ONE operand rounded once (no second GEMM, a convert instead of the split): each such
    conv adds one storage rounding of its input (2.5e-4 relative in fp16, in quadrature) -- the VAE encoder's two LARGEST
    downsample convs take this form (round 4): they were 2.2 ms of the parity mode for 0.8e-4 of its 7.5e-4."""
    if x.dtype != torch.float32:
        if w_up2x is not None and UP2X_FOLD and kw.get("ups") and set(kw) <= {"ups", "gn_groups"}:
            y = conv3x3_up2x(x, w_up2x, cout, bias=bias, gn_groups=kw.get("gn_groups", 0))
            if y is not None:
                return y
        return conv3x3(x, w, cout, bias=bias, **kw)
    if not lo:
        return conv3x3(to_storage(x, w.dtype), w, cout, bias=bias, out_f32=True, **kw)
    hi, lo = split_storage(x, w.dtype)
    gn_groups = kw.pop("gn_groups", 0)
    y = conv3x3(hi, w, cout, bias=bias, out_f32=True, **kw)
    return conv3x3(lo, w, cout, residual=y, out_f32=True, gn_groups=gn_groups, **kw)     # the FINAL values carry the statistics


# A/B switch of the folded upsample conv: False keeps conv3x3_stream(..., ups=True, w_up2x=...) on the unfolded route (dfw_gemm,
# ups = 1) everywhere.
UP2X_FOLD = True


def conv3x3_up2x(x, w_folded, cout, bias=None, gn_groups=0):
    """Upsample2D's nearest-2x + conv3x3 on NHWC x [B, Hi, Wi, Cin] as four 2x2 parity convs on x itself (dfw_conv_up2x):
    w_folded [Cout, 16*Cin] from packing.fold_up2x.  Returns [B, 2Hi, 2Wi, Cout] with `_gn_stats` attached as conv3x3 does,
    or None when the library declines the shape (its name query answers DFW_ESHAPE): the caller then runs
    conv3x3(..., ups=True) on the unfolded weights.  The hook sees the FLOPs executed, 2 M N 4 Cin."""
    arg = _Args("conv3x3_up2x")
    arg("x", x, dim=4)
    B, Hi, Wi, Cin = x.shape
    arg("w_folded", w_folded, x.dtype, (cout, 16 * Cin))
    out = torch.empty(B, 2 * Hi, 2 * Wi, cout, dtype=x.dtype, device=x.device)
    a = L.ConvUp2xArgs()
    a.x, a.W, a.y = x.data_ptr(), w_folded.data_ptr(), out.data_ptr()
    a.bias = arg.f32("bias", bias, cout)
    a.x_elems, a.w_elems = x.numel(), w_folded.numel()
    a.B, a.Hi, a.Wi, a.Cin, a.Cout, a.ldx, a.ldy = B, Hi, Wi, Cin, cout, Cin, cout
    a.dtype = _dt(x)
    arg.device()
    lib = L.lib()
    name = C.create_string_buffer(64)
    rc = lib.dfw_conv_up2x_kernel_name(C.byref(a), name, 64)
    if rc == -2:      # DFW_ESHAPE
        return None
    L.check(rc, "dfw_conv_up2x_kernel_name")
    stats = None
    if gn_groups:
        a.gn_groups = gn_groups
        chunks = lib.dfw_conv_up2x_gn_chunks(C.byref(a))
        if chunks > 0:
            part = torch.empty(B, chunks, gn_groups, 2, dtype=torch.float32, device=x.device)
            a.gn_partial = part.data_ptr()
            stats = (part, chunks, gn_groups)
    call = lambda: L.check(lib.dfw_conv_up2x(C.byref(a), _stream()), "dfw_conv_up2x")
    if gemm_hook is not None:
        M = B * 4 * Hi * Wi
        _timed(name.value.decode(), 2.0 * M * cout * 4 * Cin, (M, cout, 4 * Cin, 4, 1, 1, 1, 1), call)
    else:
        call()
    if stats is not None:
        out._gn_stats = stats
    return out


FSA_QSCALE = 64 ** -0.5 * math.log2(math.e)   # attn.scale (A:269-271, head_dim 64) in exp2 units


VATTN_QSCALE = 512 ** -0.5 * math.log2(math.e)   # the VAE mid-block attention's scale (one head of dim 512) in exp2 units


def vae_attention(q, k, v, out=None):
    """Flash attention of the VAE mid-block: q / k / v [B, N, 512] views (column slices of one fused QKV buffer), ONE head of
    dim 512, q pre-multiplied by VATTN_QSCALE (linear(..., colscale=(512, VATTN_QSCALE))).  The N x N scores stay on chip."""
    arg = _Args("vae_attention")
    arg("q", q, dim=3, dense=False)
    B, N, D = q.shape
    arg.need(D == 512, "q must be [B, N, 512], got {}", q.shape)
    arg("k", k, q.dtype, q.shape, dense=False)
    arg("v", v, q.dtype, q.shape, dense=False)
    if out is None:
        out = torch.empty(B, N, D, dtype=q.dtype, device=q.device)
    arg("out", out, q.dtype, q.shape, dense=False)
    a = L.VattnArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.batch, a.n, a.head_dim, a.q_prescaled = B, N, D, 1
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(1), k.stride(1), v.stride(1), out.stride(1)
    a.q_bs, a.k_bs, a.v_bs, a.o_bs = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.dtype = _dt(q)
    arg.device()
    L.check(L.lib().dfw_vae_attention(C.byref(a), _stream()), "dfw_vae_attention")
    return out


def cross_attention(q, k, v, heads, scale=None):
    """q [B, N, heads*64]; k/v [B, L, heads*64] views (short context)."""
    arg = _Args("cross_attention")
    arg("q", q, dim=3, dense=False)
    B, N, Cq = q.shape
    arg.need(Cq == heads * 64, "q must be [B, N, {}] for {} heads, got {}", heads * 64, heads, q.shape)
    arg("k", k, q.dtype, dim=3, dense=False)
    arg.need(k.shape[0] == B and k.shape[2] == Cq, "k must be [{}, L, {}], got {}", B, Cq, k.shape)
    arg("v", v, q.dtype, k.shape, dense=False)
    out = torch.empty(B, N, Cq, dtype=q.dtype, device=q.device)
    a = L.XattnArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.batch, a.heads, a.n_q, a.L = B, heads, N, k.shape[1]
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(1), k.stride(1), v.stride(1), Cq
    a.q_bs, a.k_bs, a.v_bs, a.o_bs = q.stride(0), k.stride(0), v.stride(0), N * Cq
    a.scale = scale if scale is not None else 64 ** -0.5
    a.dtype = _dt(q)
    arg.device()
    L.check(L.lib().dfw_cross_attention(C.byref(a), _stream()), "dfw_cross_attention")
    return out


def groupnorm(x, gamma, beta, groups, eps, silu=False, return_stats=False, out_dtype=None):
    """GroupNorm (+SiLU) over NHWC x [B, H, W, C] (or [B, HW, C]).
    return_stats: also return the (mean, rstd) [B, groups, 2] fp32 the kernel normalised with (training).
    x may be fp32 (the fp32 residual stream): the output is then `out_dtype` (bf16 / fp16, required)."""
    arg = _Args("groupnorm")
    arg("x", x, (*_DT, torch.float32))
    arg.need(x.dim() >= 2 and x.numel() > 0, "x must be [B, ..., C] and not empty, got {}", x.shape)
    xf32 = x.dtype == torch.float32
    if xf32 and out_dtype not in _DT:
        raise TypeError("groupnorm of an fp32 tensor needs out_dtype=torch.bfloat16 / torch.float16")
    odt = out_dtype if xf32 else x.dtype
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc)
    a = L.GroupNormArgs()
    a.gamma, a.beta = arg.f32("gamma", gamma, Cc), arg.f32("beta", beta, Cc)
    arg.device()
    y = torch.empty(x.shape, dtype=odt, device=x.device)
    a.x, a.y = x.data_ptr(), y.data_ptr()
    a.B, a.HW, a.C, a.groups, a.ldx, a.ldy = B, HW, Cc, groups, Cc, Cc
    a.eps, a.silu, a.dtype, a.x_f32 = eps, int(silu), _DT[odt], int(xf32)
    st = getattr(x, "_gn_stats", None)
    if st is not None and st[2] == groups and st[0].shape[0] == B:
        a.pre_partial, a.pre_chunks = st[0].data_ptr(), st[1]
    lib = L.lib()
    nbytes = lib.dfw_groupnorm_workspace_bytes(C.byref(a))
    if nbytes == 0:
        L.check(L.lib().dfw_groupnorm(C.byref(a), _stream()), "dfw_groupnorm")  # reports the shape error
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    a.stats_ws, a.stats_ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.dfw_groupnorm(C.byref(a), _stream()), "dfw_groupnorm")
    if return_stats:
        return y, ws[ws.numel() - B * groups * 2:].view(B, groups, 2)
    return y


def layernorm(x, gamma, beta, eps=1e-5, out_dtype=None):
    """x may be fp32 (the fp32 residual stream inside a transformer block): the output is then `out_dtype`."""
    arg = _Args("layernorm")
    arg("x", x, (*_DT, torch.float32), dim=2, dense=False)
    xf32 = x.dtype == torch.float32
    if xf32 and out_dtype not in _DT:
        raise TypeError("layernorm of an fp32 tensor needs out_dtype=torch.bfloat16 / torch.float16")
    odt = out_dtype if xf32 else x.dtype
    a = L.LayerNormArgs()
    a.gamma, a.beta = arg.f32("gamma", gamma, x.shape[1]), arg.f32("beta", beta, x.shape[1])
    arg.device()
    y = torch.empty(x.shape, dtype=odt, device=x.device)
    a.x, a.y = x.data_ptr(), y.data_ptr()
    a.rows, a.C, a.ldx, a.ldy, a.eps, a.dtype = x.shape[0], x.shape[1], x.stride(0), y.stride(0), eps, _DT[odt]
    a.x_f32 = int(xf32)
    L.check(L.lib().dfw_layernorm(C.byref(a), _stream()), "dfw_layernorm")
    return y


def conv_small(x, w, bias, cout, taps, dtype, nchw_f32_out=False, in_scale=1.0, out_scale=1.0, gn_groups=0,
               out=None, gn_part=None, out_f32=False):
    """Boundary conv with Cin <= 8: x NCHW fp32 [B, Cin, H, W], w fp32 [Cout, taps, Cin].
    gn_groups: also emit the GroupNorm partial sums of the output where the kernel supports it (y._gn_stats).
    x may be a list/tuple of up to three such tensors (same Cin, H, W): the batch is their concatenation,
    read in place (no torch.cat).
    out: write into this tensor instead of allocating -- NHWC: a batch slice of a larger contiguous buffer;
    NCHW fp32: a view [B, cout, H, W] whose channel planes are contiguous (a channel slice of a wider NCHW
    tensor is fine: the batch stride travels as y_bstride).  gn_part: the matching [B, chunks, groups, 2]
    slice of a larger partial-sum buffer (several conv_small calls filling one batch)."""
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    arg = _Args("conv_small")
    arg.need(1 <= len(xs) <= 3, "x is one tensor or a list of up to three, got {}", len(xs))
    for i, t in enumerate(xs):
        arg(f"x[{i}]", t, torch.float32, dim=4)
        arg.need(t.shape[1:] == xs[0].shape[1:], "x[{}] must be shaped like x[0] {} behind the batch, got {}", i, xs[0].shape, t.shape)
    x = xs[0]
    _, Cin, H, W = x.shape
    B = sum(t.shape[0] for t in xs)
    arg("w", w, torch.float32, elems=cout * taps * Cin)
    a = L.ConvSmallArgs()
    if len(xs) > 1:
        a.x1, a.b0 = xs[1].data_ptr(), xs[0].shape[0]
        a.b1 = a.b0 + xs[1].shape[0]
        if len(xs) > 2:
            a.x2 = xs[2].data_ptr()
    if nchw_f32_out:
        y = out if out is not None else torch.empty(B, cout, H, W, dtype=torch.float32, device=x.device)
        arg("out", y, torch.float32, (B, cout, H, W), dense=False)
        arg.need(y.stride(2) == W and y.stride(1) == H * W, "out must have contiguous channel planes, got strides {}", y.stride())
        a.y_bstride = y.stride(0) if B > 1 else cout * H * W
    else:   # NHWC: storage dtype, or fp32 (out_f32: the fp32 residual stream starts at conv_in)
        ydt = torch.float32 if out_f32 else dtype
        y = out if out is not None else torch.empty(B, H, W, cout, dtype=ydt, device=x.device)
        arg("out", y, ydt, (B, H, W, cout))
    a.x, a.W, a.bias, a.y = x.data_ptr(), w.data_ptr(), arg.f32("bias", bias, cout), y.data_ptr()
    a.B, a.Cin, a.H, a.Wd, a.Cout, a.taps, a.ldy = B, Cin, H, W, cout, taps, cout
    a.in_scale, a.out_scale = in_scale, out_scale
    a.out_mode = L.OUT_NCHW_F32 if nchw_f32_out else (L.OUT_F32 if out_f32 else L.OUT_T)
    a.dtype = _DT[dtype]
    stats = None
    if gn_part is not None:      # its chunk count is the library's to name: compared below, after the query
        arg("gn_part", gn_part, torch.float32, (B, gn_part.shape[1] if gn_part.dim() == 4 else 0, gn_groups, 2))
    arg.device()
    if gn_groups and not nchw_f32_out and not out_f32:
        a.gn_groups = gn_groups
        chunks = L.lib().dfw_conv_small_gn_chunks(C.byref(a))
        if chunks > 0:
            part = gn_part if gn_part is not None else torch.empty(B, chunks, gn_groups, 2, dtype=torch.float32, device=x.device)
            arg.need(part.shape == (B, chunks, gn_groups, 2), "gn_part must be [{}, {}, {}, 2], got {}", B, chunks, gn_groups, part.shape)
            a.gn_partial = part.data_ptr()
            stats = (part, chunks, gn_groups)
    L.check(L.lib().dfw_conv_small(C.byref(a), _stream()), "dfw_conv_small")
    if stats is not None:
        y._gn_stats = stats
    return y


def conv_small_gn_chunks(x_shape, cout, taps, dtype, gn_groups):
    """Chunks per image of conv_small's fused GroupNorm partial sums for this shape (0: unsupported)."""
    B, Cin, H, W = x_shape
    a = L.ConvSmallArgs()
    a.B, a.Cin, a.H, a.Wd, a.Cout, a.taps, a.ldy = B, Cin, H, W, cout, taps, cout
    a.out_mode, a.dtype, a.gn_groups = L.OUT_T, _DT[dtype], gn_groups
    a.x = 16    # alignment of the input pointer is part of the kernel choice: torch allocations are 16-byte aligned
    return L.lib().dfw_conv_small_gn_chunks(C.byref(a))


def meter_update(counts, class_id, inter_buf, union_buf):
    """AverageMeter.update on device: int64 atomics into the two [2, nclass] buffers (logger.py:35-37)."""
    arg = _Args("meter_update")
    arg("counts", counts, torch.int64, dim=2)
    arg.need(counts.shape[1] == 4, "counts must be [B, 4], got {}", counts.shape)
    arg("class_id", class_id, torch.int64, elems=counts.shape[0])
    arg("inter_buf", inter_buf, torch.int64, dim=2)
    arg.need(inter_buf.shape[0] == 2, "inter_buf must be [2, nclass], got {}", inter_buf.shape)
    arg("union_buf", union_buf, torch.int64, inter_buf.shape)
    arg.device()
    L.check(L.lib().dfw_meter_update(counts.data_ptr(), class_id.data_ptr(), inter_buf.data_ptr(), union_buf.data_ptr(),
                                     counts.shape[0], inter_buf.shape[1], _stream()), "dfw_meter_update")


def softmax_rows(x, dtype, scale=1.0):
    arg = _Args("softmax_rows")
    arg("x", x, torch.float32)
    arg.need(x.dim() >= 1 and x.numel() > 0, "x must be [..., L] and not empty, got {}", x.shape)
    arg.device()
    Lr = x.shape[-1]
    rows = x.numel() // Lr
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    L.check(L.lib().dfw_softmax_rows(x.data_ptr(), y.data_ptr(), rows, Lr, scale, _DT[dtype], _stream()),
            "dfw_softmax_rows")
    return y


def softmax_groups(x, groups, L_, dtype):
    """x [rows, ld] fp32 scores -> [rows, ld] `dtype`: softmax over each group's L entries, padding zeroed."""
    arg = _Args("softmax_groups")
    arg("x", x, torch.float32, dim=2)
    arg.device()
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    L.check(L.lib().dfw_softmax_groups(x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], groups, L_,
                                       _DT[dtype], _stream()), "dfw_softmax_groups")
    return y


def transpose(x):
    arg = _Args("transpose")
    arg("x", x, dim=3)
    Bt, R, Cc = x.shape
    dt = _dt(x)
    arg.device()
    y = torch.empty(Bt, Cc, R, dtype=x.dtype, device=x.device)
    L.check(L.lib().dfw_transpose(x.data_ptr(), y.data_ptr(), Bt, R, Cc, dt, _stream()), "dfw_transpose")
    return y


def concat_channels(a, b):
    arg = _Args("concat_channels")
    arg("a", a, (*_DT, torch.float32))
    arg.need(a.dim() >= 1 and a.numel() > 0, "a must be [..., Ca] and not empty, got {}", a.shape)
    arg("b", b, a.dtype, dim=a.dim())
    arg.need(a.shape[:-1] == b.shape[:-1], "b must be shaped like a {} up to the last dimension, got {}", a.shape, b.shape)
    arg.device()
    Ca, Cb = a.shape[-1], b.shape[-1]
    y = torch.empty(*a.shape[:-1], Ca + Cb, dtype=a.dtype, device=a.device)
    rows = a.numel() // Ca
    if a.dtype == torch.float32:   # fp32 residual stream: a byte copy -- C fp32 channels are 2C 16-bit units to the kernel
        L.check(L.lib().dfw_concat_channels(a.data_ptr(), b.data_ptr(), y.data_ptr(), rows, 2 * Ca, 2 * Cb, L.BF16, _stream()),
                "dfw_concat_channels")
        return y
    L.check(L.lib().dfw_concat_channels(a.data_ptr(), b.data_ptr(), y.data_ptr(), rows, Ca, Cb, _dt(a), _stream()),
            "dfw_concat_channels")
    return y


def to_storage(x, dtype):
    """fp32 -> storage dtype copy (the 16-bit MFMA-operand view of an fp32 residual-stream tensor); identity for a
    tensor that already is `dtype`."""
    if x.dtype == dtype:
        return x
    arg = _Args("to_storage")
    arg("x", x, torch.float32)
    arg.need(x.numel() % 8 == 0, "x must hold a multiple of 8 elements, got {}", x.numel())
    arg.device()
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    L.check(L.lib().dfw_convert_f32(x.data_ptr(), y.data_ptr(), x.numel(), _DT[dtype], _stream()), "dfw_convert_f32")
    return y


def timestep_embedding(timesteps, dim, dtype, flip_sin_to_cos=True, freq_shift=0.0):
    arg = _Args("timestep_embedding")
    arg("timesteps", timesteps, torch.float32, dim=1)
    arg.device()
    out = torch.empty(timesteps.shape[0], dim, dtype=dtype, device=timesteps.device)
    L.check(L.lib().dfw_timestep_embedding(timesteps.data_ptr(), out.data_ptr(), timesteps.shape[0], dim,
                                           int(flip_sin_to_cos), float(freq_shift), _DT[dtype], _stream()),
            "dfw_timestep_embedding")
    return out


def seg_postprocess(x, gt=None, r_threshold=0.25, threshold=0.0, batch_max=False, u8_out=None, counts_out=None,
                    scratch=None):
    """x: decoder output [B, 3, H, W] fp32 -> (uint8 [B,3,H,W], counts int64 [B,4] or None).
    r_threshold > 0: dynamic threshold r_threshold * max (per image, or over the batch tensor when
    batch_max -- main_oss.py:131 read literally); else the fixed `threshold` (main_oss.py:134-135)."""
    arg = _Args("seg_postprocess")
    arg("x", x, torch.float32, dim=4)
    B, _, H, W = x.shape
    arg.need(x.shape[1] == 3, "x must be [B, 3, H, W], got {}", x.shape)
    u8 = u8_out if u8_out is not None else torch.empty(B, 3, H, W, dtype=torch.uint8, device=x.device)
    arg("u8_out", u8, torch.uint8, (B, 3, H, W))
    if scratch is None:
        scratch = torch.empty(B, dtype=torch.int32, device=x.device)
    arg("scratch", scratch, torch.int32, extent=B)
    counts = None
    if gt is not None:
        arg("gt", gt, torch.uint8, (B, H, W))
        counts = counts_out if counts_out is not None else torch.empty(B, 4, dtype=torch.int64, device=x.device)
        arg("counts_out", counts, torch.int64, (B, 4))
    arg.device()
    L.check(L.lib().dfw_seg_postprocess_ex(x.data_ptr(), u8.data_ptr(), _p(gt), _p(counts), scratch.data_ptr(),
                                           B, H, W, float(r_threshold), float(threshold), int(bool(batch_max)),
                                           _stream()), "dfw_seg_postprocess")
    return u8, counts


def seg_labels(seg_u8, mx, gt=None, r_threshold=0.25, threshold=0.0, batch_max=False, labels_out=None, counts_out=None):
    """N-way label fusion.  seg_u8: uint8 [N, B, 3, H, W], the quantised masks of N classes (seg_postprocess per class,
    or per chunk of classes, into slices of one buffer); mx: int32 [N, B] (or [N*B]), the maxima those calls left in
    their `scratch` (may be None with the fixed threshold).  Returns (labels uint8 [B, H, W], counts int64 [B, 2, N+1] or
    None): label 0 = no class above its threshold (seg_postprocess' rule per class), else 1 + the foreground class of
    the largest score, lowest class on a tie; with gt (uint8 [B, H, W]: 0..N, 255 and anything above N ignored) the
    per-label intersections (row 0) and unions (row 1)."""
    arg = _Args("seg_labels")
    arg("seg_u8", seg_u8, torch.uint8, dim=5)
    N, B, _, H, W = seg_u8.shape
    arg.need(seg_u8.shape[2] == 3, "seg_u8 must be [N, B, 3, H, W], got {}", seg_u8.shape)
    if mx is not None:
        arg("mx", mx, torch.int32, elems=N * B)
    elif r_threshold > 0:
        raise ValueError("the dynamic threshold needs the per-image maxima (mx)")
    labels = labels_out if labels_out is not None else torch.empty(B, H, W, dtype=torch.uint8, device=seg_u8.device)
    arg("labels_out", labels, torch.uint8, (B, H, W))
    counts = None
    if gt is not None:
        arg("gt", gt, torch.uint8, (B, H, W))
        counts = counts_out if counts_out is not None else torch.empty(B, 2, N + 1, dtype=torch.int64, device=seg_u8.device)
        arg("counts_out", counts, torch.int64, (B, 2, N + 1))
    arg.device()
    L.check(L.lib().dfw_seg_labels(seg_u8.data_ptr(), _p(mx), _p(gt), labels.data_ptr(), _p(counts), N, B, H, W,
                                   float(r_threshold), float(threshold), int(bool(batch_max)), _stream()),
            "dfw_seg_labels")
    return labels, counts


def _check_table(arg, tab, tab_host, known):
    """seg_labels_cand's table through `arg`: tab and its host mirror tab_host are contiguous int32 vectors of one length,
    offsets + 1 + entries, of which the caller knows one count (`known`: E_cap, or the windows T).  Returns the other."""
    arg("tab", tab, torch.int32, dim=1, extent=known + 2)
    arg("tab_host", tab_host, torch.int32, (tab.numel(),), host=True)
    return tab.numel() - 1 - known


def seg_labels_cand(seg_u8, mx, tab, tab_host, nlabels, gt=None, r_threshold=0.25, threshold=0.0, want_area=False,
                    labels_out=None, counts_out=None):
    """Label fusion over candidate classes per query: seg_labels' rule per ENTRY.  seg_u8: uint8 [E_cap, 3, H, W],
    entry-major -- entry e is one (query, candidate class) pair, a query's entries adjacent; mx: int32 [E_cap], the maxima
    a gt-less seg_postprocess left (may be None with the fixed threshold).  `tab`: a DEVICE int32 [B + 1 + E_cap] tensor,
    offsets off[0..B] (query q owns entries [off[q], off[q+1]), an empty range gives label 0 everywhere) then the label
    byte lab[e] of every entry (1..nlabels; entries from off[B] on are padding and never read); `tab_host`: its int32 host
    mirror, validated by the library before the launch.  The kernel reads `tab` when it runs: under stream capture one
    graph serves every table written into the same tensor.  Returns (labels uint8 [B, H, W], counts int64
    [B, 2, nlabels+1] or None, area int64 [E_cap, 2] or None): the label is lab[e] of the foreground entry with the largest
    score, earliest entry on a tie; counts as seg_labels gives them (gt uint8 [B, H, W]: 0..nlabels, 255 and anything
    above nlabels ignored; a gt label outside the query's candidates is a miss in that label's union); area[e] = (pixels
    where e is foreground on its own, pixels where e won), ignore pixels included."""
    arg = _Args("seg_labels_cand")
    arg("seg_u8", seg_u8, torch.uint8, dim=4)
    E_cap, _, H, W = seg_u8.shape
    arg.need(seg_u8.shape[1] == 3, "seg_u8 must be [E_cap, 3, H, W], got {}", seg_u8.shape)
    B, nlabels = _check_table(arg, tab, tab_host, E_cap), int(nlabels)
    if mx is not None:
        arg("mx", mx, torch.int32, elems=E_cap)
    elif r_threshold > 0:
        raise ValueError("the dynamic threshold needs the per-entry maxima (mx)")
    labels = labels_out if labels_out is not None else torch.empty(B, H, W, dtype=torch.uint8, device=seg_u8.device)
    arg("labels_out", labels, torch.uint8, (B, H, W))
    counts = None
    if gt is not None:
        arg("gt", gt, torch.uint8, (B, H, W))
        shape = (B, 2, nlabels + 1)
        counts = counts_out if counts_out is not None else torch.empty(shape, dtype=torch.int64, device=seg_u8.device)
        arg("counts_out", counts, torch.int64, shape)
    arg.device()
    area = torch.empty(E_cap, 2, dtype=torch.int64, device=seg_u8.device) if want_area else None
    host = C.cast(tab_host.data_ptr(), C.POINTER(C.c_int32))
    L.check(L.lib().dfw_seg_labels_cand(seg_u8.data_ptr(), _p(mx), tab.data_ptr(), host, _p(gt), labels.data_ptr(),
                                        _p(counts), _p(area), B, E_cap, nlabels, H, W, float(r_threshold),
                                        float(threshold), _stream()), "dfw_seg_labels_cand")
    return labels, counts, area


def _u8_buf(arg, name, given, n, dev):
    """`given` (a caller-owned uint8 buffer of at least n bytes, checked through `arg` as `name`) or a fresh one on dev."""
    if given is None:
        return torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    arg(name, given, torch.uint8, extent=n)
    return given


def _native_setup(arg, a, seg_u8, targets, b, n, want_u8, u8_out, tmp, r_threshold, threshold):
    """What seg_native, seg_labels_native and seg_labels_cand_native share: ValueError unless `targets` were built for these
    b queries and seg_u8's (Hs, Ws); the targets' staged table made safe to read on this stream; and the fields the three
    argument records share by name -- source, item / weight tables, ground truth, thresholds, and the workspace of `n` planes
    per query (1, the classes, the longest candidate list): n strides of targets.tmp_bytes for the horizontal intermediates
    and n of targets.u8_bytes for the resized bytes, behind them in tmp or, with want_u8, in out_u8.  Returns (u8 or None,
    tmp, whether there is a ground truth); the caller keeps the buffers until it has launched."""
    Hs, Ws = seg_u8.shape[-2:]
    if targets.dev is None or targets.b != b or targets.src_hw != (Hs, Ws):
        raise ValueError(f"targets were built for {targets.b} queries from {targets.src_hw}, the call has {b} and seg_u8 is "
                         f"{tuple(seg_u8.shape)}")
    dev = seg_u8.device
    arg("targets.dev", targets.dev, torch.uint8, dim=1)
    u8 = _u8_buf(arg, "u8_out", u8_out, n * targets.u8_bytes, dev) if want_u8 else None
    tmp = _u8_buf(arg, "tmp", tmp, n * targets.tmp_bytes + (0 if want_u8 else n * targets.u8_bytes), dev)
    gt, gt_bytes = targets.gt_base
    if gt is not None:
        arg("targets.gt_base", gt, torch.uint8, extent=gt_bytes)
    arg.device()        # the callers have checked their own buffers
    if not torch.cuda.is_current_stream_capturing():
        targets.dev.record_stream(torch.cuda.current_stream())     # staged on the loader's stream, read on this one
    a.seg_u8, a.B, a.Hs, a.Ws = seg_u8.data_ptr(), b, Hs, Ws
    a.items, a.items_host = targets.dev.data_ptr(), C.addressof(targets.items)
    a.weights, a.weights_bytes = targets.dev.data_ptr(), targets.dev.numel()
    a.gt, a.gt_bytes = (gt.data_ptr(), gt_bytes) if gt is not None else (None, 0)
    a.tmp, a.tmp_bytes, a.tmp_res_off = tmp.data_ptr(), tmp.numel(), n * targets.tmp_bytes
    if u8 is not None:
        a.out_u8, a.out_u8_bytes = u8.data_ptr(), u8.numel()
    a.r_threshold, a.threshold = float(r_threshold), float(threshold)
    return u8, tmp, gt is not None


def _native_views(targets, lab, u8, n, rows=None):
    """Per-query views of the packed outputs: ([h_i, w_i] of lab, [rows_i (default n), 3, h_i, w_i] of u8's n planes), None
    for a buffer that is None."""
    items = list(targets.items)
    if lab is not None:
        lab = [lab[it.pred_off:it.pred_off + it.h * it.w].view(it.h, it.w) for it in items]
    if u8 is not None:
        per = u8[:n * targets.u8_bytes].view(n, targets.u8_bytes)
        u8 = [per[:r, it.u8_off:it.u8_off + 3 * it.h * it.w].unflatten(1, (3, it.h, it.w))
              for it, r in zip(items, rows or [n] * len(items))]
    return lab, u8


def seg_native(seg_u8, targets, r_threshold=0.25, threshold=0.0, batch_max=False, want_u8=True, want_pred=True,
               u8_out=None, pred_out=None, tmp=None):
    """Native-size masks and scores: seg_u8 uint8 [b, 3, Hs, Ws] (seg_postprocess' output) resized back to every query's
    own h x w exactly as `Image.fromarray(hwc).resize((w, h))` does (Pillow's default filter, BICUBIC), thresholded with
    the launcher's expressions on the RESIZED image -- r_threshold > 0: max * r_threshold with the resized image's own
    maximum (bicubic overshoots), or the batch's with batch_max; else the fixed `threshold` -- and, when `targets`
    carries a ground truth, counted against it at native size (main_oss.py:128-155 under --use_original_imgsize).

    targets: input_pipeline.NativeTargets for this batch and this (Hs, Ws).  Four launches whatever b.  Returns
    dict(seg_u8=[uint8 views [3, h_i, w_i]] or None, pred=[uint8 0/1 views [h_i, w_i]] or None, counts=int64 [b, 4]
    (inter0, inter1, union0, union1) or None, mx=int32 [b] resized maxima, sizes=[(h_i, w_i)]); the views of each list
    are backed by one packed buffer.  u8_out / pred_out / tmp: caller-owned uint8 buffers of at least targets.u8_bytes /
    pred_bytes / tmp_bytes (tmp_bytes + u8_bytes without want_u8) instead of fresh ones."""
    arg = _Args("seg_native")
    arg("seg_u8", seg_u8, torch.uint8, dim=4)
    arg.need(seg_u8.shape[1] == 3, "seg_u8 must be [b, 3, Hs, Ws], got {}", seg_u8.shape)
    b, dev = seg_u8.shape[0], seg_u8.device
    a = L.SegNativeArgs()
    pred = _u8_buf(arg, "pred_out", pred_out, targets.pred_bytes, dev) if want_pred else None
    u8, tmp, has_gt = _native_setup(arg, a, seg_u8, targets, b, 1, want_u8, u8_out, tmp, r_threshold, threshold)
    counts = torch.empty(b, 4, dtype=torch.int64, device=dev) if has_gt else None
    mx = torch.empty(b, dtype=torch.int32, device=dev)
    if pred is not None:
        a.pred, a.pred_bytes = pred.data_ptr(), pred.numel()
    a.mx, a.counts, a.batch_max = mx.data_ptr(), _p(counts), int(bool(batch_max))
    L.check(L.lib().dfw_seg_native(C.byref(a), _stream()), "dfw_seg_native")
    pred, planes = _native_views(targets, pred, u8, 1)
    return dict(seg_u8=planes and [p[0] for p in planes], pred=pred, counts=counts, mx=mx, sizes=list(targets.sizes))


def seg_labels_native(seg_u8, targets, r_threshold=0.25, threshold=0.0, batch_max=False, class_ids=None, want_u8=False,
                      labels_out=None, u8_out=None, tmp=None):
    """N-way labels and counts at every query's own size: seg_u8 uint8 [N, b, 3, Hs, Ws] (segment_classes' class-major
    masks) resized per class and image as seg_native does (Pillow's default BICUBIC, exact), then seg_labels' rule on the
    RESIZED bytes -- thresholds from the maxima of the resized planes (bicubic overshoots), label 0 or 1 + the foreground
    class of the largest score, lowest class on a tie -- and, when `targets` carries a ground truth, per-label counts
    against it at native size.

    targets: input_pipeline.NativeTargets for these b queries and this (Hs, Ws); its ground truth is label maps (0 =
    background, 1 + c = class c, ids above N dropped) or, with class_ids (N ints or an int32 tensor: the ground-truth id of
    class c), class-id maps: 1 + the lowest c with class_ids[c] == id, every other id background.  Pixels equal to the
    targets' ignore_value are dropped; their class_value is not read.  Four launches whatever N and b.  Returns
    dict(labels=[uint8 views [h_i, w_i]], counts=int64 [b, 2, N+1] or None, mx=int32 [N, b] resized maxima,
    seg_u8=[uint8 views [N, 3, h_i, w_i]] or None (want_u8), sizes=[(h_i, w_i)]); the views of each list are backed by one
    packed buffer, classes targets.u8_bytes apart.  labels_out / u8_out / tmp: caller-owned uint8 buffers of at least
    targets.pred_bytes / N * u8_bytes / N * tmp_bytes (N * (tmp_bytes + u8_bytes) without want_u8) instead of fresh ones."""
    arg = _Args("seg_labels_native")
    arg("seg_u8", seg_u8, torch.uint8, dim=5)
    arg.need(seg_u8.shape[2] == 3, "seg_u8 must be [N, b, 3, Hs, Ws], got {}", seg_u8.shape)
    N, b, dev = seg_u8.shape[0], seg_u8.shape[1], seg_u8.device
    a = L.SegLabelsNativeArgs()
    labels = _u8_buf(arg, "labels_out", labels_out, targets.pred_bytes, dev)
    if class_ids is not None:
        class_ids = torch.as_tensor(class_ids, dtype=torch.int32).to(dev).contiguous()
        if class_ids.shape != (N,):
            raise ValueError(f"class_ids must hold one id per class ({N}), got {tuple(class_ids.shape)}")
    u8, tmp, has_gt = _native_setup(arg, a, seg_u8, targets, b, N, want_u8, u8_out, tmp, r_threshold, threshold)
    counts = torch.empty(b, 2, N + 1, dtype=torch.int64, device=dev) if has_gt else None
    mx = torch.empty(N, b, dtype=torch.int32, device=dev)
    a.N, a.tmp_cls_stride, a.u8_cls_stride = N, targets.tmp_bytes, targets.u8_bytes
    a.labels, a.labels_bytes = labels.data_ptr(), labels.numel()
    a.mx, a.counts, a.class_ids, a.batch_max = mx.data_ptr(), _p(counts), _p(class_ids), int(bool(batch_max))
    L.check(L.lib().dfw_seg_labels_native(C.byref(a), _stream()), "dfw_seg_labels_native")
    lab, planes = _native_views(targets, labels, u8, N)
    return dict(labels=lab, counts=counts, mx=mx, seg_u8=planes, sizes=list(targets.sizes))


def cand_native_workspace(targets, K, want_u8=False):
    """(tmp bytes, tmp_res_off, out_u8 bytes) of seg_labels_cand_native for a longest candidate list of K entries: K
    strides of targets.tmp_bytes for the horizontal intermediates and K of targets.u8_bytes for the resized bytes -- behind
    the intermediates in tmp, or in out_u8 with want_u8.  K, not E_cap: a query's entries share the strides by position."""
    K = max(int(K), 1)
    tmp_part, u8_part = K * targets.tmp_bytes, K * targets.u8_bytes
    return (tmp_part if want_u8 else tmp_part + u8_part), tmp_part, (u8_part if want_u8 else 0)


def seg_labels_cand_native(seg_u8, targets, tab, tab_host, nlabels, r_threshold=0.25, threshold=0.0, class_ids=None,
                           entry_ids=None, want_area=False, want_u8=False, labels_out=None, u8_out=None, tmp=None):
    """Candidate classes per query at every query's own size: seg_u8 uint8 [E_cap, 3, Hs, Ws], entry-major, and `tab` /
    `tab_host` as seg_labels_cand takes them (offsets off[0..b], then the label byte of every entry; the device table is
    read when the kernels run, the host mirror is validated).  Every entry is resized to ITS query's h x w as
    seg_labels_native resizes a class (Pillow's default BICUBIC, exact), then seg_labels_cand's rule runs on the RESIZED
    bytes: thresholds from the maxima of the resized planes, label = lab[e] of the foreground entry with the largest
    score, earliest entry on a tie, 0 with none.

    targets: input_pipeline.NativeTargets for the b queries and this (Hs, Ws).  With a ground truth it is read in place
    at native size; pixels equal to the targets' ignore_value are dropped, and an id becomes a label
      with neither table: as it is (ids outside 0..nlabels dropped);
      class_ids (nlabels ints or an int32 tensor; labels are 1 + set index): 1 + the lowest c with class_ids[c] == id,
        every other id background -- a class outside the query's candidates is a miss in its own label's union;
      entry_ids (E_cap ints or an int32 tensor: the ground-truth id of every entry's class; labels local to the query):
        the label of the query's earliest entry with that id, every other id background (local labels have no bin for a
        class the query did not name).
    Giving both is a ValueError.  Four launches whatever b and E.  The workspace is K strides, K the longest list
    (cand_native_workspace).  Returns dict(labels=[uint8 views [h_i, w_i]], counts=int64 [b, 2, nlabels+1] or None,
    area=int64 [E_cap, 2] or None (want_area; counted on the resized bytes), mx=int32 [E_cap] resized maxima,
    seg_u8=[uint8 views [K_i, 3, h_i, w_i], K_i the query's entries] or None (want_u8), sizes=[(h_i, w_i)])."""
    arg = _Args("seg_labels_cand_native")
    arg("seg_u8", seg_u8, torch.uint8, dim=4)
    arg.need(seg_u8.shape[1] == 3, "seg_u8 must be [E_cap, 3, Hs, Ws], got {}", seg_u8.shape)
    E_cap, dev = seg_u8.shape[0], seg_u8.device
    b, nlabels = _check_table(arg, tab, tab_host, E_cap), int(nlabels)
    if class_ids is not None and entry_ids is not None:
        raise ValueError("seg_labels_cand_native: give class_ids (labels = 1 + set index) or entry_ids (local labels), not both")
    off = tab_host[:b + 1].tolist()
    rows = [hi - lo for lo, hi in zip(off, off[1:])]
    K = max(max(rows), 1)                  # cand_native_workspace(targets, K, want_u8) is what _native_setup lays out
    a = L.SegLabelsCandNativeArgs()

    def ids(t, n, name):
        if t is None:
            return None
        t = torch.as_tensor(t, dtype=torch.int32).to(dev).contiguous()
        if t.shape != (n,):
            raise ValueError(f"{name} must hold {n} ids, got {tuple(t.shape)}")
        return t
    class_ids, entry_ids = ids(class_ids, nlabels, "class_ids"), ids(entry_ids, E_cap, "entry_ids")
    labels = _u8_buf(arg, "labels_out", labels_out, targets.pred_bytes, dev)
    u8, tmp, has_gt = _native_setup(arg, a, seg_u8, targets, b, K, want_u8, u8_out, tmp, r_threshold, threshold)
    counts = torch.empty(b, 2, nlabels + 1, dtype=torch.int64, device=dev) if has_gt else None
    area = torch.empty(E_cap, 2, dtype=torch.int64, device=dev) if want_area else None
    mx = torch.empty(E_cap, dtype=torch.int32, device=dev)
    a.E_cap, a.nlabels, a.tab, a.tab_host = E_cap, nlabels, tab.data_ptr(), tab_host.data_ptr()
    a.tmp_cls_stride, a.u8_cls_stride = targets.tmp_bytes, targets.u8_bytes
    a.labels, a.labels_bytes = labels.data_ptr(), labels.numel()
    a.mx, a.counts, a.area = mx.data_ptr(), _p(counts), _p(area)
    a.class_ids, a.entry_ids = _p(class_ids), _p(entry_ids)
    L.check(L.lib().dfw_seg_labels_cand_native(C.byref(a), _stream()), "dfw_seg_labels_cand_native")
    lab, planes = _native_views(targets, labels, u8, K, rows)
    return dict(labels=lab, counts=counts, area=area, mx=mx, seg_u8=planes, sizes=list(targets.sizes))


def _tile_plan(plan):
    """input_pipeline.TilePlan (or a ready _lib.TilePlan record) -> the record, its T."""
    c = plan if isinstance(plan, L.TilePlan) else plan.c_struct()
    return c, c.ny * c.nx


def tiles_cut(plan, img_u8, lut, first=0, count=None, out=None):
    """Windows first .. first + count - 1 (default: all from `first`) of a staged image: img_u8 uint8 [h, w, 3] on the
    device, plan an input_pipeline.TilePlan for (h, w), lut the 256-entry fp32 table of DeviceImageTransform -> fp32
    [count, 3, th, tw], each window bit for bit DeviceImageTransform((th, tw)).image(crop).  One launch; `out`: a
    caller-owned contiguous fp32 [count, 3, th, tw] instead of a fresh one."""
    c, T = _tile_plan(plan)
    arg = _Args("tiles_cut")
    arg("img_u8", img_u8, torch.uint8, (c.img_h, c.img_w, 3))
    arg("lut", lut, torch.float32, elems=256)
    if count is None:
        count = T - first
    shape = (count, 3, c.tile_h, c.tile_w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=img_u8.device)
    arg("out", out, torch.float32, shape)
    arg.device()
    L.check(L.lib().dfw_tiles_cut(C.byref(c), img_u8.data_ptr(), lut.data_ptr(), out.data_ptr(), int(first), int(count),
                                  _stream()), "dfw_tiles_cut")
    return out


def tiles_merge(plan, win, out=None, mx=None):
    """Blend the windows' masks back into the image: win uint8 [N, T, 3, th, tw] (the seg_u8 of every window and class) ->
    (uint8 [N, 3, h, w], mx int32 [N] = the maximum byte of each class' merged image).  Per byte the weighted mean of the
    windows over it in integers, round half up (csrc/tiles.hip); exact and independent of any order; one window is the
    identity.  out.view(N, 1, 3, h, w) and mx are seg_labels' inputs.  Two launches; `out` / `mx`: caller-owned buffers."""
    c, T = _tile_plan(plan)
    arg = _Args("tiles_merge")
    arg("win", win, torch.uint8, dim=5)
    N = win.shape[0]
    arg.need(win.shape[1:] == (T, 3, c.tile_h, c.tile_w), "win must be [N, {}, 3, {}, {}], got {}", T, c.tile_h, c.tile_w, win.shape)
    if out is None:
        out = torch.empty(N, 3, c.img_h, c.img_w, dtype=torch.uint8, device=win.device)
    if mx is None:
        mx = torch.empty(N, dtype=torch.int32, device=win.device)
    arg("out", out, torch.uint8, (N, 3, c.img_h, c.img_w))
    arg("mx", mx, torch.int32, elems=N)
    arg.device()
    L.check(L.lib().dfw_tiles_merge(C.byref(c), win.data_ptr(), N, out.data_ptr(), mx.data_ptr(), _stream()),
            "dfw_tiles_merge")
    return out, mx


def tiles_labels_cand(plan, ent, tab, tab_host, N, gt=None, r_threshold=0.25, threshold=0.0, want_area=False,
                      labels_out=None, counts_out=None, mx_out=None, area_out=None):
    """tiles_merge + seg_labels over a SPARSE set of (window, class) entries: ent uint8 [E_cap, 3, th, tw], entry-major, the
    entries of one window adjacent in ascending class (None when no window lists anything); `tab` a DEVICE int32
    [T + 1 + E_cap] tensor -- offsets off[0..T] (window t owns entries [off[t], off[t+1])), then the class 0..N-1 of every
    entry -- and `tab_host` its host mirror, validated by the library before the launch (input_pipeline.TilePlan.
    candidate_table builds it).  A (window, class) pair that is not listed counts as an all-zero mask, so the result is bit
    for bit tiles_merge + seg_labels on the dense [N, T, 3, th, tw] buffer that holds the entries and zeros elsewhere --
    the blend weight of a window counts at every pixel it covers, whatever it lists -- without that buffer and without the
    merged [N, 3, h, w] image.  gt: optional uint8 [h, w] as seg_labels takes it.

    Returns (labels uint8 [h, w], counts int64 [2, N+1] or None, mx int32 [N] = the maximum byte of every class' merged
    image, area int64 [N, 2] or None = per class (pixels foreground on its own, pixels where it won), ignore pixels
    included).  Two or three launches, no memset node; labels_out / counts_out / mx_out / area_out: caller-owned buffers."""
    c, T = _tile_plan(plan)
    N = int(N)
    arg = _Args("tiles_labels_cand")
    E_cap, dev = _check_table(arg, tab, tab_host, T), tab.device
    if ent is not None:     # a table of tab.numel() words names E_cap entries
        arg("ent", ent, torch.uint8, (E_cap, 3, c.tile_h, c.tile_w))
    hw = (c.img_h, c.img_w)

    def buf(name, given, shape, dtype):
        if given is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        arg(name, given, dtype, shape)
        return given
    labels = buf("labels_out", labels_out, hw, torch.uint8)
    mx = buf("mx_out", mx_out, (N,), torch.int32)
    counts = None
    if gt is not None:
        arg("gt", gt, torch.uint8, hw)
        counts = buf("counts_out", counts_out, (2, N + 1), torch.int64)
    area = buf("area_out", area_out, (N, 2), torch.int64) if want_area or area_out is not None else None
    arg.device()
    host = C.cast(tab_host.data_ptr(), C.POINTER(C.c_int32))
    L.check(L.lib().dfw_tiles_labels_cand(C.byref(c), _p(ent), tab.data_ptr(), host, _p(gt), labels.data_ptr(),
                                          mx.data_ptr(), _p(counts), _p(area), E_cap, N, float(r_threshold),
                                          float(threshold), _stream()), "dfw_tiles_labels_cand")
    return labels, counts, mx, area


def seg_components_workspace(B, H, W):
    """Bytes of seg_components' workspace for a [B, H, W] label map."""
    return int(L.lib().dfw_seg_components_workspace_bytes(int(B), int(H), int(W)))


def seg_components(labels, ids, n, ws, filtered=None, stats=None, gt=None, counts=None, connectivity=8, min_area=0,
                   nlabels=None):
    """Connected components of a label map, on caller-owned buffers only (objects.ComponentBuffers holds a set): labels
    uint8 [B, H, W], 0 = background, equal non-zero bytes connect over `connectivity` (4 | 8) neighbours; a component with
    fewer than min_area pixels is removed.  Writes ids int32 [B, H, W] (0 = background or removed, else 1..n_b in row-major
    order of each component's first pixel, restarting per image), n int32 [B, 2] = (kept, found before the filter) and,
    where given, filtered uint8 [B, H, W] (the labels without the removed components; not `labels` itself), stats int32
    [B, cap, 8] = (label, area, y0, x0, y1, x1 half-open, first pixel y * W + x, 0) per kept component, rows from
    min(n_b, cap) on zero -- only stats truncates -- and counts int64 [B, 2, nlabels + 1], seg_labels' counts of the FILTERED
    bytes against gt uint8 [B, H, W] (nlabels: the number of classes; a byte above it has no bin).  ws: a uint8 buffer of at
    least seg_components_workspace(B, H, W) bytes, which needs no initialisation.  A fixed number of launches (at most 8),
    no host synchronisation, no memset node: the call can be captured.  Returns None."""
    own = _Args("seg_components")
    own("labels", labels, torch.uint8, dim=3)
    B, H, W = labels.shape
    a = L.SegComponentsArgs()
    a.labels, a.ids, a.n = labels.data_ptr(), own("ids", ids, torch.int32, (B, H, W)), own("n", n, torch.int32, (B, 2))
    a.ws, a.ws_bytes = own("ws", ws, torch.uint8), ws.numel()
    if filtered is not None:
        a.filtered = own("filtered", filtered, torch.uint8, (B, H, W))
    if stats is not None:
        if stats.dim() != 3:
            raise ValueError("seg_components: stats must be int32 [B, cap, 8]")
        a.stats, a.cap = own("stats", stats, torch.int32, (B, stats.shape[1], 8)), stats.shape[1]
    if counts is not None and gt is None:
        raise ValueError("seg_components: counts need a ground truth")
    if gt is not None:
        if nlabels is None:
            raise ValueError("seg_components: a ground truth needs nlabels, the number of classes")
        a.gt, a.nlabels = own("gt", gt, torch.uint8, (B, H, W)), int(nlabels)
        if counts is not None:
            a.counts = own("counts", counts, torch.int64, (B, 2, int(nlabels) + 1))
    a.B, a.H, a.W, a.connectivity, a.min_area = B, H, W, int(connectivity), int(min_area)
    own.device()
    L.check(L.lib().dfw_seg_components(C.byref(a), _stream()), "dfw_seg_components")


def seg_holes_workspace(B, H, W):
    """Bytes of seg_holes' workspace for [B, H, W] maps; 0 for sizes the call refuses."""
    return int(L.lib().dfw_seg_holes_workspace_bytes(int(B), int(H), int(W)))


def seg_holes(labels, ids, ids_out, labels_out, holes, ws, stats=None, stats_out=None, gt=None, counts=None, connectivity=8,
              max_area=None, nlabels=None):
    """Fills the holes of labelled objects, on caller-owned buffers only (objects.HoleBuffers holds a set): labels uint8
    [B, H, W] and ids int32 [B, H, W], normally seg_components' filtered and ids.  A region is a connected component of
    zero bytes under the DUAL of `connectivity` (the objects': 8 -> regions over 4 neighbours, 4 -> over 8); it is filled
    when it touches no row or column of the image frame, the id left of its first pixel (the owner) is at least 1, every
    non-background pixel around it carries that id, and it has at most max_area pixels (None: 2^31 - 1; 0 fills nothing).
    Regions bordered by two objects -- of one class or two -- and holes with an island of another object inside are left
    alone.  Writes ids_out int32 and labels_out uint8 [B, H, W] (the inputs with every filled pixel set to the owner's id
    and label byte), holes int32 [B, 2] = (regions filled, regions enclosed) and, where given, stats_out int32 [B, cap, 8]
    = stats with column 1 (area) grown by, and column 7 set to, each object's filled pixels, and counts int64 [B, 2,
    nlabels + 1], seg_labels' counts of labels_out against gt uint8 [B, H, W].  No output may share memory with an input.
    ws: a uint8 buffer of at least seg_holes_workspace(B, H, W) bytes, which needs no initialisation.  A fixed number of
    launches (at most 6), no host synchronisation, no memset node: the call can be captured.  Returns None."""
    own = _Args("seg_holes")
    own("labels", labels, torch.uint8, dim=3)
    B, H, W = labels.shape
    a = L.SegHolesArgs()
    a.labels, a.ids = labels.data_ptr(), own("ids", ids, torch.int32, (B, H, W))
    a.ids_out, a.labels_out = own("ids_out", ids_out, torch.int32, (B, H, W)), own("labels_out", labels_out, torch.uint8, (B, H, W))
    a.holes = own("holes", holes, torch.int32, (B, 2))
    a.ws, a.ws_bytes = own("ws", ws, torch.uint8), ws.numel()
    if (stats is None) != (stats_out is None):
        raise ValueError("seg_holes: stats and stats_out come together")
    if stats is not None:
        if stats.dim() != 3:
            raise ValueError("seg_holes: stats must be int32 [B, cap, 8]")
        cap = stats.shape[1]
        a.stats, a.stats_out, a.cap = own("stats", stats, torch.int32, (B, cap, 8)), own("stats_out", stats_out, torch.int32, (B, cap, 8)), cap
    if counts is not None and gt is None:
        raise ValueError("seg_holes: counts need a ground truth")
    if gt is not None:
        if nlabels is None:
            raise ValueError("seg_holes: a ground truth needs nlabels, the number of classes")
        a.gt, a.nlabels = own("gt", gt, torch.uint8, (B, H, W)), int(nlabels)
        if counts is not None:
            a.counts = own("counts", counts, torch.int64, (B, 2, int(nlabels) + 1))
    max_area = 2 ** 31 - 1 if max_area is None else int(max_area)
    if not 0 <= max_area <= 2 ** 31 - 1:
        raise ValueError(f"seg_holes: max_area must lie in 0..2^31 - 1, got {max_area}")
    a.B, a.H, a.W, a.connectivity, a.max_area = B, H, W, int(connectivity), max_area
    own.device()
    L.check(L.lib().dfw_seg_holes(C.byref(a), _stream()), "dfw_seg_holes")


_RLE_ORDERS = {"row": 0, "column": 1}


def _rle_order(order):
    if order not in _RLE_ORDERS:
        raise ValueError(f"order must be 'row' or 'column', not {order!r}")
    return _RLE_ORDERS[order]


def seg_rle_workspace(B, H, W, cap, max_runs, order="column"):
    """Bytes of seg_rle's workspace for a [B, H, W] id map, objects 1..cap, max_runs rows per image."""
    return int(L.lib().dfw_seg_rle_workspace_bytes(int(B), int(H), int(W), int(cap), int(max_runs), _rle_order(order)))


def seg_rle(ids, runs, run_off, nruns, ws, cap, order="column"):
    """Run-length encoding of the objects 1..cap of an id map, on caller-owned buffers only (objects.RunBuffers holds a
    set): ids int32 [B, H, W], normally seg_components' (any int32 map is accepted; ids outside 1..cap count as 0).  A
    pixel's position is y * W + x (order "row") or x * H + y ("column", COCO's order); a run is a maximal interval of
    positions with one equal non-zero id and does not stop at a line's end.  Writes nruns int32 [B, 2] = (kept, found),
    kept = min(found, max_runs) runs in ascending start; runs int32 [B, max_runs, 2] = (start, length) grouped by id ascending
    and ascending in start within an id, rows from kept on left as they were; run_off int32 [B, cap + 1]: object k's rows are
    run_off[k-1] .. run_off[k].  ws: a uint8 buffer of at least seg_rle_workspace(B, H, W, cap, max_runs, order) bytes, which
    needs no initialisation.  A number of launches fixed by the arguments, no host synchronisation, no memset node: the call
    can be captured.  Returns None."""
    own = _Args("seg_rle")
    own("ids", ids, torch.int32, dim=3)
    B, H, W = ids.shape
    cap = int(cap)
    own.need(runs.dim() == 3, "runs must be int32 [B, max_runs, 2]")
    max_runs = runs.shape[1]
    a = L.SegRleArgs()
    a.ids, a.runs = ids.data_ptr(), own("runs", runs, torch.int32, (B, max_runs, 2))
    a.run_off, a.nruns = own("run_off", run_off, torch.int32, (B, cap + 1)), own("nruns", nruns, torch.int32, (B, 2))
    a.ws, a.ws_bytes = own("ws", ws, torch.uint8), ws.numel()
    a.B, a.H, a.W, a.cap, a.max_runs, a.order = B, H, W, cap, max_runs, _rle_order(order)
    own.device()
    L.check(L.lib().dfw_seg_rle(C.byref(a), _stream()), "dfw_seg_rle")


def seg_contours_workspace(B, H, W, cap, max_edges):
    """Bytes of seg_contours' workspace for a [B, H, W] id map, objects 1..cap, max_edges edges per image; 0 for arguments
    seg_contours answers DFW_EINVAL for."""
    return int(L.lib().dfw_seg_contours_workspace_bytes(int(B), int(H), int(W), int(cap), int(max_edges)))


def seg_contours_simplify_block():
    """The ring length up to which seg_contours' simplification keeps a ring's state in LDS; longer rings keep it in the
    workspace."""
    v = C.c_int32()
    L.check(L.lib().dfw_seg_contours_simplify_block(C.byref(v)), "dfw_seg_contours_simplify_block")
    return int(v.value)


def seg_contours(ids, verts, rings, ring_off, n, ws, cap, connectivity=8, simp_verts=None, simp_rings=None, simp_n=None,
                 tol4=0):
    """Outlines of the objects 1..cap of an id map as rings of corner points, on caller-owned buffers only
    (objects.ContourBuffers holds a set): ids int32 [B, H, W], normally seg_components' or seg_holes' (any int32 map is
    accepted; ids outside 1..cap count as 0); connectivity = 4 | 8, the one the ids were made with.  Pixel (x, y) is the
    unit square from (x, y) to (x + 1, y + 1); a ring runs clockwise on screen (y down), the object on its right, so an
    outer ring has a positive area and a hole ring a negative one (include/diffews_hip.h holds the definition).  Writes n
    int32 [B, 4] = (edges found, corners, rings, complete); rings int32 [B, max_edges / 4, 4] = (id, first, count, area)
    sorted by id and then by the ring's smallest edge key; ring_off int32 [B, cap + 1]: object k's rings are rows
    ring_off[k-1] .. ring_off[k]; verts int32 [B, max_edges, 2] = (X, Y), the corners of ring r being rows first ..
    first + count.  An image with more than max_edges edges gets n = (found, 0, 0, 0), a zero ring_off and no row: there
    are no partial results.  Rows behind the kept ones are left as they were.  ws: a uint8 buffer of at least
    seg_contours_workspace(B, H, W, cap, max_edges) bytes, which needs no initialisation.  A number of launches fixed by
    the arguments, no host synchronisation, no memset node: the call can be captured.  Returns None.

    simp_verts, simp_rings, simp_n (all three or none; shaped like verts, rings and n) and tol4, the tolerance in quarter
    pixels, 0..32768: the same rings simplified by Douglas-Peucker in integers (include/diffews_hip.h holds the
    definition), three more launches.  simp_rings = (id, first', count', area of the original ring) in the rows of rings,
    simp_verts the kept corners, simp_n = (corners in, corners kept, rings, complete), (0, 0, 0, 0) for an image that is
    not complete; ring_off serves both.  Without them the call is what it was."""
    own = _Args("seg_contours")
    own("ids", ids, torch.int32, dim=3)
    simp = (simp_verts, simp_rings, simp_n)
    if any(t is None for t in simp) != all(t is None for t in simp):
        raise ValueError("seg_contours: simp_verts, simp_rings and simp_n come together or not at all")
    tol4 = int(tol4)
    if not 0 <= tol4 <= 32768 or (simp_n is None and tol4):
        raise ValueError("seg_contours: tol4 must be 0..32768 quarter pixels, and 0 without the simp_ buffers")
    if connectivity not in (4, 8):
        raise ValueError(f"seg_contours: connectivity must be 4 or 8, not {connectivity!r}")
    B, H, W = ids.shape
    cap = int(cap)
    if verts.dim() != 3 or verts.shape[1] < 4 or verts.shape[1] % 4:
        raise ValueError("seg_contours: verts must be int32 [B, max_edges, 2] with max_edges a multiple of 4, at least 4")
    max_edges = verts.shape[1]
    a = L.SegContoursArgs()
    a.ids, a.verts = ids.data_ptr(), own("verts", verts, torch.int32, (B, max_edges, 2))
    a.rings, a.ring_off = own("rings", rings, torch.int32, (B, max_edges // 4, 4)), own("ring_off", ring_off, torch.int32, (B, cap + 1))
    a.n = own("n", n, torch.int32, (B, 4))
    a.ws, a.ws_bytes = own("ws", ws, torch.uint8), ws.numel()
    a.B, a.H, a.W, a.cap, a.max_edges, a.connectivity = B, H, W, cap, max_edges, int(connectivity)
    if simp_n is not None:
        a.simp_verts = own("simp_verts", simp_verts, torch.int32, (B, max_edges, 2))
        a.simp_rings = own("simp_rings", simp_rings, torch.int32, (B, max_edges // 4, 4))
        a.simp_n, a.tol4 = own("simp_n", simp_n, torch.int32, (B, 4)), tol4
    own.device()
    L.check(L.lib().dfw_seg_contours(C.byref(a), _stream()), "dfw_seg_contours")


def seg_match_workspace(B, H, W, cap_p, cap_g, max_records, max_pairs):
    """Bytes of seg_match's workspace for [B, H, W] id maps, objects 1..cap_p against 1..cap_g, max_records records and
    max_pairs pair rows per image; 0 for sizes seg_match refuses."""
    return int(L.lib().dfw_seg_match_workspace_bytes(int(B), int(H), int(W), int(cap_p), int(cap_g), int(max_records),
                                                     int(max_pairs)))


def seg_match(pids, gids, pairs, pair_off, area, match, gmatch, pq, n, ws, max_records, pstats=None, gstats=None, skip=None,
              iou=(1, 2)):
    """Predicted objects matched to ground-truth objects, on caller-owned buffers only (objects.MatchBuffers holds a set):
    pids and gids int32 [B, H, W], normally seg_components' ids of the prediction and of the ground truth (any int32 maps
    are accepted; ids outside 1..cap count as 0).  pstats / gstats (optional) int32 [B, cap, 8], seg_components' tables:
    column 0 is an object's class, 1 for every object of a side without a table.  skip (optional) uint8 [B, H, W]: a pixel
    whose byte is 255 is not counted.  iou = (num, den): objects of one class in 1..nlabels match when inter * den > num *
    union, strictly; the threshold is at least 1/2, so every object has at most one partner.

    Writes n int32 [B, 4] = (pairs kept, pairs found, records kept, records found); pairs int32 [B, max_pairs, 3] = (p, g,
    inter) ascending in (p, g), rows from kept on left as they were; pair_off int32 [B, cap_p + 2]: the rows of p are
    pair_off[p] .. pair_off[p + 1]; area int32 [B, cap_p + cap_g + 2] = areaP[0..cap_p], areaG[0..cap_g]; match int32
    [B, cap_p, 3] = (g, inter, union) of each predicted object's partner or zeros; gmatch int32 [B, cap_g], the partner p or
    0; pq int64 [B, nlabels + 1, 4] = (TP, FP, FN, S) per class, S the sum of floor(inter * 2^32 / union) over the TPs.
    cap_p, cap_g, nlabels and max_pairs are the buffers' shapes; max_records, the records kept per image (a record is a
    maximal interval of positions with one equal (p, g) other than (0, 0)), is given.  ws: a uint8 buffer of at least
    seg_match_workspace(B, H, W, cap_p, cap_g, max_records, max_pairs) bytes, which needs no initialisation.  A number of
    launches fixed by the arguments, no host synchronisation, no memset node: the call can be captured.  Returns None."""
    own = _Args("seg_match")
    own("pids", pids, torch.int32, dim=3)
    B, H, W = pids.shape
    if match.dim() != 3 or gmatch.dim() != 2 or pairs.dim() != 3 or pq.dim() != 3:
        raise ValueError("seg_match: match must be int32 [B, cap_p, 3], gmatch int32 [B, cap_g], pairs int32 [B, max_pairs, 3] "
                         "and pq int64 [B, nlabels + 1, 4]")
    cap_p, cap_g, max_pairs, nlabels = match.shape[1], gmatch.shape[1], pairs.shape[1], pq.shape[1] - 1
    num, den = (int(v) for v in iou)
    a = L.SegMatchArgs()
    a.pids, a.gids = pids.data_ptr(), own("gids", gids, torch.int32, (B, H, W))
    if pstats is not None:
        a.pstats = own("pstats", pstats, torch.int32, (B, cap_p, 8))
    if gstats is not None:
        a.gstats = own("gstats", gstats, torch.int32, (B, cap_g, 8))
    if skip is not None:
        a.skip = own("skip", skip, torch.uint8, (B, H, W))
    a.pairs, a.pair_off = own("pairs", pairs, torch.int32, (B, max_pairs, 3)), own("pair_off", pair_off, torch.int32, (B, cap_p + 2))
    a.area, a.match = own("area", area, torch.int32, (B, cap_p + cap_g + 2)), own("match", match, torch.int32, (B, cap_p, 3))
    a.gmatch, a.pq = own("gmatch", gmatch, torch.int32, (B, cap_g)), own("pq", pq, torch.int64, (B, nlabels + 1, 4))
    a.n, a.ws, a.ws_bytes = own("n", n, torch.int32, (B, 4)), own("ws", ws, torch.uint8), ws.numel()
    a.B, a.H, a.W, a.capP, a.capG, a.nlabels = B, H, W, cap_p, cap_g, nlabels
    a.max_records, a.max_pairs, a.num, a.den = int(max_records), max_pairs, num, den
    own.device()
    L.check(L.lib().dfw_seg_match(C.byref(a), _stream()), "dfw_seg_match")


def seg_scores_workspace(B, cap):
    """Bytes of seg_scores' workspace for B images and objects 1..cap; 0 for sizes seg_scores refuses."""
    return int(L.lib().dfw_seg_scores_workspace_bytes(int(B), int(cap)))


def seg_scores_block():
    """Positions one workgroup of seg_scores covers: the size at which its kernel changes path."""
    p = C.c_int32()
    L.check(L.lib().dfw_seg_scores_block(C.byref(p)), "dfw_seg_scores_block")
    return p.value


def seg_scores(ids, labels, seg_u8, planes, planes_host, scores, ws):
    """Per-object confidence, on caller-owned buffers only (objects.ScoreBuffers holds a set): ids int32 [B, H, W] and
    labels uint8 [B, H, W], normally seg_components' ids and filtered map; seg_u8 uint8 [P, 3, H, W], P plane groups of
    three channels; planes int32 [B, nlabels + 1] on the device, the plane group of every label of every image (-1: none;
    entry 0 is never read), and planes_host, its host mirror (a CPU tensor, pinned or not), which is what the call
    validates -- the kernel reads the device table when it runs and treats an entry outside 0..P-1 as "not counted".  A
    pixel is counted when 1 <= id <= cap, its label l lies in 1..nlabels and planes[b, l] in 0..P-1; its value is the sum
    of the three bytes of that plane group at the pixel, 0..765.  Writes scores int64 [B, cap, 4] = (sum, counted pixels,
    min, max) of object id in row id - 1, zeros for a row without a counted pixel; cap and nlabels are the buffers' shapes.
    ws: a uint8 buffer of at least seg_scores_workspace(B, cap) bytes, which needs no initialisation.  Three launches, no
    host synchronisation, no memset node: the call can be captured.  Returns None."""
    own = _Args("seg_scores")
    own("ids", ids, torch.int32, dim=3)
    B, H, W = ids.shape
    if scores.dim() != 3 or planes.dim() != 2 or seg_u8.dim() != 4:
        raise ValueError("seg_scores: scores must be int64 [B, cap, 4], planes int32 [B, nlabels + 1] and seg_u8 uint8 "
                         "[P, 3, H, W]")
    cap, nl1, P = scores.shape[1], planes.shape[1], seg_u8.shape[0]
    a = L.SegScoresArgs()
    a.ids, a.labels = ids.data_ptr(), own("labels", labels, torch.uint8, (B, H, W))
    a.seg_u8, a.planes = own("seg_u8", seg_u8, torch.uint8, (P, 3, H, W)), own("planes", planes, torch.int32, (B, nl1))
    a.planes_host = own("planes_host", planes_host, torch.int32, (B, nl1), host=True)
    a.scores = own("scores", scores, torch.int64, (B, cap, 4))
    a.ws, a.ws_bytes = own("ws", ws, torch.uint8), ws.numel()
    a.B, a.H, a.W, a.cap, a.nlabels, a.P = B, H, W, cap, nl1 - 1, P
    own.device()
    L.check(L.lib().dfw_seg_scores(C.byref(a), _stream()), "dfw_seg_scores")


def seg_boundary_workspace(B, H, W, elem=1):
    """Bytes of seg_boundary's workspace for a [B, H, W] map of elem-byte values (1 | 4); 0 for sizes it refuses."""
    return int(L.lib().dfw_seg_boundary_workspace_bytes(int(B), int(H), int(W), int(elem)))


def seg_boundary_block():
    """(rows, cols, positions): the tile of seg_boundary's column pass and the positions a workgroup of its row pass
    covers -- the sizes at which its kernels change path."""
    r, c, p = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib().dfw_seg_boundary_block(C.byref(r), C.byref(c), C.byref(p)), "dfw_seg_boundary_block")
    return r.value, c.value, p.value


_BOUNDARY_METRICS = {"chessboard": 0, "euclidean": 1}


def seg_boundary(map, dist, ws, dmax, band=None, d=None, metric="chessboard", peaks=None, cap=None):
    """Capped distance to the contour, on caller-owned buffers only (objects.BoundaryBuffers holds a set).  The default
    metric, "chessboard", is described first; metric="euclidean" (below) writes SQUARED Euclidean distances.  map
    uint8 or int32 [B, H, W], values compared for equality only, 0 = background, every other value (255, values above 255
    and negative ints included) an object value.  Writes dist uint8 [B, H, W]: 0 where map == 0, else min(D, dmax + 1), D
    the smallest max(|dy|, |dx|) to a position outside the image or of another value (1 on the image's edge and next to
    another value); 1 <= dmax <= 254 and dmax + 1 means "deeper than dmax".  band (optional, map's dtype) receives the value
    where 1 <= dist <= d and 0 elsewhere, 1 <= d <= dmax, from the same launch.  ws: a uint8 buffer of at least
    seg_boundary_workspace(B, H, W, map.element_size()) bytes, which needs no initialisation.  Two launches, no host
    synchronisation, no memset node, no atomics: the call can be captured.  Returns None.

    metric="euclidean": dist is uint16 [B, H, W] and receives 0 where map == 0, else min(D2, (dmax + 1)^2), D2 the smallest
    dy^2 + dx^2 to a position outside the image or of another value; (dmax + 1)^2 means "at least dmax + 1 away".  band
    receives the value where 1 <= dist <= d^2.  The workspace is the same.  peaks (optional, int64 [B, cap], int32 id maps
    only; cap defaults to its second size): row k - 1 receives the maximum over the pixels (y, x) of id k of (dist << 32) |
    (0xFFFFFFFF - (y * W + x)) -- the squared radius of the object's largest inscribed circle and, among equals, its first
    centre -- and 0 when id k has no pixel; ids outside 1..cap are not counted.  Two launches, three with peaks (a library
    kernel zeroes the table, the column pass reduces it with integer atomic maxima: order-free)."""
    own = _Args("seg_boundary")
    own("map", map, (torch.uint8, torch.int32), dim=3)
    if metric not in _BOUNDARY_METRICS:
        raise ValueError(f"seg_boundary: metric must be one of {sorted(_BOUNDARY_METRICS)}, got {metric!r}")
    B, H, W = map.shape
    a = L.SegBoundaryArgs()
    a.metric = _BOUNDARY_METRICS[metric]
    a.map, a.dist = map.data_ptr(), own("dist", dist, torch.uint16 if a.metric else torch.uint8, (B, H, W))
    a.ws, a.ws_bytes = own("ws", ws, torch.uint8), ws.numel()
    if (band is None) != (d is None):
        raise ValueError("seg_boundary: band and d go together")
    if band is not None:
        a.band, a.d = own("band", band, map.dtype, (B, H, W)), int(d)
    if peaks is not None:
        if not a.metric or map.dtype != torch.int32 or peaks.dim() != 2:
            raise ValueError("seg_boundary: peaks (int64 [B, cap]) go with metric='euclidean' and an int32 id map")
        a.cap = peaks.shape[1] if cap is None else int(cap)
        a.peaks = own("peaks", peaks, torch.int64, (B, a.cap))
    elif cap is not None:
        raise ValueError("seg_boundary: cap goes with peaks")
    a.elem, a.B, a.H, a.W, a.dmax = map.element_size(), B, H, W, int(dmax)
    own.device()
    L.check(L.lib().dfw_seg_boundary(C.byref(a), _stream()), "dfw_seg_boundary")


def seg_boundary_counts(pred, pdist, gt, gdist, counts, d):
    """Per-class counts of two boundary bands, on caller-owned buffers only: pred and gt uint8 [B, H, W] label maps, pdist
    and gdist their seg_boundary dist maps, d the band's width (at most the dmax the maps were made with).  Per pixel:
    dropped when gt > nlabels (255 included); l = pred if 1 <= pdist <= d else 0, g = gt if 1 <= gdist <= d else 0;
    predicted[l]++ when l <= nlabels, truth[g]++, intersection[l]++ when l == g.  Writes counts int64 [B, 2, nlabels + 1] =
    (intersections, unions), seg_labels' layout: metrics.boundary_iou(counts) is Boundary IoU per class.  nlabels is the
    buffer's shape.  gdist is the distance of gt as given, so a class pixel beside a 255 region lies in the band.  Two
    launches, no host synchronisation, no memset node: the call can be captured.  Returns None.

    pdist and gdist may both be the uint16 squared maps of seg_boundary(metric="euclidean"); a pixel then lies in the band
    when 1 <= dist <= d * d."""
    own = _Args("seg_boundary_counts")
    own("pred", pred, torch.uint8, dim=3)
    B, H, W = pred.shape
    if counts.dim() != 3:
        raise ValueError("seg_boundary_counts: counts must be int64 [B, 2, nlabels + 1]")
    a = L.SegBoundaryCountsArgs()
    kind = torch.uint16 if pdist.dtype == torch.uint16 else torch.uint8      # both maps are of pdist's kind
    a.pred, a.pdist = pred.data_ptr(), own("pdist", pdist, kind, (B, H, W))
    a.gt, a.gdist = own("gt", gt, torch.uint8, (B, H, W)), own("gdist", gdist, kind, (B, H, W))
    a.counts = own("counts", counts, torch.int64, (B, 2, counts.shape[2]))
    a.B, a.H, a.W, a.d, a.nlabels = B, H, W, int(d), counts.shape[2] - 1
    a.dist_elem = 2 if kind == torch.uint16 else 0
    own.device()
    L.check(L.lib().dfw_seg_boundary_counts(C.byref(a), _stream()), "dfw_seg_boundary_counts")
