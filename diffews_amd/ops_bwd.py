"""Host-side wrappers of the backward kernels (include/diffews_hip.h, "Training step").

Counterpart of ops.py for the training step of
/root/reference/train_tools/train_icl_multitask_nocrop_nearest_nshot_v3.py:1374-1396: torch tensors carry device
memory and the current stream only; every gradient is computed by libdiffews_hip.so.  Activation gradients are
NHWC / [rows, C] tensors in the engine storage dtype, parameter gradients fp32.
"""
import ctypes as C

import torch

from . import _lib as L
from .ops import _Args, _dt, _p, _stream, _f32


def _ws(nbytes, device):
    return torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.float32, device=device)


def gemm_tn(dy, x, n=None, kc=None, out=None, taps=1, geom=None, accumulate=False, scale=1.0, batch=1, batch2=1,
            strides=(0, 0, 0, 0), M=None, lda=None, ldb=None, out_strides=(0, 0, 0)):
    """out[b][n][tap][k] (+)= scale * sum_m dy[m][n] * x[row(m, tap)][k]   (fp32).
    dy [M, >=n] / x [rows, >=kc] are 2-D (or NHWC) storage-dtype tensors whose last dim is contiguous.
    geom = (Hi, Wi, Ho, Wo, stride, pad, ups) for taps == 9 (the forward conv's geometry)."""
    arg = _Args("gemm_tn")
    arg.need(dy.dim() >= 1 and x.dim() >= 1, "dy and x need at least one dimension")
    dy2 = dy.reshape(-1, dy.shape[-1]) if dy.dim() != 2 else dy
    x2 = x.reshape(-1, x.shape[-1]) if x.dim() != 2 else x
    arg("dy", dy2, dense=False)
    arg("x", x2, dy2.dtype, dense=False)
    M = M if M is not None else dy2.shape[0]
    n = n if n is not None else dy2.shape[1]
    kc = kc if kc is not None else x2.shape[1]
    nb = max(1, batch) * max(1, batch2)
    if out is None:
        out = torch.empty(nb, n, taps, kc, dtype=torch.float32, device=dy.device)
        arg.need(not accumulate, "accumulate needs an out to add to")
    ldo_n, ldo_t, ldo_b = [int(v) for v in out_strides]
    a = L.GemmTnArgs()
    a.A, a.B = dy2.data_ptr(), x2.data_ptr()
    a.out = arg("out", out, torch.float32, dense=False, extent=(nb - 1) * (ldo_b or n * (ldo_n or taps * (ldo_t or kc)))
                + (n - 1) * (ldo_n or taps * (ldo_t or kc)) + (taps - 1) * (ldo_t or kc) + kc)
    a.a_elems = dy2.numel() if dy2.is_contiguous() else (dy2.shape[0] - 1) * dy2.stride(0) + dy2.shape[1]
    a.b_elems = x2.numel() if x2.is_contiguous() else (x2.shape[0] - 1) * x2.stride(0) + x2.shape[1]
    if nb > 1:   # batched problems address beyond one matrix: the extents are those of the whole buffers
        a.a_elems = dy.numel() if dy.is_contiguous() else a.a_elems
        a.b_elems = x.numel() if x.is_contiguous() else a.b_elems
    a.M, a.N, a.Kc = M, n, kc
    a.lda = lda if lda is not None else dy2.stride(0)
    a.ldb = ldb if ldb is not None else x2.stride(0)
    a.taps = taps
    if taps == 9:
        a.Hi, a.Wi, a.Ho, a.Wo, a.stride, a.pad, a.ups = [int(v) for v in geom]
    a.batch, a.batch2 = batch, batch2
    a.strideA, a.strideB, a.strideA2, a.strideB2 = [int(v) for v in strides]
    a.ldo_n, a.ldo_t, a.ldo_b = ldo_n, ldo_t, ldo_b
    span = (max(1, batch) - 1) * a.strideA + (max(1, batch2) - 1) * a.strideA2 + (M - 1) * a.lda + n
    arg.need(span <= a.a_elems, "dy must span {} elements for M {}, n {}, lda {} and the batch strides, it has {}", span, M, n, a.lda, a.a_elems)
    span = (max(1, batch) - 1) * a.strideB + (max(1, batch2) - 1) * a.strideB2 + (x2.shape[0] - 1 if taps == 9 else M - 1) * a.ldb + kc
    arg.need(nb > 1 and taps == 9 or span <= a.b_elems, "x must span {} elements for kc {}, ldb {} and the batch strides, it has {}", span, kc, a.ldb, a.b_elems)
    a.scale, a.accumulate, a.dtype = scale, int(accumulate), _dt(dy2)
    arg.device()
    lib = L.lib()
    nbytes = lib.dfw_gemm_tn_workspace_bytes(C.byref(a))
    if nbytes == 0:
        L.check(lib.dfw_gemm_tn(C.byref(a), _stream()), "dfw_gemm_tn")   # reports the argument error
    ws = _ws(nbytes, dy.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    L.check(lib.dfw_gemm_tn(C.byref(a), _stream()), "dfw_gemm_tn")
    return out


def colsum(x, segs=1, out=None, accumulate=False, scale=1.0):
    """Column sums of x [rows, N] (storage dtype) per segment of rows / segs rows -> fp32 [segs, N]."""
    arg = _Args("colsum")
    x2, rows, N, ldo = _colsum_args(arg, x, out, segs)
    if out is None:
        out = torch.empty(segs, N, dtype=torch.float32, device=x.device)
        arg.need(not accumulate, "accumulate needs an out to add to")
    dt = _dt(x2)
    arg.device()
    lib = L.lib()
    nbytes = lib.dfw_colsum_workspace_bytes(rows // segs, segs, N)
    ws = _ws(nbytes, x.device)
    L.check(lib.dfw_colsum(x2.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, rows // segs, segs, N, x2.stride(0), ldo,
                           float(scale), int(accumulate), dt, _stream()), "dfw_colsum")
    return out


def _colsum_args(arg, x, out, segs):
    """What colsum and ColsumQueue.add check: x [..., N] with a unit last stride as rows x2 [rows, N], rows a multiple of
    segs; out (None: colsum allocates it) fp32 with a unit last stride that holds segs rows of N at its row stride.
    Returns (x2, rows, N, ldo)."""
    arg.need(x.dim() >= 1 and x.numel() > 0, "x must be [..., N] and not empty, got {}", x.shape)
    x2 = x.reshape(-1, x.shape[-1])
    arg("x", x2, dense=False)
    rows, N = x2.shape
    arg.need(segs >= 1 and rows % segs == 0, "the {} rows of x are not a multiple of segs {}", rows, segs)
    ldo = out.stride(0) if out is not None and out.dim() == 2 else N
    if out is not None:
        arg("out", out, torch.float32, dense=False, extent=(segs - 1) * ldo + N)
    return x2, rows, N, ldo


class ColsumQueue:
    """Deferred column sums of a backward walk: add() records what colsum() would launch (and keeps the operand alive),
    flush() issues everything recorded so far in TWO launches (dfw_colsum_batch) instead of two per item -- ~190 bias /
    time-projection gradients per training step.  Results are identical to colsum()'s (same partial-sum plan per item, same
    fold order).  flush() must run before anything reads an output (the trainer flushes before the time-projection closure,
    before it reports gradients as final to the gradient reducer, and at the end of the walk)."""

    def __init__(self):
        self.items, self.keep = [], []

    def add(self, x, out, segs=1, accumulate=False, scale=1.0):
        arg = _Args("ColsumQueue.add")
        x2, rows, N, ldo = _colsum_args(arg, x, out, segs)
        arg.need(N % 8 == 0 and x2.stride(0) % 8 == 0, "N and the row stride of x must be multiples of 8, got {} and {}", N, x2.stride(0))
        arg.need(not self.items or self.items[0][-1] == _dt(x2), "one storage dtype per batch")
        arg.need(not self.keep or self.keep[0][0].device == x2.device, "one device per batch")
        arg.device()
        self.items.append((x2.data_ptr(), out.data_ptr(), rows // segs, segs, N, x2.stride(0), ldo, float(scale), int(accumulate), _dt(x2)))
        self.keep.append((x2, out))

    def flush(self):
        if not self.items:
            return
        import struct
        lib = L.lib()
        rows, b1, b2, off = [], 0, 0, 0
        ch, rp = C.c_int32(0), C.c_int32(0)
        for (xp, op, rps, segs, N, ldx, ldo, scale, acc, _) in self.items:
            L.check(lib.dfw_colsum_plan(rps, C.byref(ch), C.byref(rp)), "dfw_colsum_plan")
            sbits = struct.unpack("<i", struct.pack("<f", scale))[0]
            rows.append([xp, op, rps, segs, N, ldx, ldo, sbits, acc, ch.value, rp.value, off, b1, b2, 0, 0])
            b1 += ((N + 255) // 256) * ch.value * segs
            b2 += ((N + 15) // 16) * segs
            off += segs * ch.value * N
        dev = self.keep[0][0].device
        table = torch.empty(len(rows), 16, dtype=torch.int64, device=dev)
        for i0 in range(0, len(rows), 24):          # the records travel as kernel arguments (capture-safe: no pinned memory)
            chunk = rows[i0:i0 + 24]
            flat = (C.c_int64 * (16 * len(chunk)))(*[v for r in chunk for v in r])
            L.check(lib.dfw_table_write(table.data_ptr(), i0, flat, len(chunk), _stream()), "dfw_table_write")
        ws = torch.empty(max(off, 1), dtype=torch.float32, device=dev)
        L.check(lib.dfw_colsum_batch(table.data_ptr(), len(rows), b1, b2, ws.data_ptr(), self.items[0][-1], _stream()), "dfw_colsum_batch")
        self.items, self.keep = [], []


def groupnorm_bwd(x, dy, mean_rstd, gamma, beta, groups, silu, dgamma=None, dbeta=None, accumulate=False, grad_scale=1.0, dx_add=None):
    """-> dx (like x).  x, dy NHWC (or [B, HW, C]) contiguous; mean_rstd [B, groups, 2] fp32 from the forward.
    dx_add: a gradient x already has (same memory layout as x), added in the kernel (fp32 sum, one rounding)."""
    arg = _Args("groupnorm_bwd")
    arg("x", x)
    arg.need(x.dim() >= 2 and x.numel() > 0, "x must be [B, ..., C] and not empty, got {}", x.shape)
    arg("dy", dy, x.dtype, x.shape)
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc)
    dx = torch.empty_like(x)
    a = L.GroupNormBwdArgs()
    a.x, a.dy, a.dx = x.data_ptr(), dy.data_ptr(), dx.data_ptr()
    a.gamma, a.beta = arg.f32("gamma", gamma, Cc), arg.f32("beta", beta, Cc)
    a.mean_rstd = arg("mean_rstd", mean_rstd, torch.float32, elems=B * groups * 2)
    a.dgamma, a.dbeta = arg.f32("dgamma", dgamma, Cc), arg.f32("dbeta", dbeta, Cc)
    a.B, a.HW, a.C, a.groups, a.ldx, a.lddy, a.lddx = B, HW, Cc, groups, Cc, Cc, Cc
    a.silu, a.accumulate, a.grad_scale, a.dtype = int(silu), int(accumulate), grad_scale, _dt(x)
    if dx_add is not None:
        a.dx_add = arg("dx_add", dx_add, x.dtype, elems=x.numel())
    arg.device()
    lib = L.lib()
    nbytes = lib.dfw_groupnorm_bwd_workspace_bytes(C.byref(a))
    ws = _ws(nbytes, x.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    L.check(lib.dfw_groupnorm_bwd(C.byref(a), _stream()), "dfw_groupnorm_bwd")
    return dx


def layernorm_bwd(x, dy, gamma, dgamma, dbeta, eps=1e-5, accumulate=False, grad_scale=1.0, dx_add=None):
    arg = _Args("layernorm_bwd")
    arg("x", x, dim=2, dense=False)
    arg("dy", dy, x.dtype, x.shape, dense=False)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    a = L.LayerNormBwdArgs()
    a.x, a.dy, a.dx, a.gamma = x.data_ptr(), dy.data_ptr(), dx.data_ptr(), arg.f32("gamma", gamma, x.shape[1])
    arg.need(dgamma is not None and dbeta is not None, "dgamma and dbeta are required")
    a.dgamma, a.dbeta = arg.f32("dgamma", dgamma, x.shape[1]), arg.f32("dbeta", dbeta, x.shape[1])
    a.rows, a.C, a.ldx, a.lddy, a.lddx = x.shape[0], x.shape[1], x.stride(0), dy.stride(0), dx.stride(0)
    a.eps, a.accumulate, a.grad_scale, a.dtype = eps, int(accumulate), grad_scale, _dt(x)
    if dx_add is not None:     # rows at dx's stride (dx is contiguous)
        a.dx_add = arg("dx_add", dx_add, x.dtype, elems=x.numel())
    arg.device()
    lib = L.lib()
    nbytes = lib.dfw_layernorm_bwd_workspace_bytes(x.shape[0], x.shape[1])
    ws = _ws(nbytes, x.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    L.check(lib.dfw_layernorm_bwd(C.byref(a), _stream()), "dfw_layernorm_bwd")
    return dx


def geglu_fwd(pre):
    """pre [rows, 2H] in the packed column order (packing.pack_geglu) -> [rows, H]."""
    arg = _Args("geglu_fwd")
    arg("pre", pre, dim=2)
    arg.device()
    rows, H2 = pre.shape
    out = torch.empty(rows, H2 // 2, dtype=pre.dtype, device=pre.device)
    L.check(L.lib().dfw_geglu(pre.data_ptr(), None, out.data_ptr(), rows, H2 // 2, _dt(pre), _stream()), "dfw_geglu")
    return out


def geglu_bwd(pre, dout):
    arg = _Args("geglu_bwd")
    arg("pre", pre, dim=2)
    arg("dout", dout, pre.dtype, (pre.shape[0], pre.shape[1] // 2))
    arg.device()
    dpre = torch.empty_like(pre)
    L.check(L.lib().dfw_geglu(pre.data_ptr(), dout.data_ptr(), dpre.data_ptr(), pre.shape[0], pre.shape[1] // 2, _dt(pre),
                              _stream()), "dfw_geglu")
    return dpre


def _ew(arg, mode, a, b, y, rows, Cc, lda=0, c0=0, H=0, W=0):
    """dfw_elementwise on operands the caller has checked through `arg`; y is the caller's fresh output."""
    arg.need(y.numel() > 0, "a must not be empty, got {}", a.shape)
    dt = _dt(a)
    arg.device()
    L.check(L.lib().dfw_elementwise(mode, a.data_ptr(), _p(b), y.data_ptr(), rows, Cc, lda, c0, H, W, dt, _stream()),
            "dfw_elementwise")
    return y


def add(a, b):
    arg = _Args("add")
    arg("a", a)
    arg("b", b, a.dtype, a.shape)
    Cc = max(a.shape[-1], 1) if a.dim() else 1
    return _ew(arg, 0, a, b, torch.empty_like(a), a.numel() // Cc, Cc)


def slice_channels(a, c0, Cc):
    """a[..., c0:c0+Cc] as a contiguous tensor (backward of concat_channels)."""
    arg = _Args("slice_channels")
    arg("a", a)
    arg.need(a.dim() >= 1 and 0 <= c0 and 0 < Cc and c0 + Cc <= a.shape[-1], "channels {}..{} leave the {} of a", c0, c0 + Cc, a.shape[-1])
    y = torch.empty(*a.shape[:-1], Cc, dtype=a.dtype, device=a.device)
    return _ew(arg, 1, a, None, y, a.numel() // a.shape[-1], Cc, lda=a.shape[-1], c0=c0)


def zero_stuff2x(a):
    """[B, H, W, C] -> [B, 2H, 2W, C] with a at the even positions, zeros elsewhere."""
    arg = _Args("zero_stuff2x")
    arg("a", a, dim=4)
    B, H, W, Cc = a.shape
    y = torch.empty(B, 2 * H, 2 * W, Cc, dtype=a.dtype, device=a.device)
    return _ew(arg, 2, a, None, y, B * 4 * H * W, Cc, H=H, W=W)


def pool2x2_sum(a):
    """[B, 2H, 2W, C] -> [B, H, W, C], sums of the 2x2 blocks (backward of the nearest-2x upsample)."""
    arg = _Args("pool2x2_sum")
    arg("a", a, dim=4)
    B, H2, W2, Cc = a.shape
    arg.need(H2 % 2 == 0 and W2 % 2 == 0, "a must be [B, 2H, 2W, C], got {}", a.shape)
    y = torch.empty(B, H2 // 2, W2 // 2, Cc, dtype=a.dtype, device=a.device)
    return _ew(arg, 3, a, None, y, B * (H2 // 2) * (W2 // 2), Cc, H=H2 // 2, W=W2 // 2)


def nchw_to_nhwc(x, dtype, cp=8, scale=1.0):
    """NCHW fp32 -> NHWC `dtype` with channels zero-padded to cp."""
    arg = _Args("nchw_to_nhwc")
    arg("x", x, torch.float32, dim=4)
    arg.need(x.shape[1] <= cp, "x has {} channels, more than cp {}", x.shape[1], cp)
    arg.device()
    B, Cc, H, W = x.shape
    y = torch.empty(B, H, W, cp, dtype=dtype, device=x.device)
    L.check(L.lib().dfw_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), B, Cc, H * W, cp, float(scale), L.BF16 if dtype == torch.bfloat16 else L.F16,
                                     _stream()), "dfw_nchw_to_nhwc")
    return y


def mse_loss(pred, target, dtype, loss_scale=1.0, dpred_out=None, dpred_nchw_out=None):
    """-> (loss fp32 tensor [1], dpred NHWC [B, H, W, 8] in `dtype` = 2 (pred - target) / numel * loss_scale).
    dpred_out: zero-initialised destination (e.g. the query rows of a larger batch); dpred_nchw_out: optional fp32
    [B, C, H, W] that receives the same rounded values."""
    arg = _Args("mse_loss")
    arg("pred", pred, torch.float32, dim=4)
    arg("target", target, torch.float32, pred.shape)
    B, Cc, H, W = pred.shape
    arg.need(Cc <= 8, "pred has {} channels, more than the 8 of dpred", Cc)
    dpred = dpred_out if dpred_out is not None else torch.zeros(B, H, W, 8, dtype=dtype, device=pred.device)
    arg("dpred_out", dpred, dtype, (B, H, W, 8))
    if dpred_nchw_out is not None:
        arg("dpred_nchw_out", dpred_nchw_out, torch.float32, pred.shape)
    arg.device()
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    ws = torch.empty(256, dtype=torch.float32, device=pred.device)
    L.check(L.lib().dfw_mse_loss(pred.data_ptr(), target.data_ptr(), dpred.data_ptr(), _p(dpred_nchw_out), loss.data_ptr(),
                                 ws.data_ptr(), B, Cc, H * W, float(loss_scale), L.BF16 if dtype == torch.bfloat16 else L.F16,
                                 _stream()), "dfw_mse_loss")
    return loss, dpred


def fsa_attention_bwd(qkv, out, dout, lse, heads, nshot=0, n_plain=0, scale=None, key_split=True):
    """qkv [B, N, 3C] (q pre-scaled), out / dout [B, N, C], lse [B, heads, N] -> dqkv [B, N, 3C]."""
    arg = _Args("fsa_attention_bwd")
    arg("qkv", qkv, dim=3)
    B, N, C3 = qkv.shape
    Cq = heads * 64
    arg.need(C3 == 3 * Cq, "qkv must be [B, N, {}] for {} heads, got {}", 3 * Cq, heads, qkv.shape)
    arg("out", out, qkv.dtype, (B, N, Cq))
    arg("dout", dout, qkv.dtype, (B, N, Cq))
    arg("lse", lse, torch.float32, (B, heads, N))
    dt = _dt(qkv)
    arg.device()
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(2, B, heads, N, dtype=torch.float32, device=qkv.device)   # (-delta | -lse), see the header
    a = L.FsaBwdArgs()
    a.qkv, a.out, a.dout, a.lse, a.delta, a.dqkv = qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr()
    a.delta_bytes = delta.numel() * 4
    a.batch, a.heads, a.n, a.nshot, a.n_plain = B, heads, N, nshot, n_plain
    a.ld, a.ldo, a.ldd = C3, Cq, C3
    a.scale = scale if scale is not None else 64 ** -0.5
    a.dtype = dt
    lib = L.lib()
    nbytes = lib.dfw_fsa_attention_bwd_workspace_bytes(C.byref(a)) if (nshot >= 2 and key_split) else 0
    if nbytes:      # dQ key split of the bank readers (many shots)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=qkv.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    from . import ops as _ops
    if _ops.gemm_hook is not None:      # bench.py roofline leg: the dQ + dK/dV kernels of this launch (5 GEMMs = 2.5 x the forward's 2)
        keys = n_plain * N + (B - n_plain) * (N + nshot * N)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.dfw_fsa_attention_bwd(C.byref(a), _stream()), "dfw_fsa_attention_bwd")
        e1.record()
        _ops.gemm_hook("fsa_attention_bwd", 10.0 * heads * 64 * N * keys, e0, e1, (B, heads, N, keys))
        return dqkv
    L.check(lib.dfw_fsa_attention_bwd(C.byref(a), _stream()), "dfw_fsa_attention_bwd")
    return dqkv


def _qkv_args(arg, q, k, v, heads, dk_out, dv_out, same_strides=True):
    """What attention_bwd and cross_attention_bwd check alike: q [B, N, heads*64] and k / v [B, L, heads*64] views with a
    unit last stride (k and v with equal strides where the kernel has one pair of them), dk_out / dv_out shaped like k with
    equal strides.  Returns (B, N, heads*64, L)."""
    arg("q", q, dim=3, dense=False)
    B, N, Cq = q.shape
    arg.need(Cq == heads * 64, "q must be [B, N, {}] for {} heads, got {}", heads * 64, heads, q.shape)
    arg("k", k, q.dtype, dim=3, dense=False)
    arg.need(k.shape[0] == B and k.shape[2] == Cq, "k must be [{}, L, {}], got {}", B, Cq, k.shape)
    arg("v", v, q.dtype, k.shape, dense=False)
    arg.need(not same_strides or k.stride() == v.stride(), "k and v must have equal strides, got {} and {}", k.stride(), v.stride())
    arg("dk_out", dk_out, q.dtype, k.shape, dense=False)
    arg("dv_out", dv_out, q.dtype, k.shape, dense=False)
    arg.need(dk_out.stride() == dv_out.stride(), "dk_out and dv_out must have equal strides, got {} and {}", dk_out.stride(), dv_out.stride())
    return B, N, Cq, k.shape[1]


def attention_bwd(q, k, v, out, dout, lse, heads, dk_out, dv_out, scale=None, q_split=True):
    """Flash backward with queries and keys / values in their own tensors (attn2 on the MFMA path).  q [B, N, heads*64]
    PRE-SCALED (linear(..., colscale=(C, FSA_QSCALE))); k / v [B, L, heads*64] column slices of one buffer; out / dout
    [B, N, heads*64] contiguous; lse [B, heads, N] from fsa_attention(..., lse=); dk_out / dv_out: views that receive
    dK / dV.  -> dq [B, N, heads*64] with respect to the unscaled projection output."""
    arg = _Args("attention_bwd")
    B, N, Cq, Lc = _qkv_args(arg, q, k, v, heads, dk_out, dv_out)
    arg.need(v.data_ptr() >= k.data_ptr(), "v must lie behind k in one buffer")
    arg("out", out, q.dtype, (B, N, Cq))
    arg("dout", dout, q.dtype, (B, N, Cq))
    arg("lse", lse, torch.float32, (B, heads, N))
    dt = _dt(q)
    arg.device()
    dq = torch.empty(B, N, Cq, dtype=q.dtype, device=q.device)
    delta = torch.empty(2, B, heads, N, dtype=torch.float32, device=q.device)
    a = L.AttnBwdArgs()
    a.q, a.k, a.v, a.out, a.dout, a.lse, a.delta = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr()
    a.delta_bytes = delta.numel() * 4
    a.dq, a.dk, a.dv = dq.data_ptr(), dk_out.data_ptr(), dv_out.data_ptr()
    a.batch, a.heads, a.n_q, a.n_kv = B, heads, N, Lc
    a.ldq, a.ldkv, a.ldo, a.lddq, a.lddkv = q.stride(1), k.stride(1), Cq, Cq, dk_out.stride(1)
    a.q_bs, a.kv_bs, a.o_bs, a.dq_bs, a.dkv_bs = q.stride(0), k.stride(0), N * Cq, N * Cq, dk_out.stride(0)
    a.scale = scale if scale is not None else 64 ** -0.5
    a.dtype = dt
    nbytes = L.lib().dfw_attention_bwd_workspace_bytes(C.byref(a)) if q_split else 0
    if nbytes:      # short key axis: query split of the dK/dV kernel
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    L.check(L.lib().dfw_attention_bwd(C.byref(a), _stream()), "dfw_attention_bwd")
    return dq


def cross_attention_bwd(q, k, v, dout, heads, dk_out, dv_out, scale=None):
    """attn2 backward.  q / dout [B, N, heads*64]; k / v [B, L, heads*64] views; dk_out / dv_out: [B, L, heads*64]
    views (column slices of the fused prompt-K/V gradient buffer) that receive dK / dV.  -> dq [B, N, heads*64]."""
    arg = _Args("cross_attention_bwd")
    B, N, Cq, Lc = _qkv_args(arg, q, k, v, heads, dk_out, dv_out, same_strides=False)
    arg("dout", dout, q.dtype, (B, N, Cq), dense=False)
    dt = _dt(q)
    arg.device()
    dq = torch.empty(B, N, Cq, dtype=q.dtype, device=q.device)
    a = L.XattnBwdArgs()
    a.q, a.k, a.v, a.dout, a.dq, a.dk, a.dv = q.data_ptr(), k.data_ptr(), v.data_ptr(), dout.data_ptr(), dq.data_ptr(), dk_out.data_ptr(), dv_out.data_ptr()
    a.batch, a.heads, a.n_q, a.L = B, heads, N, Lc
    a.ldq, a.ldk, a.ldv, a.ldo, a.lddq, a.lddkv = q.stride(1), k.stride(1), v.stride(1), dout.stride(1), Cq, dk_out.stride(1)
    a.q_bs, a.k_bs, a.v_bs, a.o_bs, a.dq_bs, a.dkv_bs = q.stride(0), k.stride(0), v.stride(0), dout.stride(0), N * Cq, dk_out.stride(0)
    a.scale = scale if scale is not None else 64 ** -0.5
    a.dtype = dt
    lib = L.lib()
    nbytes = lib.dfw_cross_attention_bwd_workspace_bytes(B, heads, N, Lc)
    ws = _ws(nbytes, q.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    L.check(lib.dfw_cross_attention_bwd(C.byref(a), _stream()), "dfw_cross_attention_bwd")
    return dq


def silu(a, dy=None):
    """silu(a), or dy * silu'(a) when dy is given (storage dtype, any shape, contiguous)."""
    arg = _Args("silu")
    arg("a", a)
    if dy is not None:
        arg("dy", dy, a.dtype, a.shape)
    dt = _dt(a)
    arg.device()
    y = torch.empty_like(a)
    L.check(L.lib().dfw_silu(a.data_ptr(), _p(dy), y.data_ptr(), a.numel(), dt, _stream()), "dfw_silu")
    return y


def sumsq(x):
    arg = _Args("sumsq")
    arg("x", x, torch.float32)
    arg.device()
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = torch.empty(1024, dtype=torch.float32, device=x.device)
    L.check(L.lib().dfw_sumsq(x.data_ptr(), out.data_ptr(), ws.data_ptr(), x.numel(), _stream()), "dfw_sumsq")
    return out


def linear_wt(w):
    """W [N, K] (storage dtype, contiguous) -> W^T [K, N]: the weight of the data-gradient GEMM dX = dY W."""
    arg = _Args("linear_wt")
    arg("w", w, dim=2)
    arg.device()
    N, K = w.shape
    y = torch.empty(K, N, dtype=w.dtype, device=w.device)
    L.check(L.lib().dfw_weight_relayout(w.data_ptr(), y.data_ptr(), N, K, K, N, 1, 0, 0, 0, _stream()), "dfw_weight_relayout")
    return y


def conv3x3_wd(w, cout):
    """packed conv weight [Cout, 9*Cin] -> [Cin, 9*Cout] with mirrored taps (packing.pack_conv3x3_dgrad on device)."""
    arg = _Args("conv3x3_wd")
    arg("w", w, dim=2)
    arg.need(w.shape[0] == cout and w.shape[1] % 9 == 0, "w must be [{}, 9 * Cin], got {}", cout, w.shape)
    arg.device()
    cin = w.shape[1] // 9
    y = torch.empty(cin, 9 * cout, dtype=w.dtype, device=w.device)
    L.check(L.lib().dfw_weight_relayout(w.data_ptr(), y.data_ptr(), cout, cin, 9 * cin, 9 * cout, 9, cin, cout, 1, _stream()),
            "dfw_weight_relayout")
    return y


def relayout_table(entries, device):
    """entries: [(kind, w, y)] with kind 'T' (Linear W [N, K] -> y [K, N]) or 'D' (packed conv W [Cout, 9*Cin] ->
    y [Cin, 9*Cout], taps mirrored).  -> (device int64 table [n, 12], n, total_blocks) for weight_relayout_batch: the
    tensors' addresses are baked in, so the table is valid while they live."""
    rows, blk, arg = [], 0, _Args("relayout_table")
    for i, (kind, w, y) in enumerate(entries):
        arg(f"entries[{i}] w", w, dim=2)
        arg(f"entries[{i}] y", y, w.dtype, elems=w.numel())
        if kind == "T":
            N, K = w.shape
            R, Cc, ldx, ldy, nb, x_bs, y_bs, flip = N, K, K, N, 1, 0, 0, 0
        else:
            cout, cin = w.shape[0], w.shape[1] // 9
            R, Cc, ldx, ldy, nb, x_bs, y_bs, flip = cout, cin, 9 * cin, 9 * cout, 9, cin, cout, 1
        arg.need(R % 8 == 0 and Cc % 8 == 0 and (kind == "T" or 9 * Cc == w.shape[1]), "entries[{}] w must have sizes that are multiples of 8 (a conv weight [Cout, 9 * Cin]), got {}", i, w.shape)
        arg.need(w.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0, "entries[{}] w and y must be 16-byte aligned", i)
        rows.append([w.data_ptr(), y.data_ptr(), R, Cc, ldx, ldy, x_bs, y_bs, nb, flip, blk, 0])
        blk += ((Cc + 63) // 64) * ((R + 63) // 64) * nb
    arg.device()
    return torch.tensor(rows, dtype=torch.int64).to(device), len(rows), blk


def weight_relayout_batch(table):
    t, n, blocks = table
    arg = _Args("weight_relayout_batch")
    arg("table", t, torch.int64, elems=n * 12)
    arg.device()
    L.check(L.lib().dfw_weight_relayout_batch(t.data_ptr(), n, blocks, _stream()), "dfw_weight_relayout_batch")


def loss_grad(g, dtype, scale=1.0, dpred_out=None, dpred_nchw_out=None):
    """External d loss / d pred (NCHW fp32 [B, C, H, W]) -> the same two tensors mse_loss hands the backward:
    dpred NHWC [B, H, W, 8] in `dtype` = round(g * scale) (channels C..7 untouched) and its NCHW fp32 copy."""
    arg = _Args("loss_grad")
    arg("g", g, torch.float32, dim=4)
    B, Cc, H, W = g.shape
    arg.need(Cc <= 8, "g has {} channels, more than the 8 of dpred", Cc)
    dpred = dpred_out if dpred_out is not None else torch.zeros(B, H, W, 8, dtype=dtype, device=g.device)
    arg("dpred_out", dpred, dtype, (B, H, W, 8))
    if dpred_nchw_out is not None:
        arg("dpred_nchw_out", dpred_nchw_out, torch.float32, g.shape)
    arg.device()
    L.check(L.lib().dfw_loss_grad(g.data_ptr(), dpred.data_ptr(), _p(dpred_nchw_out), B, Cc, H * W, float(scale),
                                  L.BF16 if dtype == torch.bfloat16 else L.F16, _stream()), "dfw_loss_grad")
    return dpred


def to_f32(x, out, scale=1.0):
    """out (fp32) = x (storage dtype) * scale, flat contiguous buffers."""
    arg = _Args("to_f32")
    arg("x", x)
    arg("out", out, torch.float32, elems=x.numel())
    dt = _dt(x)
    arg.device()
    L.check(L.lib().dfw_convert_to_f32(x.data_ptr(), out.data_ptr(), x.numel(), float(scale), dt, _stream()), "dfw_convert_to_f32")
    return out


def adamw(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_sumsq=None,
          max_grad_norm=0.0, shadow=None, found_inf=None):
    arg, n = _Args("adamw"), param.numel()
    a = L.AdamWArgs()
    a.param, a.grad = arg("param", param, torch.float32), arg("grad", grad, torch.float32, elems=n)
    a.exp_avg, a.exp_avg_sq = arg("exp_avg", exp_avg, torch.float32, elems=n), arg("exp_avg_sq", exp_avg_sq, torch.float32, elems=n)
    a.grad_sumsq = arg.f32("grad_sumsq", grad_sumsq, 1)
    a.n, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = param.numel(), lr, betas[0], betas[1], eps, weight_decay
    a.max_grad_norm, a.step = max_grad_norm, step
    if found_inf is not None:
        a.found_inf = arg("found_inf", found_inf, torch.int32, extent=1)
    if shadow is not None:
        a.shadow, a.shadow_dtype = arg("shadow", shadow, elems=n), _dt(shadow)
    arg.device()
    L.check(L.lib().dfw_adamw(C.byref(a), _stream()), "dfw_adamw")
