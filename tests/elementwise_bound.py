"""Per-element error bound of a GEMM / conv kernel against an fp64 reference of the same operation.

The reference is computed in fp64 from the 16-bit operands the kernel reads (on whatever device they live), a conv3x3 as
nine shifted GEMMs over the zero-padded NHWC input (stride 2, the VAE's asymmetric pad 0 and fused nearest-2x upsampling
included), never through a library convolution.  The same expression is evaluated on absolute values (|A|.|W|, and
|bias| + |row bias| + |residual|, scaled by |scale|), and every output element y of dtype T must satisfy

    |y - r| <= u_T |r| + C_ACC 2^-24 (sqrt(K) |A||W| + |epilogue addends|) sqrt(splits) + floor_T

u_T is the unit roundoff of the output (2^-8 bf16, 2^-11 fp16, 2^-24 fp32), floor_T covers subnormal outputs.  C_ACC was
fixed before any GPU run and is not fitted to measurements.  SiLU / GEGLU propagate the pre-activation term through their
slope bound and add their own approximation error (rcp / exp, the Abramowitz-Stegun erf of csrc/common.h).

The boundary convs (ops.conv_small) have their own reference and chunk-sum checker below (conv_small_ref, cs_chunk_check):
fp32 operands, K = taps * Cin, the same bound without splits.

Unlike a global relative L2, this flags an error that stays inside one tile, one K-chunk or one image: one tile with one
64-deep K-chunk missing passes `rel(y, ref) < TOL` and fails here (tests/test_gemm_plans_cpu.py).
"""
import math

import torch

C_ACC = 8.0
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
FLOOR = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -149}
SILU_SLOPE, GELU_SLOPE = 1.1, 1.13          # max |silu'|, max |gelu'|
ERF_AS = 1.5e-7                             # |erf_as - erf| (Abramowitz-Stegun 7.1.26)
F64 = torch.float64


def conv_taps(x, stride=1, pad=1, ups=False):
    """NHWC x [B, H, W, C] -> (Ho, Wo, [9 x fp64 [B*Ho*Wo, C]]): the input column each output pixel reads at tap ky*3+kx,
    zero outside the map (ops.conv3x3's geometry: pad = top/left padding, bottom/right from the bounds)."""
    x = x.to(F64)
    if ups:
        assert stride == 1 and pad == 1
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, H, W, Cc = x.shape
    if ups or stride == 1:
        Ho, Wo = H, W
    elif pad:
        Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    else:
        Ho, Wo = H // 2, W // 2
    hp, wp = max(H + pad, (Ho - 1) * stride + 3), max(W + pad, (Wo - 1) * stride + 3)
    xp = x.new_zeros(B, hp, wp, Cc)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = []
    for ky in range(3):
        for kx in range(3):
            t = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            cols.append(t.reshape(B * Ho * Wo, Cc))
    return Ho, Wo, cols


def gemm_ref(a, w):
    """a [M, K], w [N, K] (16-bit) -> fp64 (a @ w^T, |a| @ |w|^T)."""
    a, w = a.to(F64), w.to(F64)
    return a @ w.t(), a.abs() @ w.abs().t()


def conv_ref(x, wp, stride=1, pad=1, ups=False):
    """NHWC x [B, H, W, Cin], packed w [Cout, 9*Cin] -> fp64 (S, |S|) [B*Ho*Wo, Cout] as nine shifted GEMMs."""
    cin = x.shape[-1]
    _, _, cols = conv_taps(x, stride, pad, ups)
    w = wp.to(F64)
    s = a = None
    for t, col in enumerate(cols):
        wt = w[:, t * cin:(t + 1) * cin]
        ds, da = col @ wt.t(), col.abs() @ wt.abs().t()
        s, a = (ds, da) if s is None else (s + ds, a + da)
    return s, a


def epilogue_ref(S, absS, K, bias=None, rowbias=None, rows_per_img=0, residual=None, out_scale=1.0, colscale=None,
                 act=None, geglu=False, splits=1):
    """fp64 reference r of the GEMM epilogue and its error allowance e (the bound minus u_T |r| and floor_T).
    S / absS [M, N] from gemm_ref / conv_ref; rowbias [imgs, N] is added to row m as rowbias[m // rows_per_img];
    colscale = (n, s): columns < n scaled by s instead of out_scale; act 'silu'; geglu: packing.pack_geglu's 64-column
    groups (32 value columns, then their 32 gate columns) -> [M, N / 2] (the GEGLU epilogues apply no output scale)."""
    M, N = S.shape
    dev = S.device
    add, aadd = torch.zeros_like(S), torch.zeros_like(S)
    if bias is not None:
        b = bias.to(dev, F64)[None, :]
        add, aadd = add + b, aadd + b.abs()
    if rowbias is not None:
        rb = rowbias.to(dev, F64)[torch.arange(M, device=dev) // rows_per_img]
        add, aadd = add + rb, aadd + rb.abs()
    if residual is not None:
        res = residual.reshape(M, N).to(dev, F64)
        add, aadd = add + res, aadd + res.abs()
    sc = torch.full((N,), float(out_scale), dtype=F64, device=dev)
    if colscale is not None:
        sc[:colscale[0]] = float(colscale[1])
    pre = (S + add) * sc
    e_pre = C_ACC * 2.0 ** -24 * (math.sqrt(K) * absS + aadd) * sc.abs() * math.sqrt(splits)
    if geglu:
        pv, pg = (t.reshape(M, N // 2) for t in pre.view(M, N // 64, 2, 32).unbind(2))
        ev, eg = (t.reshape(M, N // 2) for t in e_pre.view(M, N // 64, 2, 32).unbind(2))
        gel = 0.5 * pg * (1.0 + torch.erf(pg / math.sqrt(2.0)))
        r = pv * gel
        # A-S erf + the rcp / exp2 inside it, the 0.5 x (1 + erf) products, the final product (fp32)
        approx = pv.abs() * (0.5 * pg.abs() * (ERF_AS + 4 * 2.0 ** -24) + 3 * 2.0 ** -24 * gel.abs()) + 2.0 ** -24 * r.abs()
        return r, ev * gel.abs() + pv.abs() * GELU_SLOPE * eg + ev * GELU_SLOPE * eg + approx
    if act == "silu":
        r = pre * torch.sigmoid(pre)
        # exp through exp2(x log2 e) (|x| + 2 ulp), 1 + e, the hardware rcp (2 ulp), the product
        return r, SILU_SLOPE * e_pre + (pre.abs() + 6.0) * 2.0 ** -24 * r.abs()
    assert act is None, act
    return pre, e_pre


class Where:
    """Flat output index -> 'image, pixel row/column, channel, tile' text for a failure message.
    rows_per_img / Wo: conv geometry (Wo = 0: a plain GEMM, rows_per_img its row-bias image); tile = (BM, BN) of the
    planned kernel; patch: the kernel walks (BM / 16) x 16 pixel patches of one image instead of BM consecutive rows."""

    def __init__(self, N, rows_per_img=0, Wo=0, tile=None, patch=False, batch_rows=0):
        self.N, self.rpi, self.Wo, self.tile, self.patch, self.batch_rows = N, rows_per_img, Wo, tile, patch, batch_rows

    def __call__(self, flat):
        m, n = divmod(int(flat), self.N)
        out = []
        if self.batch_rows:
            b, m = divmod(m, self.batch_rows)
            out.append(f"batch {b}")
        img, pix = divmod(m, self.rpi) if self.rpi else (0, m)
        if self.Wo:
            out.append(f"image {img} pixel ({pix // self.Wo},{pix % self.Wo})")
        else:
            out.append(f"row {m}" + (f" (image {img})" if self.rpi else ""))
        out.append(f"channel {n}")
        if self.tile:
            bm, bn = self.tile
            if self.patch and self.Wo:
                oy, ox = divmod(pix, self.Wo)
                out.append(f"tile (image {img}, patch {(oy // (bm // 16)) * (self.Wo // 16) + ox // 16}, n-tile {n // bn})")
            else:
                out.append(f"tile ({m // bm}, {n // bn})")
        return ", ".join(out)


def check(y, r, e, out_dtype, where=None, label="", show=6):
    """Assert |y - r| <= u_T |r| + e + floor_T elementwise (y: any view with r's elements in r's row-major order).
    Returns the worst err / bound ratio; on failure the message names the `show` worst elements through `where`."""
    y64 = y.reshape(r.shape).to(r.device, F64)
    bound = U[out_dtype] * r.abs() + e + FLOOR[out_dtype]
    ratio = (y64 - r).abs() / bound
    ratio = torch.where(torch.isfinite(y64), ratio, torch.full_like(ratio, math.inf))
    worst = float(ratio.max())
    if not worst <= 1.0:
        flat = ratio.flatten()
        bad = int((flat > 1.0).sum())
        vals, idx = torch.topk(flat, min(show, flat.numel()))
        lines = []
        for v, i in zip(vals.tolist(), idx.tolist()):
            pos = where(i) if where is not None else f"element {i}"
            lines.append(f"  {pos}: y={float(y64.flatten()[i]):.6g} ref={float(r.flatten()[i]):.6g} ratio={v:.3g}")
        raise AssertionError(f"{label}: {bad} of {flat.numel()} elements outside the bound (worst ratio {worst:.3g})\n"
                             + "\n".join(lines))
    return worst


def gn_chunk_check(y, part, groups, bm, bn, label="", nonfinite=False):
    """Fused GroupNorm partial sums part [B, chunks, groups, 2] (sum, sum of squares) of the NHWC output y [B, Ho, Wo, N]
    against fp64 sums of y per (image, chunk, group).  Chunk c of an image is wave row wm = c % WGM (WGM = 8 / (bn / 64)
    wave rows of bh / WGM pixel rows each, bh = bm / 16) of the bh x 16 pixel patch c // WGM (patches row-major): the
    slot the epilogues of conv_patch / conv_patch8 / gemm8 / gemm_big write.  Tolerance: recursive fp32 summation of
    n terms in any order, n 2^-24 sum |y| (n + 1 for the squares).  Returns the worst err / tolerance ratio.
    nonfinite: see _nonfinite_slots."""
    B, Ho, Wo, N = y.shape
    cpg, wgm, bh = N // groups, 8 // (bn // 64), bm // 16
    band = bh // wgm
    assert tuple(part.shape) == (B, (Wo // 16) * (Ho // bh) * wgm, groups, 2), (tuple(part.shape), Ho, Wo, bm, bn)
    # [B, Ho / bh, WGM, band, Wo / 16, 16, groups, cpg] -> [B, patch, wm, group, band x 16 x cpg]
    v = y.to(F64).reshape(B, Ho // bh, wgm, band, Wo // 16, 16, groups, cpg)
    v = v.permute(0, 1, 4, 2, 6, 3, 5, 7).reshape(B, (Ho // bh) * (Wo // 16) * wgm, groups, band * 16 * cpg)
    n = v.shape[-1]
    s, q = v.sum(-1), (v * v).sum(-1)
    got = part.to(v.device, F64)
    tol_s = n * 2.0 ** -24 * v.abs().sum(-1) + 1e-30
    tol_q = (n + 1) * 2.0 ** -24 * q + 1e-30
    ratio = torch.maximum((got[..., 0] - s).abs() / tol_s, (got[..., 1] - q).abs() / tol_q)
    ratio = torch.where(torch.isfinite(got).all(-1), ratio, torch.full_like(ratio, math.inf))
    if nonfinite:
        ratio = _nonfinite_slots(ratio, s, q, got, label)
    worst = float(ratio.max())
    if not worst <= 1.0:
        b, c, g = [int(t) for t in torch.nonzero(ratio == ratio.max())[0]]
        raise AssertionError(f"{label}: fused GroupNorm sums off (worst ratio {worst:.3g}) at image {b}, chunk {c} "
                             f"(patch {c // wgm}, wave row {c % wgm}), group {g}: got {got[b, c, g].tolist()}, "
                             f"fp64 {[float(s[b, c, g]), float(q[b, c, g])]}")
    return worst


def _nonfinite_slots(ratio, s, q, got, label):
    """nonfinite=True of the chunk checkers (tests/nonfinite.py): a slot whose stored values sum to a non-finite number
    must hold a non-finite sum and a non-finite sum of squares; such slots then count as exact (ratio 0), every other
    slot keeps its ratio.  Finite y never reaches this."""
    expect = ~(torch.isfinite(s) & torch.isfinite(q))
    lost = expect & torch.isfinite(got).any(-1)
    if bool(lost.any()):
        b, c, g = [int(t) for t in torch.nonzero(lost)[0]]
        raise AssertionError(f"{label}: fused GroupNorm sums finite over non-finite outputs at image {b}, chunk {c}, "
                             f"group {g}: got {got[b, c, g].tolist()}")
    return torch.where(expect, torch.zeros_like(ratio), ratio)


def conv_small_ref(x, w, bias, taps, in_scale=1.0, out_scale=1.0):
    """Boundary conv (ops.conv_small): NCHW fp32 x [B, Cin, H, W], fp32 w [Cout, taps, Cin], fp32 bias or None ->
    fp64 (r, e) [B*H*W, Cout] in NHWC order, as `taps` shifted products over the zero-padded input (pad 1 for 9 taps,
    none for 1), in_scale applied to the input, bias added, out_scale last;
    e = C_ACC 2^-24 (sqrt(K) |x in_scale|.|w| + |bias|) |out_scale|, K = taps * Cin."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    w = w.reshape(Cout, taps, Cin).to(F64)
    pad = 1 if taps == 9 else 0
    assert taps in (1, 9)
    xs = x.to(F64) * float(in_scale)
    xp = xs.new_zeros(B, Cin, H + 2 * pad, W + 2 * pad)
    xp[:, :, pad:pad + H, pad:pad + W] = xs
    xp = xp.permute(0, 2, 3, 1)                                  # [B, Hp, Wp, Cin]
    s = a = None
    k = 3 if taps == 9 else 1
    for ky in range(k):
        for kx in range(k):
            col = xp[:, ky:ky + H, kx:kx + W].reshape(B * H * W, Cin)
            wt = w[:, ky * k + kx]
            ds, da = col @ wt.t(), col.abs() @ wt.abs().t()
            s, a = (ds, da) if s is None else (s + ds, a + da)
    add = aadd = 0.0
    if bias is not None:
        add = bias.to(x.device, F64)[None, :]
        aadd = add.abs()
    r = (s + add) * float(out_scale)
    e = C_ACC * 2.0 ** -24 * (math.sqrt(taps * Cin) * a + aadd) * abs(float(out_scale))
    return r, e


def cs_chunk_check(y, part, groups, iters, label="", nonfinite=False):
    """Fused GroupNorm partial sums part [B, chunks, groups, 2] of conv_small8w's NHWC output y [B, H, W, N] against
    fp64 sums of the STORED y per (image, chunk, group).  Chunk c of an image is the c-th run of 16 * iters consecutive
    8-pixel groups in row-major order (one workgroup's pixels).  Tolerance as in gn_chunk_check: recursive fp32 summation
    of n terms in any order, n 2^-24 sum |y| (n + 1 for the squares).  Returns the worst err / tolerance ratio.
    nonfinite: see _nonfinite_slots."""
    B, H, W, N = y.shape
    per_img, per_blk = H * (W // 8), 16 * iters
    assert W % 8 == 0 and per_img % per_blk == 0 and N % groups == 0, (H, W, iters, N, groups)
    chunks, cpg = per_img // per_blk, N // groups
    assert tuple(part.shape) == (B, chunks, groups, 2), (tuple(part.shape), B, chunks, groups)
    # [B, chunks, per_blk * 8 pixels, groups, cpg] -> [B, chunks, groups, pixels x cpg]
    v = y.to(F64).reshape(B, chunks, per_blk * 8, groups, cpg).permute(0, 1, 3, 2, 4).reshape(B, chunks, groups, -1)
    n = v.shape[-1]
    s, q = v.sum(-1), (v * v).sum(-1)
    got = part.to(v.device, F64)
    tol_s = n * 2.0 ** -24 * v.abs().sum(-1) + 1e-30
    tol_q = (n + 1) * 2.0 ** -24 * q + 1e-30
    ratio = torch.maximum((got[..., 0] - s).abs() / tol_s, (got[..., 1] - q).abs() / tol_q)
    ratio = torch.where(torch.isfinite(got).all(-1), ratio, torch.full_like(ratio, math.inf))
    if nonfinite:
        ratio = _nonfinite_slots(ratio, s, q, got, label)
    worst = float(ratio.max())
    if not worst <= 1.0:
        b, c, g = [int(t) for t in torch.nonzero(ratio == ratio.max())[0]]
        g0 = c * per_blk
        raise AssertionError(f"{label}: fused GroupNorm sums off (worst ratio {worst:.3g}) at image {b}, chunk {c} "
                             f"(pixel groups {g0}..{g0 + per_blk - 1}), group {g}: got {got[b, c, g].tolist()}, "
                             f"fp64 {[float(s[b, c, g]), float(q[b, c, g])]}")
    return worst
