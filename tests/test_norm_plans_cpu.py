"""CPU tests (no GPU) of the norm / reduction checker (tests/norm_bound.py) and of the coverage of
tests/test_norm_plans_gpu.py.

numpy emulations of the kernels' fp32 summation order (gn_stats_kernel + gn_finalize_kernel, gn_bwd_*, ln_bwd_*,
colsum_*), driven by the geometry functions as the host code states them, must lie inside the new bounds: the fp64
references and the allowances alone are consistent.  The same emulations with one injected fault each pass the existing
global-L2 assertion (copied from test_ops_gpu.py / test_backward_gpu.py) and fail the per-element bound at the right place.
The Python restatement of the geometry is checked against the library's host-only queries for every GPU case, and the GPU
case tables are shown to reach every thread layout, pixel walk, fold path and kernel instantiation.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import norm_bound as nb
import test_norm_plans_gpu as G

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
f32 = np.float32


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def seq_sum(a, axis=0):
    """Sequential fp32 sum along `axis` (one accumulator, terms in index order)."""
    a = np.moveaxis(a, axis, 0)
    s = np.zeros(a.shape[1:], f32)
    for i in range(a.shape[0]):
        s = (s + a[i]).astype(f32)
    return s


def seq_fma_sq(a):
    """ss = fma(f, f, ss) along axis 0."""
    s = np.zeros(a.shape[1:], f32)
    for i in range(a.shape[0]):
        s = (a[i].astype(np.float64) * a[i] + s).astype(f32)
    return s


def butterfly(a):
    """wave_sum over the last axis (64 lanes, xor butterfly 32 .. 1) -> lane 0's value."""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = (a + a[..., idx ^ o]).astype(f32)
    return a[..., 0]


def chunked(x, chunks, ppc, slots):
    """[B, HW, C] -> [n1, B, chunks, slots, C]: slot s of a chunk walks pixels p0 + s, p0 + s + slots, ... (zero padded:
    adding 0.0 leaves an fp32 sum unchanged, so the padding stands for the pixels a slot does not have)."""
    B, HW, Cc = x.shape
    n1 = nb.cdiv(ppc, slots)
    v = np.zeros((B, chunks * ppc, Cc), x.dtype)
    v[:, :HW] = x
    v = v.reshape(B, chunks, ppc, Cc)
    w = np.zeros((B, chunks, n1 * slots, Cc), x.dtype)
    w[:, :, :ppc] = v
    return np.moveaxis(w.reshape(B, chunks, n1, slots, Cc), 2, 0)


# ------------------------------------------------------------------------------------------------ emulations

def emu_gn_stats(x, groups, eps, drop=None):
    """gn_stats_kernel + gn_finalize_kernel on fp32 values x [B, HW, C] -> (mean, rstd) fp32 [B, G, 2].
    drop = (image, group, chunk): that chunk partial is lost."""
    B, HW, Cc = x.shape
    chunks, ppc, threads, slots = nb.gn_geometry(B, HW, Cc)
    cpg = Cc // groups
    w = chunked(x, chunks, ppc, slots)
    s, ss = seq_sum(w), seq_fma_sq(w)                                         # [B, chunks, slots, C]: a thread's registers
    fold = lambda t: seq_sum(t.reshape(B, chunks, slots, groups, cpg).transpose(0, 1, 3, 2, 4).reshape(B, chunks, groups, slots * cpg), 3)
    ps, pq = fold(s), fold(ss)                                                # part[b][chunk][g]
    if drop is not None:
        ps[drop[0], drop[2], drop[1]] = 0.0
        pq[drop[0], drop[2], drop[1]] = 0.0
    n = float(HW * cpg)
    a, a2 = ps.astype(np.float64).sum(1), pq.astype(np.float64).sum(1)        # the fp64 fold
    mean = a / n
    var = np.maximum(a2 / n - mean * mean, 0.0)
    return np.stack([mean.astype(f32), (1.0 / np.sqrt(var + np.float64(f32(eps)))).astype(f32)], -1)


def emu_gn_apply(x, mr, gamma, beta, groups, out_dtype):
    cpg = x.shape[-1] // groups
    mean, rstd = np.repeat(mr[..., 0], cpg, 1)[:, None], np.repeat(mr[..., 1], cpg, 1)[:, None]
    rs = (rstd * gamma).astype(f32)
    rh = (beta - (mean * rs).astype(f32)).astype(f32)
    return T((x.astype(np.float64) * rs + rh).astype(f32)).to(out_dtype)


def emu_gn_bwd(x, dy, mr, gamma, beta, groups, out_dtype, drop_m2=None, drop_chunk=None):
    """gn_bwd_stats / fold / group_param / apply (no SiLU) -> dx, dgamma, dbeta.  drop_m2 = (image, group): the
    xhat * mean(gamma dz xhat) term is missing from that group's dx; drop_chunk = (image, channel): that image's last pixel
    chunk is missing from the channel's dgamma."""
    B, HW, Cc = x.shape
    chunks, ppc, threads, slots = nb.gnb_geometry(B, HW, Cc)
    cpg = Cc // groups
    mean, rstd = np.repeat(mr[..., 0], cpg, 1)[:, None], np.repeat(mr[..., 1], cpg, 1)[:, None]
    xh = ((x - mean).astype(f32) * rstd).astype(f32)
    dz = dy.astype(f32)
    t2 = (dz * xh).astype(f32)
    part = lambda t: seq_sum(seq_sum(chunked(t, chunks, ppc, slots)), 2)      # thread, then slots -> [B, chunks, C]
    p1, p2 = part(dz), part(t2)
    if drop_chunk is not None:
        p2 = p2.copy()
        p2_g = p2.copy()
        p2_g[drop_chunk[0], chunks - 1, drop_chunk[1]] = 0.0
    else:
        p2_g = p2

    def fold(p):                                                              # gn_bwd_fold_kernel: 4 lanes, then a tree
        q = np.zeros((B, nb.cdiv(chunks, 4) * 4, Cc), f32)
        q[:, :chunks] = p
        r = seq_sum(q.reshape(B, -1, 4, Cc), 1)
        return ((r[:, 0] + r[:, 1]).astype(f32) + (r[:, 2] + r[:, 3]).astype(f32)).astype(f32)

    s1, s2, s2g = fold(p1), fold(p2), fold(p2_g)
    dbeta, dgamma = seq_sum(s1), seq_sum(s2g)

    def gmean(s):                                                             # one wave per (image, group)
        w = (gamma * s).astype(f32).reshape(B, groups, cpg)
        lanes = np.zeros((B, groups, nb.cdiv(cpg, 64) * 64), f32)
        lanes[..., :cpg] = w
        a = butterfly(seq_sum(lanes.reshape(B, groups, -1, 64), 2))
        return np.repeat((a / f32(HW * cpg)).astype(f32), cpg, 1)[:, None]

    m1, m2 = gmean(s1), gmean(s2)
    if drop_m2 is not None:
        m2 = m2.copy()
        m2[drop_m2[0], 0, drop_m2[1] * cpg:(drop_m2[1] + 1) * cpg] = 0.0
    dx = (rstd * ((gamma * dz).astype(f32) - m1 - (xh * m2).astype(f32)).astype(f32)).astype(f32)
    return T(dx).to(out_dtype), T(dgamma), T(dbeta)


def emu_ln_bwd(x, dy, gamma, eps, out_dtype, skip=None):
    """ln_bwd_kernel + ln_bwd_fold_kernel -> dx, dgamma, dbeta.  skip = (block, column group): the fold misses that
    block's partial for the 16 channels of the column group."""
    rows, Cc = x.shape
    nbk, maxc = nb.lnb_blocks(rows), nb.ln_maxc(Cc)

    def wave(t):                                                              # lane l holds channel chunks l, l + 64, ...
        v = np.zeros((rows, maxc * 64 * 8), f32)
        v[:, :Cc] = t
        return butterfly(seq_sum(v.reshape(rows, maxc, 64, 8).transpose(1, 3, 0, 2).reshape(maxc * 8, rows, 64)))[:, None]

    mean = (wave(x) / f32(Cc)).astype(f32)
    dlt = (x - mean).astype(f32)
    rstd = (1.0 / np.sqrt((wave((dlt * dlt).astype(f32)) / f32(Cc)).astype(f32) + f32(eps))).astype(f32)
    xh = (dlt * rstd).astype(f32)
    gd = (gamma * dy).astype(f32)
    m1, m2 = (wave(gd) / f32(Cc)).astype(f32), (wave((gd * xh).astype(f32)) / f32(Cc)).astype(f32)
    dx = (rstd * ((gd - m1).astype(f32) - (xh * m2).astype(f32)).astype(f32)).astype(f32)
    rpw = nb.cdiv(rows, nbk * 4)

    def partials(t):                                                          # wave (block k, wave w): rows 4 k + w + 4 nb j
        v = np.zeros((rpw * nbk * 4, Cc), f32)
        v[:rows] = t
        return seq_sum(seq_sum(v.reshape(rpw, nbk, 4, Cc)), 1)                # [nb, C]

    def fold(p, which):
        if skip is not None and which == "dgamma":
            p = p.copy()
            p[skip[0], skip[1] * 16:(skip[1] + 1) * 16] = 0.0
        lanes = np.zeros((16, Cc), f32)
        for ln in range(16):
            a, k = np.zeros(Cc, f32), ln
            while k + 48 < nbk:
                a = (a + ((p[k] + p[k + 16]).astype(f32) + (p[k + 32] + p[k + 48]).astype(f32)).astype(f32)).astype(f32)
                k += 64
            while k < nbk:
                a = (a + p[k]).astype(f32)
                k += 16
            lanes[ln] = a
        return seq_sum(lanes)

    return T(dx).to(out_dtype), T(fold(partials((dy * xh).astype(f32)), "dgamma")), T(fold(partials(dy.astype(f32)), "dbeta"))


def emu_colsum(x, segs, scale=1.0, old=None, skip_last_chunk_of=None):
    """colsum_kernel + colsum_fold_kernel on fp32 values x [segs * rps, N] -> [segs, N]."""
    rows, N = x.shape
    rps = rows // segs
    chunks, rpc = nb.colsum_plan(rps)
    v = np.zeros((segs, chunks * rpc, N), f32)
    v[:, :rps] = x.reshape(segs, rps, N)
    part = seq_sum(seq_sum(v.reshape(segs, chunks, rpc // 8, 8, N), 2), 2)     # [segs, chunks, N]
    if skip_last_chunk_of is not None:
        part[skip_last_chunk_of, chunks - 1] = 0.0
    q = np.zeros((segs, nb.cdiv(chunks, 16) * 16, N), f32)
    q[:, :chunks] = part
    t = seq_sum(q.reshape(segs, -1, 16, N), 1)                                # [segs, 16, N]
    for w in (8, 4, 2, 1):
        t = (t[:, :w] + t[:, w:2 * w]).astype(f32)
    base = np.zeros((segs, N), np.float64) if old is None else old.astype(np.float64)
    return T((base + np.float64(f32(scale)) * t[:, 0]).astype(f32))


def data(shape, seed, dtype, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype)


def npf(t):
    return t.float().numpy()


# ------------------------------------------------------------------------------------------------ emulation within bound

@pytest.mark.parametrize("B,HW,Cc,dtype,offset", [
    (2, 1024, 320, BF16, 0.25), (2, 4096, 128, F32, 0.0), (2, 4096, 128, F32, 8.0), (2, 4096, 128, F32, 64.0),
    (2, 4096, 128, BF16, 64.0), (16, 700, 1280, F16, 0.25), (3, 64, 2560, F32, 8.0), (2, 100, 64, F16, 0.25), (1, 1000, 960, BF16, 8.0)])
def test_groupnorm_forward_emulation_lies_within_the_bound(B, HW, Cc, dtype, offset):
    x = data((B, HW, Cc), 1, dtype, 2.0, 2.0 * offset)
    gamma, beta = data((Cc,), 2, F32, 0.2, 1.0), data((Cc,), 3, F32, 0.2)
    mr = emu_gn_stats(npf(x), 32, 1e-5)
    r, e, mr_ref, e_mr = nb.gn_fwd_ref(x, gamma, beta, 32, 1e-5, False)
    ws = nb.check(T(mr), mr_ref, e_mr, F32, nb.Where("stats", groups=32), "emulated statistics")
    y = emu_gn_apply(npf(x), mr, gamma.numpy(), beta.numpy(), 32, BF16)
    wy = nb.check(y, r, e, BF16, nb.Where("gn", HW=HW, C=Cc, groups=32, ppc=nb.gn_geometry(B, HW, Cc)[1]), "emulated groupnorm")
    rel_rstd = float(((T(mr)[..., 1].double() - mr_ref[..., 1]).abs() / mr_ref[..., 1]).max())
    print(f"emulated GroupNorm B={B} HW={HW} C={Cc} |mean|/std={offset:g}: rstd rel err {rel_rstd:.2e}, ratios {ws:.3f} / {wy:.3f}")
    assert ws < 1.0 and wy < 1.0


@pytest.mark.parametrize("B,HW,Cc,dtype", [(2, 1024, 320, BF16), (3, 100, 320, F16), (16, 700, 1280, BF16), (2, 4, 1280, F16),
                                           (2, 4096, 128, BF16)])
def test_groupnorm_backward_emulation_lies_within_the_bound(B, HW, Cc, dtype):
    x, dy = data((B, HW, Cc), 1, dtype, 1.0, 0.5), data((B, HW, Cc), 2, dtype)
    gamma, beta = data((Cc,), 3, F32, 0.5, 1.0), data((Cc,), 4, F32, 0.2)
    mr = emu_gn_stats(npf(x), 32, 1e-5)
    dx, dg, db = emu_gn_bwd(npf(x), npf(dy), mr, gamma.numpy(), beta.numpy(), 32, dtype)
    ref = nb.gn_bwd_ref(x, dy, T(mr), gamma, beta, 32, False)
    assert nb.check(dx, *ref["dx"], dtype, label="dx") < 1.0
    assert nb.check(dg, *ref["dgamma"], F32, label="dgamma") < 1.0 and nb.check(db, *ref["dbeta"], F32, label="dbeta") < 1.0


@pytest.mark.parametrize("rows,Cc,dtype", [(4096, 320, BF16), (777, 640, F16), (64, 1280, BF16), (5, 64, F16), (3, 2048, BF16),
                                           (1025, 1032, F16)])
def test_layernorm_backward_emulation_lies_within_the_bound(rows, Cc, dtype):
    x, dy = data((rows, Cc), 1, dtype, 3.0, 1.0), data((rows, Cc), 2, dtype)
    gamma = data((Cc,), 3, F32, 0.5, 1.0)
    dx, dg, db = emu_ln_bwd(npf(x), npf(dy), gamma.numpy(), 1e-5, dtype)
    ref = nb.ln_bwd_ref(x, dy, gamma, 1e-5)
    assert nb.check(dx, *ref["dx"], dtype, label="dx") < 1.0
    assert nb.check(dg, *ref["dgamma"], F32, label="dgamma") < 1.0 and nb.check(db, *ref["dbeta"], F32, label="dbeta") < 1.0
    # the forward of the same rows, correctly rounded from the fp64 reference, is accepted too
    r, e = nb.ln_fwd_ref(x, gamma, gamma * 0.1, 1e-5)
    assert nb.check(r.to(dtype), r, e, dtype) < 1.0


@pytest.mark.parametrize("rps,segs,N,dtype", [(3000, 1, 640, BF16), (1000, 3, 640, F16), (65536, 1, 16, BF16), (7, 5, 1000, F16),
                                              (65409, 2, 8, BF16), (1, 1, 8, F16)])
def test_colsum_emulation_lies_within_the_bound(rps, segs, N, dtype):
    x, old = data((rps * segs, N), 1, dtype, 1.0, 0.25), data((segs, N), 2, F32)
    assert nb.check(emu_colsum(npf(x), segs), *nb.colsum_ref(x, segs), F32, label="colsum") < 1.0
    assert nb.check(emu_colsum(npf(x), segs, 0.25, old.numpy()), *nb.colsum_ref(x, segs, 0.25, old), F32, label="colsum +=") < 1.0


def test_pointwise_references_accept_correctly_rounded_results():
    for dtype in (BF16, F16):
        pre, dout = data((40, 128), 1, dtype, 1.5), data((40, 64), 2, dtype)
        for r, e in (nb.geglu_fwd_ref(pre), nb.geglu_bwd_ref(pre, dout), nb.add_ref(pre, pre), nb.silu_ref(pre), nb.silu_ref(pre, pre),
                     nb.softmax_rows_ref(data((9, 100), 3, F32, 4.0), 0.3), nb.softmax_groups_ref(data((9, 64), 3, F32, 3.0), 5, 4),
                     nb.pool2x2_ref(data((2, 4, 6, 8), 4, dtype))):
            assert nb.check(r.to(dtype), r, e, dtype) <= 1.0
    # GEGLU backward against autograd in fp64 (the packed layout included)
    pre = data((7, 128), 5, torch.float64).requires_grad_()
    a, g = nb.geglu_unpack(pre)
    (a * 0.5 * g * (1 + torch.erf(g / 2 ** 0.5))).backward(torch.ones(7, 64, dtype=torch.float64))
    r, _ = nb.geglu_bwd_ref(pre.detach(), torch.ones(7, 64, dtype=torch.float64))
    assert torch.allclose(r, pre.grad, rtol=0, atol=1e-12)
    # one AdamW step against torch.optim.AdamW in fp64
    p, gr = data((1000,), 6, F32), data((1000,), 7, F32)
    tp = torch.nn.Parameter(p.double())
    opt = torch.optim.AdamW([tp], lr=float(torch.tensor(3e-4)), betas=(float(torch.tensor(0.9)), float(torch.tensor(0.999))),
                            weight_decay=float(torch.tensor(1e-2)), eps=float(torch.tensor(1e-8)))
    tp.grad = gr.double()
    opt.step()
    ref = nb.adamw_ref(p, gr, torch.zeros(1000), torch.zeros(1000), 1, 3e-4, 0.9, 0.999, 1e-8, 1e-2)
    assert torch.allclose(ref["p"][0], tp.detach(), rtol=0, atol=1e-12)
    assert nb.check(ref["p"][0].float(), *ref["p"], F32) <= 1.0


# ------------------------------------------------------------------------------------------------ injected faults

def test_groupnorm_forward_dropped_chunk_partial_passes_global_l2_and_fails_the_bound():
    """One of the 43 chunk partials of (image 1, group 7) is lost (B=2, HW=1024, C=320, bf16, offset 0.5)."""
    from test_ops_gpu import TOL, rel
    import torch.nn.functional as F
    B, HW, Cc, dtype = 2, 1024, 320, BF16
    x = data((B, HW, Cc), 1, dtype) * 2 + 0.5
    g, b = torch.randn(Cc) * 0.2 + 1, torch.randn(Cc) * 0.2
    r, e, mr_ref, e_mr = nb.gn_fwd_ref(x, g, b, 32, 1e-5, False)
    wh = nb.Where("gn", HW=HW, C=Cc, groups=32, ppc=nb.gn_geometry(B, HW, Cc)[1])
    good = emu_gn_apply(npf(x), emu_gn_stats(npf(x), 32, 1e-5), g.numpy(), b.numpy(), 32, dtype)
    assert nb.check(good, r, e, dtype, wh) < 1.0
    mr_bad = emu_gn_stats(npf(x), 32, 1e-5, drop=(1, 7, 20))
    y = emu_gn_apply(npf(x), mr_bad, g.numpy(), b.numpy(), 32, dtype)
    ref = F.group_norm(x.float().transpose(1, 2), 32, g, b, eps=1e-5).transpose(1, 2)
    assert rel(y, ref) < TOL[dtype]                                  # the gap: test_groupnorm's assertion passes
    with pytest.raises(AssertionError, match=r"image 1, group 7, channel 7\d"):
        nb.check(y, r, e, dtype, wh, "dropped chunk partial")
    with pytest.raises(AssertionError, match=r"image 1, group 7, (mean|rstd)"):
        nb.check(T(mr_bad), mr_ref, e_mr, F32, nb.Where("stats", groups=32), "dropped chunk partial")


def _gn_bwd_case(B, HW, Cc, dtype, G_=32):
    import torch.nn.functional as F
    x, dy = data((B, HW, Cc), 1, dtype) + 0.5, data((B, HW, Cc), 2, dtype)
    gamma, beta = torch.randn(Cc) * 0.5 + 1.0, torch.randn(Cc) * 0.2
    xr, gr, br = x.float().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    z = F.group_norm(xr.transpose(1, 2), G_, gr, br, 1e-5).transpose(1, 2)
    z.backward(dy.float())
    mr = emu_gn_stats(npf(x), G_, 1e-5)
    return x, dy, gamma, beta, xr, gr, br, mr


def test_groupnorm_backward_dropped_group_term_passes_global_l2_and_fails_the_bound():
    """dx of (image 2, group 5) misses xhat * mean(gamma dz xhat)."""
    from test_backward_gpu import TOL, rel
    B, HW, Cc, dtype = 3, 256, 1280, BF16
    x, dy, gamma, beta, xr, gr, br, mr = _gn_bwd_case(B, HW, Cc, dtype)
    ref = nb.gn_bwd_ref(x, dy, T(mr), gamma, beta, 32, False)
    wh = nb.Where("gn", HW=HW, C=Cc, groups=32, ppc=nb.gnb_geometry(B, HW, Cc)[1])
    good, _, _ = emu_gn_bwd(npf(x), npf(dy), mr, gamma.numpy(), beta.numpy(), 32, dtype)
    assert nb.check(good, *ref["dx"], dtype, wh) < 1.0
    dx, _, _ = emu_gn_bwd(npf(x), npf(dy), mr, gamma.numpy(), beta.numpy(), 32, dtype, drop_m2=(2, 5))
    assert rel(dx, xr.grad) < 2 * TOL[dtype]                         # test_groupnorm_backward's assertion passes
    with pytest.raises(AssertionError, match=r"image 2, group 5, channel 2\d\d"):
        nb.check(dx, *ref["dx"], dtype, wh, "dropped group term")


def test_groupnorm_backward_missing_last_chunk_of_one_channel_passes_global_l2_and_fails_the_bound():
    """dgamma[77] misses image 1's last pixel chunk (4 of the channel's 3 x 1024 pixels)."""
    from test_backward_gpu import rel
    B, HW, Cc, dtype = 3, 1024, 1280, BF16
    x, dy, gamma, beta, xr, gr, br, mr = _gn_bwd_case(B, HW, Cc, dtype)
    ref = nb.gn_bwd_ref(x, dy, T(mr), gamma, beta, 32, False)
    _, good, _ = emu_gn_bwd(npf(x), npf(dy), mr, gamma.numpy(), beta.numpy(), 32, dtype)
    assert nb.check(good, *ref["dgamma"], F32, nb.Where("cols", N=Cc)) < 1.0
    _, dg, db = emu_gn_bwd(npf(x), npf(dy), mr, gamma.numpy(), beta.numpy(), 32, dtype, drop_chunk=(1, 77))
    assert rel(dg, gr.grad) < 2e-3 and rel(db, br.grad) < 2e-3       # test_groupnorm_backward's assertion passes
    with pytest.raises(AssertionError, match=r"segment 0, channel 77 "):
        nb.check(dg, *ref["dgamma"], F32, nb.Where("cols", N=Cc), "dgamma without one chunk")


def test_layernorm_backward_skipped_block_partial_passes_global_l2_and_fails_the_bound():
    """The fold skips block 255's partial for the 16 channels of column group 9.  rows = 1021: 256 blocks, the last one
    holds the single row 1020, whose gradient is small (2^-6 of the others): 16 of 2048 channels lose one small term."""
    from test_backward_gpu import rel
    import torch.nn.functional as F
    rows, Cc, dtype = 1021, 2048, BF16
    assert nb.lnb_blocks(rows) == 256 and rows - 255 * 4 == 1
    x, dy = data((rows, Cc), 1, dtype) + 0.3, data((rows, Cc), 2, dtype)
    dy[1020] *= 2.0 ** -6
    gamma, beta = torch.randn(Cc) * 0.5 + 1.0, torch.randn(Cc) * 0.2
    xr, gr, br = x.float().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    F.layer_norm(xr, (Cc,), gr, br, 1e-5).backward(dy.float())
    ref = nb.ln_bwd_ref(x, dy, gamma, 1e-5)
    _, good, _ = emu_ln_bwd(npf(x), npf(dy), gamma.numpy(), 1e-5, dtype)
    assert nb.check(good, *ref["dgamma"], F32, nb.Where("cols", N=Cc)) < 1.0
    _, dg, db = emu_ln_bwd(npf(x), npf(dy), gamma.numpy(), 1e-5, dtype, skip=(255, 9))
    assert rel(dg, gr.grad) < 1e-4 and rel(db, br.grad) < 1e-4       # test_layernorm_backward's assertion passes
    with pytest.raises(AssertionError, match=r"channel 1[45]\d \(column group 9\)"):
        nb.check(dg, *ref["dgamma"], F32, nb.Where("cols", N=Cc), "skipped block partial")


def test_colsum_skipped_last_chunk_passes_global_l2_and_fails_the_bound():
    """65409 rows per segment: 1023 chunks (1023 % 16 = 15), the last one a single row; segment 1 loses it."""
    from test_backward_gpu import rel
    rps, segs, N = 65409, 2, 8
    chunks, rpc = nb.colsum_plan(rps)
    assert chunks == 1023 and chunks % 16 != 0 and rps - (chunks - 1) * rpc == 1
    dy = data((rps * segs, N), 1, BF16, 0.1, 1.0)
    r, e = nb.colsum_ref(dy, segs)
    wh = nb.Where("cols", N=N)
    assert nb.check(emu_colsum(npf(dy), segs), r, e, F32, wh) < 1.0
    per_img = emu_colsum(npf(dy), segs, skip_last_chunk_of=1)
    assert rel(per_img, dy.float().view(segs, rps, N).sum(1)) < 2e-5     # test_linear_dgrad_and_colsum's assertion passes
    with pytest.raises(AssertionError, match=r"segment 1, channel \d"):
        nb.check(per_img, r, e, F32, wh, "skipped chunk")


def test_softmax_rows_maximum_over_the_first_1024_columns_passes_global_l2_and_fails_the_bound():
    """softmax_rows_reg_kernel with the row maximum taken over its first 256 x 4 columns only: row 11, flat over columns
    1024 .. 4095 and far below them on the left, overflows its sum and comes out as zeros."""
    from test_ops_gpu import TOL, rel
    rows, Lr, dtype = 100, 4096, BF16
    s = torch.randn(rows, Lr, generator=torch.Generator().manual_seed(1)) * 40       # peaked rows: a few large probabilities each
    s[11, :1024], s[11, 1024:] = -200.0, 93.0
    c = np.float32(0.3) * np.float32(1.4426950408889634)

    def kernel(m):
        p = torch.exp2((s - m) * float(c))                           # fp32, as the kernel
        return (p * (1.0 / p.sum(1, keepdim=True))).to(dtype)

    r, e = nb.softmax_rows_ref(s, 0.3)
    wh = nb.Where("rows", C=Lr)
    assert nb.check(kernel(s.max(1, keepdim=True).values), r, e, dtype, wh) < 1.0
    y = kernel(s[:, :1024].max(1, keepdim=True).values)
    assert bool(torch.isfinite(y.float()).all())
    assert rel(y, torch.softmax(s * 0.3, -1)) < TOL[dtype]          # test_softmax_transpose_concat_bmm's assertion passes
    with pytest.raises(AssertionError, match=r"row 11, channel \d+"):
        nb.check(y, r, e, dtype, wh, "partial row maximum")


# ------------------------------------------------------------------------------------------------ geometry against the library

def test_geometry_restatement_matches_the_library_for_every_gpu_case(hip_lib):
    from diffews_amd import _lib as L
    lib = L.lib()
    for c in G.GN_CASES:
        for pad in {0, c.pad}:
            a = L.GroupNormArgs()
            a.B, a.HW, a.C, a.groups, a.ldx, a.ldy, a.dtype = c.B, c.HW, c.C, c.groups, c.C + pad, c.C + pad + (8 if pad else 0), L.BF16
            chunks = nb.gn_geometry(c.B, c.HW, c.C)[0]
            nbytes = lib.dfw_groupnorm_workspace_bytes(C.byref(a))
            assert nbytes == (c.B * chunks * c.groups * 2 + c.B * c.groups * 2) * 4, c.id
            assert (nbytes // 4 - c.B * c.groups * 2) // (c.B * c.groups * 2) == chunks
            b = L.GroupNormBwdArgs()
            b.B, b.HW, b.C, b.groups, b.ldx, b.lddy, b.lddx, b.dtype = c.B, c.HW, c.C, c.groups, c.C + pad, c.C + pad, c.C + pad, L.BF16
            bchunks = nb.gnb_geometry(c.B, c.HW, c.C)[0]
            assert lib.dfw_groupnorm_bwd_workspace_bytes(C.byref(b)) == (c.B * bchunks * c.C * 2 + c.B * c.groups * 2) * 4, c.id
    for rows, Cc, pad, xf32 in G.LN_CASES:
        assert lib.dfw_layernorm_bwd_workspace_bytes(rows, Cc) == nb.lnb_blocks(rows) * Cc * 2 * 4
    ch, rp = C.c_int32(0), C.c_int32(0)
    for rps, segs, N in G.COLSUM_CASES + [(r, 1, 8) for r in range(1, 300)] + [(65535, 1, 8), (65537, 1, 8), (200000, 1, 8)]:
        L.check(lib.dfw_colsum_plan(rps, C.byref(ch), C.byref(rp)), "dfw_colsum_plan")
        assert (ch.value, rp.value) == nb.colsum_plan(rps), rps
        assert lib.dfw_colsum_workspace_bytes(rps, segs, N) == segs * ch.value * N * 4


# ------------------------------------------------------------------------------------------------ coverage of the GPU cases

def _walk(B, HW, Cc, geometry):
    """Per case: (chunks, ppc, slots, tpp, per-slot pixel counts of a full chunk, pixels of the last chunk)."""
    chunks, ppc, threads, slots = geometry(B, HW, Cc)
    full = min(ppc, HW)
    counts = {len(range(s, full, slots)) for s in range(slots)}
    return chunks, ppc, slots, Cc // 8, counts, HW - (chunks - 1) * ppc


def test_gpu_cases_reach_every_layout_walk_and_instantiation():
    gn = [(c, _walk(c.B, c.HW, c.C, nb.gn_geometry)) for c in G.GN_CASES]
    has = lambda pred: any(pred(c, w) for c, w in gn)
    # thread layouts
    assert has(lambda c, w: w[2] == 1 and w[3] > 256 and c.C == 2560)
    for Cc in (320, 960, 1920):
        assert has(lambda c, w: c.C == Cc and 256 % w[3] != 0)
    cpgs = {c.C // c.groups for c, _ in gn}
    assert any(v < 8 for v in cpgs) and any(v % 8 == 0 for v in cpgs) and {10, 30} <= cpgs
    # pixel walks: unrolled loop (four or more pixels per slot) with a tail (count % 4 != 0); short last chunk; lanes loop; one chunk
    assert has(lambda c, w: any(n >= 4 and n % 4 for n in w[4]))
    assert has(lambda c, w: w[0] > 1 and w[5] < w[1])
    assert has(lambda c, w: w[0] > 64) and has(lambda c, w: w[0] == 1)
    # the same for the backward geometry (16-bit cases only)
    gb = [_walk(c.B, c.HW, c.C, nb.gnb_geometry) for c in G.GN_CASES if not c.xf32]
    assert any(w[0] > 1 and w[5] < w[1] for w in gb) and any(w[0] == 1 for w in gb) and any(w[0] % 4 for w in gb)
    # the real shapes, the offsets, the ABI corners
    shapes = {(c.HW, c.C) for c, _ in gn}
    assert {(262144, 128), (65536, 256), (16384, 512)} <= shapes
    assert {c.C for c, _ in gn} >= {320, 640, 960, 1280, 1920, 2560} and {c.HW for c, _ in gn} >= {4096, 1024, 256, 64}
    assert max(c.B for c, _ in gn) >= 16
    for xf32 in (False, True):
        assert {0.0, 8.0, 64.0} <= {c.offset for c, _ in gn if c.xf32 == xf32}
        assert has(lambda c, w: c.xf32 == xf32 and c.outlier) and has(lambda c, w: c.xf32 == xf32 and not c.affine)
        assert has(lambda c, w: c.xf32 == xf32 and c.pad) and {True, False} <= {c.silu for c, _ in gn if c.xf32 == xf32}
    assert {"plain", "full", "null"} <= {c.bwd for c, _ in gn if not c.xf32}
    # LayerNorm: every MAXC of ln_kernel (16-bit and fp32 input) and of ln_bwd_kernel; fold paths
    assert {nb.ln_maxc(Cc) for r, Cc, p, f in G.LN_CASES if not f} == {1, 2, 4}
    assert {nb.ln_maxc(Cc) for r, Cc, p, f in G.LN_CASES if f} == {1, 2, 4}
    assert {Cc for r, Cc, p, f in G.LN_CASES} >= {64, 320, 512, 520, 640, 1024, 1032, 1280, 2048}
    assert {r for r, Cc, p, f in G.LN_CASES} >= {1, 3, 5, 1023, 1025, 4096, 70000}
    blocks = {nb.lnb_blocks(r) for r, Cc, p, f in G.LN_CASES if not f}
    assert 256 in blocks and any(b > 64 and b % 64 for b in blocks) and any(b < 16 for b in blocks)
    assert any(r > 1024 for r, Cc, p, f in G.LN_CASES if not f)                   # rows strided over the grid
    assert any(r < 4 for r, Cc, p, f in G.LN_CASES) and any(p for r, Cc, p, f in G.LN_CASES)
    # column sums
    plans = [(nb.colsum_plan(rps)[0], segs, N) for rps, segs, N in G.COLSUM_CASES]
    assert any(ch == 1024 for ch, s, N in plans) and any(ch > 16 and ch % 16 for ch, s, N in plans)
    assert any(N % 256 for ch, s, N in plans) and any(N % 16 == 8 for ch, s, N in plans) and any(s > 1 for ch, s, N in plans)
    assert len(G.COLSUM_CASES) * len(G.COLSUM_VARIANTS) >= 50
    # both softmax kernels
    reg = {Lr <= 4096 and Lr % 4 == 0 for Lr in G.SOFTMAX_L}
    assert reg == {True, False} and {4, 1020, 1024, 4096, 4100, 4098, 16384} <= set(G.SOFTMAX_L)
    assert any(g * l < ld for r, ld, g, l in G.SOFTMAX_GROUPS) and any(g * l == ld for r, ld, g, l in G.SOFTMAX_GROUPS)
    rows, H = G.GEGLU_CASES[0]
    assert rows * H // 8 > 4096 * 256
