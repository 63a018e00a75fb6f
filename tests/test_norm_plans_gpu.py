"""Geometry matrix of the norm, reduction and pointwise kernels in both storage dtypes, checked element by element.

Every output element of GroupNorm (statistics, apply, backward), LayerNorm (forward, backward), the column sums (single
call and ColsumQueue), both row-softmax kernels, softmax_groups, GEGLU, the element-wise modes, the loss kernels, sumsq and
AdamW is compared with an fp64 reference within the bound of tests/norm_bound.py; `-s` prints the worst err / bound ratio
of every case (lines starting with NORMRATIO).  tests/test_norm_plans_cpu.py imports the case tables below and proves,
without a GPU, that they reach every thread layout, pixel walk, fold path and kernel instantiation listed there.

Shapes: the VAE's GroupNorms (C=128 at HW=262144, C=256 at 65536, C=512 at 16384), the UNet's (C in 320 .. 2560 at HW in
4096 .. 64, B up to 16), chunks == 1, chunks > 64, a short last chunk, an unrolled pixel loop with a tail, cpg < 8 / 8k /
10 / 30, |mean| / std in {0, 8, 64} for 16-bit and fp32 input, an outlier channel, NULL gamma / beta, NULL dgamma / dbeta,
ldx / ldy / lddy / lddx wider than C (columns outside the view must stay untouched), statistics fused into the producing
conv; LayerNorm C in {64 .. 2048} x rows in {1 .. 70000} with strided rows; column sums at the chunk cap, chunks % 16 != 0,
N % 256 != 0, N % 16 == 8, segs > 1; softmax L in {4 .. 16384}.
"""
import ctypes as C
from dataclasses import dataclass

import pytest
import torch

import norm_bound as nb

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
TNAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
F32 = torch.float32
SENTINEL = 3.0
EPS = 1e-5


# ------------------------------------------------------------------------------------------------ case tables

@dataclass
class Gn:
    id: str
    B: int
    HW: int
    C: int
    groups: int = 32
    silu: bool = True
    xf32: bool = False        # fp32 residual stream in (forward only: the backward reads 16-bit x)
    offset: float = 0.0       # |mean| / std of every group
    outlier: bool = False     # one channel of image 0, group 3 is 50x larger
    affine: bool = True       # False: gamma == beta == NULL
    pad: int = 0              # > 0: x, y, dy, dx are column views of buffers pad (x, dy) and pad + 8 (y, dx) columns wider
    bwd: str = "full"         # 'plain': fresh dgamma / dbeta; 'full': dx_add, accumulate, grad_scale 0.5; 'null': no dgamma


GN_CASES = [
    # the VAE's: C=128 at 512 x 512, C=256 at 256 x 256, C=512 at 128 x 128
    Gn("vae128", 1, 262144, 128), Gn("vae256", 1, 65536, 256), Gn("vae512", 1, 16384, 512),
    # the UNet's
    Gn("u320_4096_b16", 16, 4096, 320), Gn("u640_4096", 2, 4096, 640), Gn("u960_4096", 2, 4096, 960),
    Gn("u320_1024", 2, 1024, 320, bwd="plain"), Gn("u640_1024", 4, 1024, 640), Gn("u960_1024", 3, 1024, 960, silu=False),
    Gn("u1920_1024", 2, 1024, 1920), Gn("u1280_256", 8, 256, 1280), Gn("u1920_256", 2, 256, 1920, bwd="plain"),
    Gn("u2560_256", 2, 256, 2560), Gn("u1280_64_b16", 16, 64, 1280), Gn("u2560_64", 5, 64, 2560, silu=False),
    Gn("u640_256", 2, 256, 640, bwd="null"), Gn("u320_64", 3, 64, 320, bwd="plain"),
    Gn("u1280_4096", 2, 4096, 1280), Gn("u1920_4096", 1, 4096, 1920, bwd="plain"), Gn("u2560_4096", 1, 4096, 2560, silu=False),
    Gn("u1280_1024", 7, 1024, 1280, bwd="plain"), Gn("u2560_1024", 3, 1024, 2560), Gn("u320_256", 16, 256, 320),
    Gn("u960_256", 4, 256, 960, bwd="plain"), Gn("u640_64", 7, 64, 640), Gn("u960_64", 16, 64, 960, silu=False),
    Gn("u1920_64", 3, 64, 1920, bwd="plain"),
    # pixel walks: unrolled loop + tail with a short last chunk (ppc 6, slots 1); one chunk; ragged single chunk
    Gn("walk_tail", 16, 700, 1280), Gn("one_chunk", 2, 4, 1280, bwd="plain"), Gn("one_chunk_ragged", 2, 100, 64),
    Gn("ragged_320", 1, 1000, 320, silu=False, bwd="plain"), Gn("tiny_1920", 1, 16, 1920),
    # channels per group below 8 (64 / 32 = 2), wave-sized groups
    Gn("cpg2", 2, 256, 64, bwd="plain"), Gn("groups8", 2, 300, 512, groups=8),
    # offsets and the outlier, 16-bit and fp32 input
    Gn("off0", 2, 4096, 128, bwd="plain"), Gn("off8", 2, 4096, 128, offset=8.0), Gn("off64", 2, 4096, 128, offset=64.0),
    Gn("outlier", 2, 1024, 320, outlier=True),
    Gn("f32_off0", 2, 4096, 128, xf32=True), Gn("f32_off8", 2, 4096, 128, xf32=True, offset=8.0),
    Gn("f32_off64", 2, 4096, 128, xf32=True, offset=64.0), Gn("f32_outlier", 2, 1024, 320, xf32=True, outlier=True),
    Gn("f32_2560", 3, 64, 2560, xf32=True, silu=False), Gn("f32_960", 1, 1000, 960, xf32=True),
    # NULL affine, strided views
    Gn("null_affine", 2, 256, 640, affine=False, bwd="plain"), Gn("null_affine_f32", 2, 100, 320, affine=False, xf32=True, silu=False),
    Gn("strided_320", 2, 1000, 320, pad=8), Gn("strided_128", 3, 4096, 128, pad=64, silu=False),
    Gn("strided_f32", 2, 256, 1280, pad=16, xf32=True),
]

# LayerNorm: (rows, C, row padding, fp32 input)
LN_CASES = [(1, 64, 0, False), (3, 320, 0, False), (5, 512, 0, False), (1023, 520, 0, False), (1025, 640, 0, False),
            (4096, 1024, 0, False), (70000, 320, 0, False), (1025, 1032, 0, False), (4096, 1280, 0, False),
            (1023, 2048, 0, False), (70000, 640, 0, False), (3, 2048, 0, False), (777, 1280, 0, False), (500, 64, 0, False),
            (5, 1024, 0, False), (1, 1280, 0, False), (300, 320, 8, False), (1025, 1024, 16, False), (100, 2048, 8, False),
            (257, 64, 0, True), (1000, 320, 0, True), (300, 1024, 0, True), (64, 1280, 0, True), (3, 2048, 8, True)]

# column sums: (rows per segment, segs, N)
COLSUM_CASES = [(3000, 1, 640), (1000, 3, 640), (65536, 1, 16), (65409, 2, 8), (32768, 1, 320), (4096, 16, 1280),
                (100, 1, 24), (7, 5, 1000), (1, 1, 8), (64, 2, 264), (777, 2, 1032)]
# how each case enters the ColsumQueue flush: (x column padding, out column padding, scale, accumulate)
COLSUM_VARIANTS = [(0, 0, 1.0, False), (0, 0, 0.25, True), (8, 0, 1.0, False), (0, 8, -2.0, False), (16, 24, 0.5, True)]

SOFTMAX_L = [4, 1020, 1024, 4096, 4100, 4098, 16384, 264]
# softmax_groups: (rows, ld, groups, L)
SOFTMAX_GROUPS = [(1000, 64, 5, 2), (64, 64, 20, 2), (300, 64, 10, 4), (7, 64, 1, 64), (33, 128, 3, 8)]

# GEGLU (rows, H): the first has rows * H / 8 above grid_for's cap of 4096 x 256 threads
GEGLU_CASES = [(4100, 2560), (500, 256), (3, 32)]


# ------------------------------------------------------------------------------------------------ helpers

@pytest.fixture(scope="module")
def env(hip_lib):
    from diffews_amd import ops, ops_bwd, _lib
    return ops, ops_bwd, _lib


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(shape, g, dtype=F32, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g, device="cuda") * scale + shift).to(dtype)


def report(kernel, dtype, case, ratio):
    print(f"NORMRATIO {kernel} {TNAME.get(dtype, 'f32')} {case} {ratio:.4f}")
    return ratio


def wide(shape, width, g, dtype, fill=None):
    """[..., C] view of a [..., width] buffer (random or constant fill) -> (buffer, view)."""
    Cc = shape[-1]
    buf = randn((*shape[:-1], width), g, dtype) if fill is None else torch.full((*shape[:-1], width), fill, dtype=dtype, device="cuda")
    return buf, buf[..., :Cc]


def gn_input(c, dtype, g):
    x = randn((c.B, c.HW, c.C), g, F32, 2.0, 2.0 * c.offset if c.offset else 0.5)
    if c.outlier:
        cpg = c.C // c.groups
        x[0, :, 3 * cpg + 1] *= 50.0
    return x if c.xf32 else x.to(dtype)


def gn_forward(L, x, y, gamma, beta, groups, eps, silu, pre=None):
    """dfw_groupnorm on [B, HW, C] views x (16-bit or fp32) and y (row strides = ldx, ldy) -> the (mean, rstd) buffer."""
    B, HW, Cc = x.shape
    a = L.GroupNormArgs()
    a.x, a.y = x.data_ptr(), y.data_ptr()
    a.gamma, a.beta = (gamma.data_ptr() if gamma is not None else None), (beta.data_ptr() if beta is not None else None)
    a.B, a.HW, a.C, a.groups, a.ldx, a.ldy = B, HW, Cc, groups, x.stride(1), y.stride(1)
    a.eps, a.silu, a.dtype, a.x_f32 = eps, int(silu), (L.BF16 if y.dtype == torch.bfloat16 else L.F16), int(x.dtype == F32)
    if pre is not None:
        a.pre_partial, a.pre_chunks = pre[0].data_ptr(), pre[1]
    lib = L.lib()
    nbytes = lib.dfw_groupnorm_workspace_bytes(C.byref(a))
    assert nbytes > 0
    ws = torch.empty(nbytes // 4, dtype=F32, device="cuda")
    a.stats_ws, a.stats_ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.dfw_groupnorm(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dfw_groupnorm")
    return ws[ws.numel() - B * groups * 2:].view(B, groups, 2)


def gn_backward(L, x, dy, dx, mr, gamma, beta, groups, silu, dgamma, dbeta, accumulate, grad_scale, dx_add):
    B, HW, Cc = x.shape
    a = L.GroupNormBwdArgs()
    a.x, a.dy, a.dx, a.mean_rstd = x.data_ptr(), dy.data_ptr(), dx.data_ptr(), mr.data_ptr()
    for k, t in (("gamma", gamma), ("beta", beta), ("dgamma", dgamma), ("dbeta", dbeta), ("dx_add", dx_add)):
        setattr(a, k, t.data_ptr() if t is not None else None)
    a.B, a.HW, a.C, a.groups, a.ldx, a.lddy, a.lddx = B, HW, Cc, groups, x.stride(1), dy.stride(1), dx.stride(1)
    a.silu, a.accumulate, a.grad_scale = int(silu), int(accumulate), grad_scale
    a.dtype = L.BF16 if x.dtype == torch.bfloat16 else L.F16
    lib = L.lib()
    nbytes = lib.dfw_groupnorm_bwd_workspace_bytes(C.byref(a))
    assert nbytes > 0
    ws = torch.empty(nbytes // 4, dtype=F32, device="cuda")
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    L.check(lib.dfw_groupnorm_bwd(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dfw_groupnorm_bwd")


def rstd_rel_error(mr, ref):
    return float(((mr[..., 1].double() - ref[..., 1]).abs() / ref[..., 1]).max())


# ------------------------------------------------------------------------------------------------ GroupNorm

@pytest.mark.parametrize("dtype", DTYPES, ids=list(TNAME.values()))
@pytest.mark.parametrize("c", GN_CASES, ids=lambda c: c.id)
def test_groupnorm_forward_and_backward(env, c, dtype):
    ops, ob, L = env
    g = gen(len(c.id) * 1000 + c.C + c.HW)
    x = gn_input(c, dtype, g)
    gamma = randn((c.C,), g, F32, 0.2, 1.0) if c.affine else None
    beta = randn((c.C,), g, F32, 0.2) if c.affine else None
    if c.pad:
        xb, xv = wide((c.B, c.HW, c.C), c.C + c.pad, g, x.dtype)
        xv.copy_(x)
        yb, y = wide((c.B, c.HW, c.C), c.C + c.pad + 8, g, dtype, fill=SENTINEL)
        mr = gn_forward(L, xv, y, gamma, beta, c.groups, EPS, c.silu)
        assert bool((yb[..., c.C:] == SENTINEL).all()), "groupnorm wrote outside its ldy view"
        x = xv
    else:
        y, mr = ops.groupnorm(x, gamma, beta, c.groups, EPS, silu=c.silu, return_stats=True, out_dtype=dtype if c.xf32 else None)
    r, e, mr_ref, e_mr = nb.gn_fwd_ref(x, gamma, beta, c.groups, EPS, c.silu)
    chunks, ppc, _, _ = nb.gn_geometry(c.B, c.HW, c.C)
    tag = "f32in" if c.xf32 else "16in"
    print(f"NORMRSTD {c.id} {TNAME[dtype]} offset {c.offset:g} {tag} rstd_rel_err {rstd_rel_error(mr, mr_ref):.3e}")
    report(f"gn_stats[{tag}]", F32, c.id, nb.check(mr, mr_ref, e_mr, F32, nb.Where("stats", groups=c.groups), f"{c.id} (mean, rstd)"))
    report(f"gn_apply[{tag}]", dtype, c.id, nb.check(y, r, e, dtype, nb.Where("gn", HW=c.HW, C=c.C, groups=c.groups, ppc=ppc),
                                                     f"{c.id} groupnorm"))
    del r, e
    if c.xf32:
        return
    # ---- backward, from the forward's own (mean, rstd) buffer
    bchunks, bppc, _, _ = nb.gnb_geometry(c.B, c.HW, c.C)
    wh = nb.Where("gn", HW=c.HW, C=c.C, groups=c.groups, ppc=bppc)
    whc = nb.Where("cols", N=c.C)
    full = c.bwd == "full"
    dg0 = randn((c.C,), g) if full else None
    db0 = randn((c.C,), g) if full else None
    gs = 0.5 if full else 1.0
    if c.bwd == "null":
        dg = db = None
    else:
        dg, db = (dg0.clone(), db0.clone()) if full else (torch.full((c.C,), SENTINEL, device="cuda"), torch.full((c.C,), SENTINEL, device="cuda"))
    if c.pad:
        dyb, dy = wide((c.B, c.HW, c.C), c.C + c.pad, g, dtype)
        dxb, dx = wide((c.B, c.HW, c.C), c.C + c.pad + 8, g, dtype, fill=SENTINEL)
        addb, add = wide((c.B, c.HW, c.C), c.C + c.pad + 8, g, dtype)       # dx_add rows at dx's stride
        add = add if full else None
        gn_backward(L, x, dy, dx, mr, gamma, beta, c.groups, c.silu, dg, db, full, gs, add)
        assert bool((dxb[..., c.C:] == SENTINEL).all()), "groupnorm_bwd wrote outside its lddx view"
    else:
        dy = randn((c.B, c.HW, c.C), g, dtype)
        add = randn((c.B, c.HW, c.C), g, dtype) if full else None
        if c.bwd == "null":
            dx = torch.empty_like(x)
            gn_backward(L, x, dy, dx, mr, gamma, beta, c.groups, c.silu, None, None, False, 1.0, None)
        else:
            dx = ob.groupnorm_bwd(x, dy, mr, gamma, beta, c.groups, c.silu, dg, db, accumulate=full, grad_scale=gs, dx_add=add)
    ref = nb.gn_bwd_ref(x, dy, mr, gamma, beta, c.groups, c.silu, add, dg0, db0, gs)
    report("gn_bwd_dx", dtype, c.id, nb.check(dx, *ref["dx"], dtype, wh, f"{c.id} groupnorm_bwd dx"))
    if dg is not None:
        report("gn_bwd_dgamma", F32, c.id, nb.check(dg, *ref["dgamma"], F32, whc, f"{c.id} dgamma"))
        report("gn_bwd_dbeta", F32, c.id, nb.check(db, *ref["dbeta"], F32, whc, f"{c.id} dbeta"))


@pytest.mark.parametrize("dtype", DTYPES, ids=list(TNAME.values()))
def test_groupnorm_with_statistics_fused_into_the_producing_conv(env, dtype):
    """pre_partial: the conv's epilogue emitted the chunk sums (of the rounded 16-bit output, or of the fp32 output)."""
    ops, ob, L = env
    from diffews_amd.packing import pack_conv3x3
    g = gen(7)
    B, H, W, Cin, Cout = 3, 128, 128, 64, 256
    x = randn((B, H, W, Cin), g, dtype)
    w = pack_conv3x3(randn((Cout, Cin, 3, 3), g, dtype, (9 * Cin) ** -0.5).cpu()).cuda()
    bias, gamma, beta = randn((Cout,), g), randn((Cout,), g, F32, 0.2, 1.0), randn((Cout,), g, F32, 0.2)
    res = randn((B, H, W, Cout), g)
    for tag, y in (("16in", ops.conv3x3(x, w, Cout, bias=bias, gn_groups=32)),
                   ("f32in", ops.conv3x3(x, w, Cout, bias=bias, residual=res, out_f32=True, gn_groups=32))):
        st = getattr(y, "_gn_stats", None)
        assert st is not None, "fused statistics expected for this shape"
        out, mr = ops.groupnorm(y, gamma, beta, 32, 1e-6, silu=True, return_stats=True, out_dtype=dtype if y.dtype == F32 else None)
        yv = y.reshape(B, H * W, Cout)
        r, e, mr_ref, e_mr = nb.gn_fwd_ref(yv, gamma, beta, 32, 1e-6, True, pre_chunks=st[1])
        ppc = nb.gn_geometry(B, H * W, Cout)[1]
        report(f"gn_stats[pre,{tag}]", F32, "conv256", nb.check(mr, mr_ref, e_mr, F32, nb.Where("stats", groups=32), "fused (mean, rstd)"))
        report(f"gn_apply[pre,{tag}]", dtype, "conv256", nb.check(out, r, e, dtype, nb.Where("gn", HW=H * W, C=Cout, groups=32, ppc=ppc),
                                                                  "groupnorm from fused statistics"))


# ------------------------------------------------------------------------------------------------ LayerNorm

@pytest.mark.parametrize("dtype", DTYPES, ids=list(TNAME.values()))
@pytest.mark.parametrize("rows,Cc,pad,xf32", LN_CASES)
def test_layernorm_forward_and_backward(env, rows, Cc, pad, xf32, dtype):
    ops, ob, L = env
    g = gen(rows * 7 + Cc)
    xb = randn((rows, Cc + pad), g, F32, 3.0, 1.0)
    xb = xb if xf32 else xb.to(dtype)
    x = xb[:, :Cc]
    gamma, beta = randn((Cc,), g, F32, 0.5, 1.0), randn((Cc,), g, F32, 0.2)
    y = ops.layernorm(x, gamma, beta, EPS, out_dtype=dtype if xf32 else None)
    wh = nb.Where("rows", C=Cc)
    cid = f"{rows}x{Cc}" + (f"+{pad}" if pad else "")
    report(f"ln_kernel<{nb.ln_maxc(Cc)}>[{'f32in' if xf32 else '16in'}]", dtype, cid,
           nb.check(y, *nb.ln_fwd_ref(x, gamma, beta, EPS), dtype, wh, f"layernorm {cid}"))
    if xf32:
        return
    dyb = randn((rows, Cc + pad), g, dtype)
    dy = dyb[:, :Cc]
    for full in (False, True):
        dg0, db0 = (randn((Cc,), g), randn((Cc,), g)) if full else (None, None)
        dg = dg0.clone() if full else torch.full((Cc,), SENTINEL, device="cuda")
        db = db0.clone() if full else torch.full((Cc,), SENTINEL, device="cuda")
        add = randn((rows, Cc), g, dtype) if full else None
        gs = 0.5 if full else 1.0
        dx = ob.layernorm_bwd(x, dy, gamma, dg, db, EPS, accumulate=full, grad_scale=gs, dx_add=add)
        ref = nb.ln_bwd_ref(x, dy, gamma, EPS, add, dg0, db0, gs)
        k = f"ln_bwd_kernel<{nb.ln_maxc(Cc)}>"
        report(k + " dx", dtype, cid, nb.check(dx, *ref["dx"], dtype, wh, f"layernorm_bwd dx {cid}"))
        whc = nb.Where("cols", N=Cc)
        report("ln_bwd dgamma", F32, cid, nb.check(dg, *ref["dgamma"], F32, whc, f"layernorm_bwd dgamma {cid}"))
        report("ln_bwd dbeta", F32, cid, nb.check(db, *ref["dbeta"], F32, whc, f"layernorm_bwd dbeta {cid}"))


# ------------------------------------------------------------------------------------------------ column sums

def colsum_operands(dtype, g):
    """Every (case, variant): x view [segs * rps, N], the initial out buffer [segs, N + out pad], scale, accumulate."""
    items = []
    for rps, segs, N in COLSUM_CASES:
        for xpad, opad, scale, accum in COLSUM_VARIANTS:
            xb = randn((segs * rps, N + xpad), g, dtype, 1.0, 0.25)
            out0 = randn((segs, N + opad), g)
            items.append(((rps, segs, N), xb[:, :N], out0, scale, accum))
    return items


@pytest.mark.parametrize("dtype", DTYPES, ids=list(TNAME.values()))
def test_colsum_single_calls_and_one_queue_flush(env, dtype):
    """Every case and variant through colsum() and through ONE ColsumQueue.flush() of all of them (55 items, three table
    writes): bit-equal results, each within the bound, columns outside the out view untouched."""
    ops, ob, L = env
    items = colsum_operands(dtype, gen(11))
    assert len(items) >= 50
    q = ob.ColsumQueue()
    single, batched = [], []
    for (rps, segs, N), x, out0, scale, accum in items:
        o1, o2 = out0.clone(), out0.clone()
        ob.colsum(x, segs=segs, out=o1[:, :N], accumulate=accum, scale=scale)
        q.add(x, o2[:, :N], segs=segs, accumulate=accum, scale=scale)
        single.append(o1)
        batched.append(o2)
    q.flush()
    torch.cuda.synchronize()
    for i, ((rps, segs, N), x, out0, scale, accum) in enumerate(items):
        cid = f"{rps}x{segs}x{N}/v{i % len(COLSUM_VARIANTS)}"
        assert torch.equal(single[i], batched[i]), f"ColsumQueue item {i} ({cid}) differs from colsum()"
        assert torch.equal(single[i][:, N:], out0[:, N:]), f"colsum {cid} wrote outside its ldo view"
        r, e = nb.colsum_ref(x, segs, scale, out0[:, :N] if accum else None)
        report("colsum", F32, cid, nb.check(single[i][:, :N], r, e, F32, nb.Where("cols", N=N), f"colsum {cid}"))


# ------------------------------------------------------------------------------------------------ softmax

@pytest.mark.parametrize("dtype", DTYPES, ids=list(TNAME.values()))
@pytest.mark.parametrize("Lr", SOFTMAX_L)
def test_softmax_rows(env, Lr, dtype):
    ops, ob, L = env
    g = gen(Lr)
    x = randn((37, Lr), g, F32, 4.0)
    x[5, :] = -30.0
    x[5, Lr - 1] = 25.0          # the maximum in the last column
    x[6, :] = 1.75               # a row of equal values
    x[7, :Lr // 2] -= 200.0      # the left half of the row underflows
    y = ops.softmax_rows(x, dtype, scale=0.3)
    kernel = "softmax_rows_reg_kernel" if Lr <= 4096 and Lr % 4 == 0 else "softmax_rows_kernel"
    report(kernel, dtype, f"L{Lr}", nb.check(y, *nb.softmax_rows_ref(x, 0.3), dtype, nb.Where("rows", C=Lr), f"softmax_rows L={Lr}"))


@pytest.mark.parametrize("dtype", DTYPES, ids=list(TNAME.values()))
@pytest.mark.parametrize("rows,ld,groups,Lg", SOFTMAX_GROUPS)
def test_softmax_groups(env, rows, ld, groups, Lg, dtype):
    ops, ob, L = env
    x = randn((rows, ld), gen(rows), F32, 3.0)
    y = ops.softmax_groups(x, groups, Lg, dtype)
    assert float(y[:, groups * Lg:].float().abs().sum()) == 0.0, "padding columns must be exactly zero"
    report("softmax_groups", dtype, f"{rows}x{ld}/{groups}x{Lg}",
           nb.check(y, *nb.softmax_groups_ref(x, groups, Lg), dtype, nb.Where("rows", C=ld), "softmax_groups"))


# ------------------------------------------------------------------------------------------------ pointwise, loss, optimizer

@pytest.mark.parametrize("dtype", DTYPES, ids=list(TNAME.values()))
@pytest.mark.parametrize("rows,H", GEGLU_CASES)
def test_geglu(env, rows, H, dtype):
    ops, ob, L = env
    g = gen(rows + H)
    pre, dout = randn((rows, 2 * H), g, dtype, 1.5), randn((rows, H), g, dtype)
    assert (rows, H) != GEGLU_CASES[0] or rows * H // 8 > nb.grid_for(rows * H // 8) * 256
    report("geglu_fwd", dtype, f"{rows}x{H}", nb.check(ob.geglu_fwd(pre), *nb.geglu_fwd_ref(pre), dtype, nb.Where("rows", C=H), "geglu_fwd"))
    report("geglu_bwd", dtype, f"{rows}x{H}",
           nb.check(ob.geglu_bwd(pre, dout), *nb.geglu_bwd_ref(pre, dout), dtype, nb.Where("rows", C=2 * H), "geglu_bwd"))


@pytest.mark.parametrize("dtype", DTYPES, ids=list(TNAME.values()))
def test_elementwise_modes(env, dtype):
    ops, ob, L = env
    g = gen(3)
    a, b = randn((2, 96, 96, 512), g, dtype), randn((2, 96, 96, 512), g, dtype)
    assert a.numel() // 8 > nb.grid_for(a.numel() // 8) * 256           # more 16-byte pieces than threads: the grid-stride loop runs
    report("ew add", dtype, "2x96x96x512", nb.check(ob.add(a, b), *nb.add_ref(a, b), dtype, nb.Where("rows", C=512), "add"))
    big = randn((2, 192, 192, 320), g, dtype)
    report("ew pool2x2", dtype, "2x192x192x320", nb.check(ob.pool2x2_sum(big), *nb.pool2x2_ref(big), dtype, nb.Where("rows", C=320), "pool2x2_sum"))
    assert torch.equal(ob.slice_channels(a, 64, 128), a[..., 64:192])
    z = ob.zero_stuff2x(a[:, :8, :8].contiguous())
    assert torch.equal(z[:, ::2, ::2], a[:, :8, :8])
    z[:, ::2, ::2] = 0
    assert int((z != 0).sum()) == 0, "zero_stuff2x wrote a non-zero outside the even positions"
    s, d = randn((3, 1000, 320), g, dtype, 3.0), randn((3, 1000, 320), g, dtype)
    report("silu", dtype, "3x1000x320", nb.check(ob.silu(s), *nb.silu_ref(s), dtype, nb.Where("rows", C=320), "silu"))
    report("silu_grad", dtype, "3x1000x320", nb.check(ob.silu(s, d), *nb.silu_ref(s, d), dtype, nb.Where("rows", C=320), "silu backward"))


@pytest.mark.parametrize("dtype", DTYPES, ids=list(TNAME.values()))
@pytest.mark.parametrize("shape", [(2, 4, 16, 16), (3, 4, 64, 64), (1, 3, 7, 5)])
def test_loss_kernels(env, shape, dtype):
    ops, ob, L = env
    g = gen(sum(shape))
    pred, tgt = randn(shape, g), randn(shape, g)
    Bn, Cc, H, W = shape
    sid = "x".join(map(str, shape))
    nchw = torch.empty(shape, device="cuda")
    loss, dpred = ob.mse_loss(pred, tgt, dtype, loss_scale=8.0, dpred_nchw_out=nchw)
    (lr, le), (gr, ge) = nb.mse_ref(pred, tgt, 8.0)
    report("mse loss", F32, sid, nb.check(loss, lr, le, F32, label="mse loss"))
    report("mse dpred", dtype, sid, nb.check(dpred[..., :Cc].permute(0, 3, 1, 2), gr, ge, dtype, label="mse dpred"))
    assert float(dpred[..., Cc:].float().abs().sum()) == 0.0
    assert torch.equal(nchw, dpred[..., :Cc].permute(0, 3, 1, 2).float())
    nchw2 = torch.empty(shape, device="cuda")
    dp = ob.loss_grad(pred, dtype, scale=0.37, dpred_nchw_out=nchw2)
    report("loss_grad", dtype, sid, nb.check(dp[..., :Cc].permute(0, 3, 1, 2), *nb.loss_grad_ref(pred, 0.37), dtype, label="loss_grad"))
    assert float(dp[..., Cc:].float().abs().sum()) == 0.0 and torch.equal(nchw2, dp[..., :Cc].permute(0, 3, 1, 2).float())


@pytest.mark.parametrize("n,off", [(100_003, 0), (100_003, 1), (1 << 20, 0), ((1 << 20) + 3, 3), (5, 1), (4_000_001, 0)])
def test_sumsq(env, n, off):
    """off != 0: the pointer is 4 x off bytes past a 16-byte boundary (the scalar path); n % 4 != 0: a scalar tail."""
    ops, ob, L = env
    buf = randn((n + off,), gen(n), F32, 3.0)
    x = buf[off:]
    assert (x.data_ptr() % 16 != 0) == (off % 4 != 0)
    report("sumsq", F32, f"n{n}+{off}", nb.check(ob.sumsq(x), *nb.sumsq_ref(x), F32, label="sumsq"))


@pytest.mark.parametrize("dtype", DTYPES, ids=list(TNAME.values()))
def test_adamw_per_element(env, dtype):
    """Three fused AdamW steps with the gradient clip, each checked per element (master, both moments, the 16-bit shadow)
    against an fp64 step from the state the kernel started from."""
    ops, ob, L = env
    n = 100_003
    g = gen(5)
    p, gr = randn((n,), g), randn((n,), g, F32, 3.0)
    gr[::97] = 0.0
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shadow = torch.empty(n, dtype=dtype, device="cuda")
    hp = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2)
    for step in (1, 2, 3):
        gc = gr * step * (0.01 if step == 3 else 1.0)          # the third step is not clipped
        ss = ob.sumsq(gc)
        ref = nb.adamw_ref(p, gc, m, v, step, sumsq=float(ss), max_norm=1.0, **hp)
        ob.adamw(p, gc, m, v, step, hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["wd"],
                 grad_sumsq=ss, max_grad_norm=1.0, shadow=shadow)
        for name, t in (("p", p), ("m", m), ("v", v)):
            report(f"adamw {name}", F32, f"step{step}", nb.check(t, *ref[name], F32, label=f"adamw {name} step {step}"))
        report("adamw shadow", dtype, f"step{step}", nb.check(shadow, *ref["p"], dtype, label=f"adamw shadow step {step}"))
        assert torch.equal(shadow, p.to(dtype))
