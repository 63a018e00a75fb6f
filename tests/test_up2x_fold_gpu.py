"""GPU tests of the folded nearest-2x upsample conv (dfw_conv_up2x, gemm8_kernel<.., up2x>; ops.conv3x3_up2x, ops.conv3x3_stream's w_up2x).

Shapes (B, Hi, Wi, Cin, Cout), the smallest at which the kernel can go wrong:
    (1, 16, 16,  64, 128)   one tile per parity, four K-tiles
    (2, 16, 32, 128, 256)   the 256-wide tile, two tiles per row, an image boundary, H != W
    (1, 32, 16,  64, 192)   ragged last tile column of the 128-wide tile
    (4, 64, 80,  64, 256), (2, 64, 80, 64, 192)   320 tiles on 256 persistent workgroups: the A / W cursors and the epilogue
                            cross from one tile to the next (another parity, another n-tile, another image)
in both storage dtypes.

Parity bounds (elementwise_bound.py, imported, not edited).  S is the float64 result of the four 2x2 parity convs with the
folded, ROUNDED weights the kernel reads, absS the same expression on absolute values, and every element must satisfy
    |y - r| <= u_T |r| + C_ACC 2^-24 (sqrt(4 Cin) absS + |bias|) + floor_T,          r = S + bias
(eb.epilogue_ref with K = 4 Cin, the K the kernel walks).  Against the UNFOLDED float64 reference r9 (eb.conv_ref, ups) the
allowance grows by the one extra rounding the fold adds: a folded weight is fl(sum of <= 4 weights), off by at most
u_w |sum| <= u_w sum|w|, so |S - S9| <= u_w sum|a||w| = u_w absS9.  u_w is taken as 2^-9 for bf16 and 2^-11 for fp16;
round-to-nearest bf16 is 2^-8 in the worst case, so the bf16 figure is the tighter of the two readings and is kept.
Nothing here was fitted to a measurement; -s prints the worst err / bound ratios (lines starting with UP2XRATIO).
"""
import math

import pytest
import torch

import elementwise_bound as eb
import norm_bound as nb

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
TNAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
U_FOLD = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
SHAPES = [(1, 16, 16, 64, 128), (2, 16, 32, 128, 256), (1, 32, 16, 64, 192),
          # more tiles than the 256 workgroups of the persistent walk (320 each): cursors that cross tiles, parities and n-tiles
          (4, 64, 80, 64, 256), (2, 64, 80, 64, 192)]
F64 = torch.float64


def _case(shape, dtype, seed=0):
    """x NHWC, the unfolded pack (16-bit), the folded pack (folded from the 16-bit weights, rounded once), fp32 bias."""
    from diffews_amd import packing
    B, Hi, Wi, Cin, Cout = shape
    g = torch.Generator().manual_seed(1000 * seed + Hi * Wi + Cin + Cout)
    x = torch.randn(B, Hi, Wi, Cin, generator=g).to(dtype).cuda()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to(dtype)
    wp = packing.pack_conv3x3(w)
    wf = packing.fold_up2x(wp)
    bias = torch.randn(Cout, generator=g).cuda()
    return x, wp.cuda(), wf.cuda(), bias


def folded_ref(x, wf):
    """fp64 (S, absS) [B*2Hi*2Wi, Cout] in NHWC output order: per parity, four shifted GEMMs over the zero-padded input."""
    B, Hi, Wi, Cin = x.shape
    Cout = wf.shape[0]
    w = wf.to(F64).view(Cout, 2, 2, 2, 2, Cin)
    xp = x.new_zeros(B, Hi + 2, Wi + 2, Cin, dtype=F64)
    xp[:, 1:Hi + 1, 1:Wi + 1] = x.to(F64)
    S = x.new_zeros(B, 2 * Hi, 2 * Wi, Cout, dtype=F64)
    A = torch.zeros_like(S)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    col = xp[:, ty + py:ty + py + Hi, tx + px:tx + px + Wi].reshape(-1, Cin)      # source (y + ty - 1 + py, ..)
                    wt = w[:, py, px, ty, tx]
                    S[:, py::2, px::2] += (col @ wt.t()).view(B, Hi, Wi, Cout)
                    A[:, py::2, px::2] += (col.abs() @ wt.abs().t()).view(B, Hi, Wi, Cout)
    return S.view(-1, Cout), A.view(-1, Cout)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TNAME[d])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_element_is_inside_its_bound(hip_lib, shape, dtype):
    from diffews_amd import ops
    B, Hi, Wi, Cin, Cout = shape
    x, wp, wf, bias = _case(shape, dtype)
    y = ops.conv3x3_up2x(x, wf, Cout, bias=bias)
    assert y is not None and y.shape == (B, 2 * Hi, 2 * Wi, Cout) and y.dtype == dtype
    where = eb.Where(Cout, 4 * Hi * Wi, 2 * Wi)
    S, absS = folded_ref(x, wf)
    r, e = eb.epilogue_ref(S, absS, 4 * Cin, bias=bias)
    worst = eb.check(y, r, e, dtype, where, f"up2x {shape} {TNAME[dtype]} against the folded fp64 reference")
    S9, absS9 = eb.conv_ref(x, wp, ups=True)
    r9, _ = eb.epilogue_ref(S9, absS9, 9 * Cin, bias=bias)
    worst9 = eb.check(y, r9, e + U_FOLD[dtype] * absS9, dtype, where, f"up2x {shape} {TNAME[dtype]} against the unfolded fp64 reference")
    print(f"UP2XRATIO {shape} {TNAME[dtype]} folded {worst:.3g} unfolded {worst9:.3g}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TNAME[d])
def test_impulses_return_the_folded_weights_bit_for_bit(hip_lib, dtype):
    """One 1.0 per image: the four corners, an edge pixel on a tile boundary, an interior pixel next to one.  Source pixel
    (sy, sx) is tap (ty, tx) of low-resolution position (sy - ty + 1 - py, sx - tx + 1 - px) of parity (py, px): the output
    holds exactly those folded weights there (1.0 x w + zeros is exact in fp32, and w is already a storage value), zero
    elsewhere -- all 16 (parity, tap) offsets and the bounds check."""
    from diffews_amd import ops
    Hi, Wi, Cin, Cout, c0 = 32, 16, 64, 128, 37
    spots = [(0, 0), (0, Wi - 1), (Hi - 1, 0), (Hi - 1, Wi - 1), (16, 0), (15, 7)]
    B = len(spots)
    _, _, wf, _ = _case((B, Hi, Wi, Cin, Cout), dtype, seed=1)
    x = torch.zeros(B, Hi, Wi, Cin, dtype=dtype, device="cuda")
    want = torch.zeros(B, 2 * Hi, 2 * Wi, Cout, dtype=dtype, device="cuda")
    w6 = wf.view(Cout, 2, 2, 2, 2, Cin)
    placed = 0
    for b, (sy, sx) in enumerate(spots):
        x[b, sy, sx, c0] = 1.0
        for py in range(2):
            for px in range(2):
                for ty in range(2):
                    for tx in range(2):
                        yl, xl = sy - ty + 1 - py, sx - tx + 1 - px
                        if 0 <= yl < Hi and 0 <= xl < Wi:
                            want[b, 2 * yl + py, 2 * xl + px] = w6[:, py, px, ty, tx, c0]
                            placed += 1
    assert placed == 4 * 9 + 12 + 16          # a corner reaches 9 output pixels, an edge pixel 12, an interior one 16
    y = ops.conv3x3_up2x(x, wf, Cout)
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


def _chunk_sums(y, groups, bn):
    """fp64 (sum, sum of squares, sum |y|, n) per (image, chunk, group) in the kernel's chunk order: low-resolution 16 x 16
    tile (row-major), parity 2 py + px, wave row (8 / (bn / 64) of them, 16 / that many low-resolution rows each)."""
    B, Ho, Wo, N = y.shape
    Hi, Wi, wgm, cpg = Ho // 2, Wo // 2, 8 // (bn // 64), N // groups
    band = 16 // wgm
    # [B, Hi/16, wgm, band, py, Wi/16, 16, px, groups, cpg] -> [B, tile_y, tile_x, py, px, wm, group, band x 16 x cpg]
    v = y.to(F64).reshape(B, Hi // 16, wgm, band, 2, Wi // 16, 16, 2, groups, cpg)
    v = v.permute(0, 1, 5, 4, 7, 2, 8, 3, 6, 9).reshape(B, (Hi // 16) * (Wi // 16) * 4 * wgm, groups, band * 16 * cpg)
    return v.sum(-1), (v * v).sum(-1), v.abs().sum(-1), v.shape[-1]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TNAME[d])
@pytest.mark.parametrize("shape,groups", [((1, 16, 16, 64, 128), 32), ((2, 16, 32, 128, 256), 32), ((1, 32, 16, 64, 192), 24)],
                         ids=["128c", "256c", "192c"])
def test_groupnorm_partial_sums_feed_groupnorm(hip_lib, shape, groups, dtype):
    from diffews_amd import ops
    B, Hi, Wi, Cin, Cout = shape
    x, wp, wf, bias = _case(shape, dtype, seed=2)
    y = ops.conv3x3_up2x(x, wf, Cout, bias=bias, gn_groups=groups)
    st = getattr(y, "_gn_stats", None)
    bn = 256 if Cout % 256 == 0 else 128
    assert st is not None and st[1] == 4 * (Hi // 16) * (Wi // 16) * (8 // (bn // 64)) and st[2] == groups
    part = st[0]
    assert tuple(part.shape) == (B, st[1], groups, 2)
    # the sums themselves: elementwise_bound.gn_chunk_check's tolerance (fp32 summation of n terms in any order)
    s, q, a, n = _chunk_sums(y, groups, bn)
    got = part.to(F64)
    assert torch.isfinite(got).all()
    ratio = torch.maximum((got[..., 0] - s).abs() / (n * 2.0 ** -24 * a + 1e-30), (got[..., 1] - q).abs() / ((n + 1) * 2.0 ** -24 * q + 1e-30))
    assert float(ratio.max()) <= 1.0, f"chunk sums off, worst ratio {float(ratio.max()):.3g} at {torch.nonzero(ratio == ratio.max())[0].tolist()}"
    # GroupNorm fed by them against GroupNorm of the same tensor with its own statistics pass: both inside norm_bound's
    # allowance around one fp64 reference (pre_chunks: re-associated fp32 chunk sums)
    g = torch.Generator().manual_seed(5)
    gamma, beta = (torch.randn(Cout, generator=g) * 0.5 + 1.0).cuda(), torch.randn(Cout, generator=g).cuda()
    fed = ops.groupnorm(y, gamma, beta, groups, 1e-6, silu=True)
    plain_in = y.clone()
    assert getattr(plain_in, "_gn_stats", None) is None
    plain = ops.groupnorm(plain_in, gamma, beta, groups, 1e-6, silu=True)
    y3 = y.view(B, 4 * Hi * Wi, Cout)
    where = nb.Where("gn", HW=4 * Hi * Wi, C=Cout, groups=groups, ppc=1)
    r, e, _, _ = nb.gn_fwd_ref(y3, gamma, beta, groups, 1e-6, True, pre_chunks=st[1])
    w_fed = nb.check(fed, r, e, dtype, where, "groupnorm fed by the up2x partial sums")
    r0, e0, _, _ = nb.gn_fwd_ref(y3, gamma, beta, groups, 1e-6, True)
    w_plain = nb.check(plain, r0, e0, dtype, where, "groupnorm with its own statistics")
    print(f"UP2XRATIO gn {shape} {TNAME[dtype]} sums {float(ratio.max()):.3g} fed {w_fed:.3g} plain {w_plain:.3g}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TNAME[d])
def test_fallback_and_switch_take_the_unfolded_route(hip_lib, dtype):
    from diffews_amd import ops
    rec = []
    hook = lambda name, flops, e0, e1, shape=None: rec.append((name, flops, shape))
    t = TNAME[dtype]
    # Hi = 8 is not a multiple of 16: the old route, bit for bit, under the old kernel's name
    shape = (2, 8, 16, 64, 128)
    x, wp, wf, bias = _case(shape, dtype, seed=3)
    assert ops.conv3x3_up2x(x, wf, 128, bias=bias) is None
    old = ops.conv3x3(x, wp, 128, bias=bias, ups=True, gn_groups=32)
    ops.gemm_hook = hook
    try:
        ops.conv3x3(x, wp, 128, bias=bias, ups=True)
        y = ops.conv3x3_stream(x, wp, 128, bias=bias, ups=True, gn_groups=32, w_up2x=wf)
    finally:
        ops.gemm_hook = None
    assert torch.equal(y, old) and rec[1][0] == rec[0][0] and "up2x" not in rec[1][0] and rec[1][2][5] == 1
    assert (getattr(y, "_gn_stats", None) is None) == (getattr(old, "_gn_stats", None) is None)
    # an eligible shape: folded by default (executed FLOPs 2 M N 4 Cin), unfolded with the switch off
    shape = (1, 16, 16, 64, 128)
    x, wp, wf, bias = _case(shape, dtype, seed=3)
    old = ops.conv3x3(x, wp, 128, bias=bias, ups=True)
    rec.clear()
    ops.gemm_hook = hook
    try:
        new = ops.conv3x3_stream(x, wp, 128, bias=bias, ups=True, w_up2x=wf)
        assert ops.UP2X_FOLD is True
        ops.UP2X_FOLD = False
        try:
            off = ops.conv3x3_stream(x, wp, 128, bias=bias, ups=True, w_up2x=wf)
        finally:
            ops.UP2X_FOLD = True
        f32 = ops.conv3x3_stream(x.float(), wp, 128, bias=bias, ups=True, w_up2x=wf)      # the fp32 residual stream stays unfolded
    finally:
        ops.gemm_hook = None
    M = 4 * 16 * 16
    assert rec[0] == (f"gemm8_kernel<{t},256,128,64,up2x>", 2.0 * M * 128 * 4 * 64, (M, 128, 4 * 64, 4, 1, 1, 1, 1))
    assert "up2x" not in rec[1][0] and rec[1][1] == 2.0 * M * 128 * 9 * 64 and torch.equal(off, old)
    assert all("up2x" not in r[0] for r in rec[2:]) and f32.dtype == torch.float32
    assert torch.equal(new, ops.conv3x3_up2x(x, wf, 128, bias=bias))


def test_capture_and_replay_equal_eager(hip_lib):
    from diffews_amd import ops
    import ctypes as C
    shape = (2, 16, 32, 128, 256)
    x, wp, wf, bias = _case(shape, torch.bfloat16, seed=4)
    eager = [ops.conv3x3_up2x(x, wf, 256, bias=bias, gn_groups=32)]          # also warms the allocator
    x2 = (x.float() * -0.5 + 0.25).to(x.dtype)
    eager.append(ops.conv3x3_up2x(x2, wf, 256, bias=bias, gn_groups=32))
    xs = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = ops.conv3x3_up2x(xs, wf, 256, bias=bias, gn_groups=32)
    n = C.c_int32(0)
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(n)) == 0
    graph.instantiate()
    for src, want in ((x, eager[0]), (x2, eager[1])):
        xs.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(out._gn_stats[0], want._gn_stats[0])
