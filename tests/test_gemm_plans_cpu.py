"""CPU tests (no GPU) of the per-element checker (tests/elementwise_bound.py) and of the plan coverage of
tests/test_gemm_plans_gpu.py: every case plans the kernel it names, and together the cases reach every kernel
instantiation dfw_gemm and dfw_gemm_tn can launch -- evaluated through the host-only plan queries, no device call."""
import math

import pytest
import torch
import torch.nn.functional as F

import elementwise_bound as eb

BF16, F16 = torch.bfloat16, torch.float16
_P = {BF16: 8, F16: 11}         # significand bits


def _ulp(v, dtype):
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e - _P[dtype])


def _truncate(r, dtype):
    """fp64 r rounded toward zero to the precision of dtype (normal range)."""
    m, e = torch.frexp(r)
    return torch.ldexp(torch.trunc(torch.ldexp(m, torch.full_like(e, _P[dtype]))), e - _P[dtype]).to(dtype)


def _rnd(shape, g, dtype, scale=1.0):
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dtype)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_checker_accepts_rounded_and_rejects_off_by_two_ulps_and_truncation(dtype):
    g = torch.Generator().manual_seed(1)
    M, N, K = 192, 160, 320
    a, w = _rnd((M, K), g, dtype), _rnd((N, K), g, dtype, K ** -0.5)
    bias, res = _rnd((N,), g, torch.float32, 0.5), _rnd((M, N), g, dtype)
    S, A = eb.gemm_ref(a, w)
    r, e = eb.epilogue_ref(S, A, K, bias=bias, residual=res, out_scale=0.5)
    y = r.to(dtype)                                            # correctly rounded exact result
    assert eb.check(y, r, e, dtype, label="rounded") <= 1.0
    # one element moved by two ulps (a mantissa in [0.5, 0.7): the move stays inside its binade)
    mant = torch.frexp(y.double())[0].abs().flatten()
    i = int(torch.nonzero((mant >= 0.5) & (mant < 0.7))[0])
    moved = y.clone().flatten()
    moved[i] = (moved[i].double() + 2 * _ulp(moved[i].double(), dtype) * torch.sign(moved[i].double())).to(dtype)
    with pytest.raises(AssertionError, match=f"row {i // N}, channel {i % N}"):
        eb.check(moved.view(M, N), r, e, dtype, where=eb.Where(N), label="two ulps")
    with pytest.raises(AssertionError, match="outside the bound"):
        eb.check(_truncate(r, dtype), r, e, dtype, label="truncated")


def test_checker_flags_one_tile_missing_one_k_chunk_that_global_l2_accepts():
    """One 32 x 32 tile of a 2048 x 2048 bf16 output without one 64-deep K-chunk: relative L2 against the reference
    (test_ops_gpu's criterion) stays under its bf16 tolerance, the per-element bound names the tile."""
    from test_ops_gpu import TOL, rel
    g = torch.Generator().manual_seed(2)
    M = N = K = 2048
    a, w = _rnd((M, K), g, BF16), _rnd((N, K), g, BF16, K ** -0.5)
    S, A = eb.gemm_ref(a, w)
    r, e = eb.epilogue_ref(S, A, K)
    y = r.to(BF16)
    rows, cols, ks = slice(64, 96), slice(32, 64), slice(640, 704)     # tile (2, 1), K-chunk 10
    bad = r.clone()
    bad[rows, cols] -= a[rows, ks].double() @ w[cols, ks].double().t()
    y_bad = y.clone()
    y_bad[rows, cols] = bad[rows, cols].to(BF16)
    assert eb.check(y, r, e, BF16) <= 1.0
    assert rel(y_bad, r) < TOL[BF16], rel(y_bad, r)                   # the gap: global L2 passes
    with pytest.raises(AssertionError, match=r"tile \(2, 1\)"):
        eb.check(y_bad, r, e, BF16, where=eb.Where(N, tile=(32, 32)), label="dropped chunk")


@pytest.mark.parametrize("stride,pad,ups", [(1, 1, False), (2, 1, False), (2, 0, False), (1, 1, True)])
def test_conv_reference_geometry(stride, pad, ups):
    """The nine-shift fp64 conv reference against torch's CPU conv in fp64 (the VAE's pad 0 = F.pad(0, 1, 0, 1) + conv
    with padding 0; fused nearest-2x upsampling)."""
    from diffews_amd.packing import pack_conv3x3
    g = torch.Generator().manual_seed(3)
    x, w = _rnd((2, 7, 10, 16), g, torch.float64), _rnd((24, 16, 3, 3), g, torch.float64)
    S, A = eb.conv_ref(x, pack_conv3x3(w), stride, pad, ups)
    xin = x.permute(0, 3, 1, 2)
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    if pad == 0:
        xin = F.pad(xin, (0, 1, 0, 1))
    ref = F.conv2d(xin, w, stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(S.shape)
    assert torch.allclose(S, ref, rtol=0, atol=1e-12)
    assert (A >= S.abs() - 1e-12).all()


def test_gn_chunk_check_maps_chunks_to_their_pixels():
    """gn_chunk_check against a direct per-chunk loop; a chunk moved to another slot, or never written, fails."""
    g = torch.Generator().manual_seed(4)
    B, Ho, Wo, N, groups, bm, bn = 2, 32, 48, 128, 16, 512, 128
    y = _rnd((B, Ho, Wo, N), g, torch.float32)
    wgm, bh = 8 // (bn // 64), bm // 16
    band, tpr = bh // wgm, Wo // 16
    chunks = (Ho // bh) * tpr * wgm
    part = torch.zeros(B, chunks, groups, 2)
    for b in range(B):
        for c in range(chunks):
            patch, wm = divmod(c, wgm)
            ty, tx = divmod(patch, tpr)
            oy = ty * bh + wm * band
            blk = y[b, oy:oy + band, tx * 16:tx * 16 + 16].double().reshape(-1, groups, N // groups)
            part[b, c, :, 0] = blk.sum((0, 2)).float()
            part[b, c, :, 1] = (blk * blk).sum((0, 2)).float()
    assert eb.gn_chunk_check(y, part, groups, bm, bn) <= 1.0
    swapped = part.clone()
    swapped[1, [3, 5]] = part[1, [5, 3]]
    with pytest.raises(AssertionError, match="image 1, chunk [35]"):
        eb.gn_chunk_check(y, swapped, groups, bm, bn)
    unwritten = part.clone()
    unwritten[0, 2, 7] = math.nan
    with pytest.raises(AssertionError, match="image 0, chunk 2 .*group 7"):
        eb.gn_chunk_check(y, unwritten, groups, bm, bn)


# ---- plan coverage

# Every instantiation dfw_gemm launches per storage dtype T, with the dispatch line that launches it: gemm.hip's gemm_plan
# picks the kernel family and the tile (GemmPlan pl), the family's launch_* function switches on the plan.  RF32 / F32O: the
# fp32-residual / fp32-output forms (planned name + residual / output dtype).
FORWARD_INSTANTIATIONS = {
    **{f"gemm_kernel<T,{t},{k}>": f"gemm.hip launch_gemm -> launch_tile: gemm_kernel<T, BM, BN, {c}> ({t})"
       for t in ("128,128", "128,64", "64,64") for k, c in (("lin", "false"), ("conv", "true"))},
    **{f"gemm_kernel<T,{t},{k},RF32>": f"gemm.hip launch_gemm -> launch_tile: if (pl.rf32) gemm_kernel<T, BM, BN, {c}, true> ({t})"
       for t in ("128,128", "128,64", "64,64") for k, c in (("lin", "false"), ("conv", "true"))},
    "splitk_reduce_kernel<T>": "gemm.hip launch_tile: if (p.splitk > 1) splitk_reduce_kernel<T>",
    **{f"gemm_big_kernel<T,256,256,32,{k}>": "gemm_big.hip launch_gemm_big: if (pl.bn == 256) launch_big<T, 256, 256, 32, 4, 1, true, true>"
       for k in ("lin", "conv")},
    **{f"gemm_big_kernel<T,512,128,32,{k}>": "gemm_big.hip launch_gemm_big: if (pl.bm == 512) launch_big<T, 512, 128, 32, 4, 1, true, true>"
       for k in ("lin", "conv")},
    **{f"gemm_big_kernel<T,256,128,64,{k}>": "gemm_big.hip launch_gemm_big: if (pl.bk == 64) launch_big<T, 256, 128, 64, 3, 1>"
       for k in ("lin", "conv")},
    **{f"gemm_big_kernel<T,256,128,32,{k}>": "gemm_big.hip launch_gemm_big: launch_big<T, 256, 128, 32, 4, 1>"
       for k in ("lin", "conv")},
    **{f"gemm_big_kernel<T,256,256,32,{k},F32O>":
       "gemm_big.hip launch_gemm_big: if (pl.f32o && pl.bm == 256) launch_big<T, 256, 256, 32, 4, 1, true, true, true>" for k in ("lin", "conv")},
    **{f"gemm_big_kernel<T,512,128,32,{k},F32O>":
       "gemm_big.hip launch_gemm_big: if (pl.f32o) launch_big<T, 512, 128, 32, 4, 1, true, true, true>" for k in ("lin", "conv")},
    "gemm8_kernel<T,256,256,64,lin>": "gemm.hip gemm_plan: gemm_big rung, if (pl.bm == 256 && gemm8_eligible(p, pl.bn)); gemm8.hip launch_gemm8: launch8<T, 256>",
    "gemm8_kernel<T,256,256,64,conv>": "gemm.hip gemm_plan: gemm_big rung, if (pl.bm == 256 && gemm8_eligible(p, pl.bn)); gemm8.hip launch_gemm8: launch8<T, 256>",
    "gemm8_kernel<T,256,128,64,lin>": "gemm.hip gemm_plan: gemm_big rung, if (pl.bm == 256 && gemm8_eligible(p, pl.bn)); gemm8.hip launch_gemm8: launch8<T, 128>",
    "gemm8_kernel<T,256,128,64,conv>": "gemm.hip gemm_plan: gemm_big rung, if (pl.bm == 256 && gemm8_eligible(p, pl.bn)); gemm8.hip launch_gemm8: launch8<T, 128>",
    "gemm8_kernel<T,256,160,64,lin>": "gemm.hip gemm_plan: if (gemm8_n160_eligible(p)); gemm8.hip launch_gemm8: launch8<T, 160>",
    "conv_patch_kernel<T,512,128>": "conv_patch.hip launch_conv_patch: if (pl.bm == 512) launch_patch<T, 512, 128>",
    "conv_patch_kernel<T,256,256>": "conv_patch.hip launch_conv_patch: launch_patch<T, 256, 256>",
    "conv_patch_kernel<T,512,128,F32O>": "conv_patch.hip launch_conv_patch: if (pl.f32o && pl.bm == 512) launch_patch<T, 512, 128, true>",
    "conv_patch_kernel<T,256,256,F32O>": "conv_patch.hip launch_conv_patch: if (pl.f32o) launch_patch<T, 256, 256, true>",
    "conv_patch8_kernel<T,256,256>": "conv_patch8.hip launch_conv_patch8: if (pl.bn == 256) launch_patch8<T, 256>",
    "conv_patch8_kernel<T,256,128>": "conv_patch8.hip launch_conv_patch8: launch_patch8<T, 128>",
    "conv_patch8_kernel<T,256,160>": "conv_patch8.hip launch_conv_patch8: if (pl.bn == 160) launch_patch8<T, 160>",
}

# Every kernel dfw_gemm_tn launches per storage dtype T (tn_reduce_kernel is fp32-only: one for both).
TN_INSTANTIATIONS = {
    "gemm_tn_kernel<T>": "backward.hip launch_tn: if (!pl.ring) gemm_tn_kernel<T>",
    **{f"gemm_tn_ring_kernel<T,{a},{b},{k}>": f"backward.hip launch_tn: case {(a - 1) * 2 + b - 1}: "
       f"launch_tn_ring<T, {a}, {b}, {'true' if k == 'conv' else 'false'}>"
       for k in ("lin", "conv") for a in (1, 2) for b in (1, 2)},
    "tn_reduce_kernel": "backward.hip dfw_gemm_tn: if (splits > 1) tn_reduce_kernel",
}


def fwd_instantiations(name, case, tname):
    base, plus, _ = name.partition("+")
    base = base.replace(tname, "T", 1)
    if base.startswith("gemm_kernel") and case.res == "F32" and not plus:
        base = base[:-1] + ",RF32>"
    if base.startswith(("gemm_big_kernel", "conv_patch_kernel")) and case.out == "F32":
        base = base[:-1] + ",F32O>"
    return {base} | ({"splitk_reduce_kernel<T>"} if plus else set())


def tn_instantiations(name, tname):
    base, plus, _ = name.partition("+")
    return {base.replace(tname, "T", 1)} | ({"tn_reduce_kernel"} if plus else set())


def test_instantiation_lists_are_complete():
    assert len(FORWARD_INSTANTIATIONS) == 37 and len(TN_INSTANTIATIONS) == 10


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_every_case_plans_its_kernel_and_the_cases_reach_every_instantiation(hip_lib, monkeypatch, dtype):
    import ctypes as C
    from diffews_amd import _lib as L, ops, ops_bwd
    import test_gemm_plans_gpu as plans
    tname = plans.TNAME[dtype]
    lib = L.lib()
    names = []

    def plan_only(a, device):          # the arguments ops built, planned instead of launched
        buf = C.create_string_buffer(96)
        L.check(lib.dfw_gemm_kernel_name(C.byref(a), buf, 96), "dfw_gemm_kernel_name")
        names.append(buf.value.decode())

    monkeypatch.setattr(ops, "_gemm_call", plan_only)
    monkeypatch.setattr(ops_bwd, "_stream", lambda: None)
    monkeypatch.setattr(ops._Args, "device", lambda self: None)     # planning on host tensors: nothing is launched
    reached, wrong = set(), []
    for case in plans.FWD_CASES:
        names.clear()
        with plans.configured(L, case.cfg):
            try:
                plans.run_fwd(ops, case, plans.make_fwd_inputs(case, dtype, "cpu", fill=False))
            except RuntimeError as e:          # argument checks of the library
                names.append(str(e))
        want = plans.expected(case, dtype)
        if names != [want]:
            wrong.append((case.id, names, want))
            continue
        reached |= fwd_instantiations(want, case, tname)
    tn_reached = set()
    for case in plans.TN_CASES:
        with plans.tn_names(L, launch=False) as tn:
            try:
                plans.run_tn(ops_bwd, case, plans.make_tn_inputs(case, dtype, "cpu", fill=False))
            except RuntimeError as e:
                tn.append(str(e))
        want = plans.expected(case, dtype)
        if len(tn) != 1 or not plans.name_matches(tn[0], want):
            wrong.append((case.id, tn, want))
            continue
        tn_reached |= tn_instantiations(tn[0], tname)
    assert not wrong, "\n" + "\n".join(f"{cid}: planned {got}, expected {want}" for cid, got, want in wrong)
    fwd_all, tn_all = set(FORWARD_INSTANTIATIONS), set(TN_INSTANTIATIONS)
    assert reached == fwd_all, (fwd_all - reached, reached - fwd_all)
    assert tn_reached == tn_all, (tn_all - tn_reached, tn_reached - tn_all)
    # every persistent kernel walks several tiles per workgroup in at least one case: grids are capped at 256
    # workgroups, gemm_kernel's at 256 x its residency (2 for 128 x 128, 3 for 128 x 64, 4 for 64 x 64)
    walks = set()
    for case in plans.FWD_CASES:
        want = plans.expected(case, dtype)
        M, N = plans.fwd_dims(case)[:2]
        bm, bn = plans.tile_of(want)
        tiles = -(-M // bm) * -(-N // bn)
        cap = 256 * {(128, 128): 2, (128, 64): 3, (64, 64): 4}[(bm, bn)] if want.startswith("gemm_kernel") else 256
        if case.op != "bmm" and tiles > cap:
            walks.add(want.split("<")[0])
    assert walks == {"gemm_kernel", "gemm_big_kernel", "gemm8_kernel", "conv_patch_kernel", "conv_patch8_kernel"}, walks
