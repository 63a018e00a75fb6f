"""CPU tests (no GPU) behind tests/test_boundary_plans_gpu.py and tests/test_glue_exact_gpu.py.

* Every case of the boundary-conv table plans the kernel, grid, `iters` and fused-sum chunk count that a Python
  restatement of dfw_conv_small's dispatch rule predicts (through the host-only queries dfw_conv_small_kernel_name and
  dfw_conv_small_gn_chunks), and together the cases reach every kernel x taps x output mode the dispatcher can produce,
  iters in {1, 2 .. 7, 8}, a last workgroup that leaves the pixel-group loop early and a partly live 128-channel block.
* An emulation of conv_small8w_kernel (the fp32 FMA chain of one thread, rounding to the storage dtype, the per-thread and
  LDS fold order of the fused GroupNorm sums) lies inside the per-element bound and inside the sum tolerance.
* Faults injected into that emulation, each confined to one 8-pixel group or one workgroup, pass the assertions the suite
  had (relative L2 of the whole tensor) and fail the new checks at the right place.
* The segmentation reference of the exhaustive GPU test equals the kernel's fp32 expression for all 2^24 byte triples.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_bound as eb
import test_boundary_plans_gpu as bp

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
DTYPES = [BF16, F16]


# ------------------------------------------------------------------------------------------------ the dispatch rule

def predict(case, gn_groups=None):
    """dfw_conv_small's rule restated: -> (kernel, iters, 'GXxGY', fused-sum chunks per image)."""
    B, H, W, Cout, K = case.batch, case.H, case.W, case.Cout, case.taps * case.Cin
    pix = B * H * W
    aligned, nhwc = not case.misalign, case.mode in ("T", "F32")
    gn = (case.gn if case.mode == "T" else 0) if gn_groups is None else gn_groups
    if W % 8 == 0 and aligned and nhwc and Cout % 8 == 0 and K <= 72:
        cblocks, groups16 = -(-Cout // 128), -(-(pix // 8) // 16)
        iters = min(max(groups16 * cblocks // 2048, 1), 8)
        chunks = 0
        if gn > 0 and case.mode == "T" and Cout % 128 == 0 and Cout % gn == 0 and 128 % (Cout // gn) == 0:
            per_img, per_blk = H * (W // 8), 16 * iters
            chunks = per_img // per_blk if per_img % per_blk == 0 else 0
        return f"conv_small8w_kernel<{case.taps}>", iters, f"{-(-groups16 // iters)}x{cblocks}", chunks
    if W % 4 == 0 and aligned:
        return "conv_small4_kernel", 1, f"{(pix // 4 + 255) // 256}x{-(-Cout // 8)}", 0
    return "conv_small_kernel", 1, f"{(pix + 255) // 256}x{-(-Cout // 8)}", 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_every_case_plans_what_the_restated_rule_predicts(hip_lib, dtype):
    from diffews_amd import _lib as L
    wrong = [(c.id, bp.planned(c, dtype, L), predict(c)) for c in bp.CASES if bp.planned(c, dtype, L) != predict(c)]
    assert not wrong, "\n" + "\n".join(f"{cid}: planned {got}, predicted {want}" for cid, got, want in wrong)


def test_ids_are_unique():
    assert len(bp.BY_ID) == len(bp.CASES)


def test_cases_reach_every_kernel_mode_and_loop_path():
    plans = {c.id: predict(c) for c in bp.CASES}
    reached = {(plans[c.id][0].split("<")[0], c.taps, c.mode) for c in bp.CASES}
    every = ({("conv_small8w_kernel", t, m) for t in (9, 1) for m in ("T", "F32")}
             | {(k, t, m) for k in ("conv_small4_kernel", "conv_small_kernel") for t in (9, 1) for m in ("T", "F32", "NCHW")})
    assert reached == every, (every - reached, reached - every)
    w8 = [c for c in bp.CASES if plans[c.id][0].startswith("conv_small8w")]
    iters = {plans[c.id][1] for c in w8}
    assert 1 in iters and 8 in iters and any(1 < i < 8 for i in iters), iters
    for taps in (9, 1):
        assert any(plans[c.id][1] > 1 for c in w8 if c.taps == taps), taps
    # the last workgroup leaves the `it` loop early: whole iterations beyond nq, and an iteration that is partly live
    nq = lambda c: c.batch * c.H * (c.W // 8)
    assert any(plans[c.id][1] > 1 and nq(c) % (16 * plans[c.id][1]) != 0 and nq(c) % 16 != 0 for c in w8)
    assert any(nq(c) < 16 for c in w8)                                        # pixel-group rows of the workgroup idle
    # a 128-channel block that is only partly inside Cout, for NHWC storage and fp32 output; one live octet of 16
    assert {c.mode for c in w8 if c.Cout % 128 == 64 and c.Cout > 128} == {"T", "F32"}
    assert any(c.Cout == 8 for c in w8)
    # the 4-wide kernel takes NCHW at W % 8 == 0, T / F32 only at W % 8 == 4; W = 4; the scalar kernel W % 4 != 0 and
    # a misaligned view of a W % 8 == 0 input
    w4 = [c for c in bp.CASES if plans[c.id][0] == "conv_small4_kernel"]
    sc = [c for c in bp.CASES if plans[c.id][0] == "conv_small_kernel"]
    assert any(c.mode == "NCHW" and c.W % 8 == 0 for c in w4) and any(c.W == 4 for c in w4)
    assert all(c.W % 8 == 4 for c in w4 if c.mode != "NCHW")
    assert any(c.misalign and c.W % 8 == 0 for c in sc) and {c.W % 4 for c in sc if not c.misalign} >= {1, 2}
    assert any(c.W == 8 for c in w8) and any(c.H == 1 for c in w8) and any(c.H == 1 for c in sc)
    # channel counts, bias, sources, destinations
    assert {c.Cin for c in bp.CASES} >= {1, 3, 4, 5, 8} and {c.Cout for c in bp.CASES} >= {3, 4, 8, 64, 128, 320, 512}
    assert any(not c.bias for c in w8) and any(not c.bias for c in w4) and any(not c.bias for c in sc)
    for group in (w8, w4, sc):
        assert any(isinstance(c.B, tuple) for c in group)
    assert {len(c.B) for c in bp.CASES if isinstance(c.B, tuple)} == {2, 3}
    for c in bp.CASES:
        if isinstance(c.B, tuple):     # unequal batch sizes; a source boundary inside a workgroup's pixel range
            assert len(set(c.B)) > 1
            if c.gn:                   # (with fused sums a workgroup never straddles images)
                continue
            per_wg = {"conv_small8w_kernel": 128 * plans[c.id][1], "conv_small4_kernel": 1024, "conv_small_kernel": 256}
            assert (c.B[0] * c.H * c.W) % per_wg[plans[c.id][0].split("<")[0]] != 0, c.id
    nchw = [c for c in bp.CASES if c.mode == "NCHW"]
    assert {c.Cout for c in nchw} >= {3, 4, 8} and any(c.wide and c.batch == 1 for c in nchw)
    assert any(c.wide and c.batch > 1 for c in nchw) and any(not c.wide for c in nchw)
    assert {c.mode for c in bp.CASES if c.batch_slice} == {"T", "F32"}
    assert any(c.in_scale != 1 and c.out_scale != 1 for c in nchw) or (any(c.in_scale != 1 for c in nchw)
                                                                       and any(c.out_scale != 1 for c in nchw))
    # fused sums: iters 1 and > 1, several images, channels per group 4, 8, 16, a slice of a larger buffer, a shape that
    # must give none
    gn = [c for c in bp.CASES if c.gn]
    assert {plans[c.id][1] > 1 for c in gn if plans[c.id][3] > 0} == {True, False}
    assert {c.Cout // c.gn for c in gn if plans[c.id][3] > 0} >= {4, 8, 16}
    assert any(c.gn_slice and c.batch > 1 and plans[c.id][1] > 1 for c in gn)
    assert any(plans[c.id][3] == 0 for c in gn) and all(c.batch > 1 for c in gn if plans[c.id][3] == 0)
    # the product's own shapes
    shapes = {(c.batch, c.Cin, c.H, c.W, c.Cout, c.taps, c.mode) for c in bp.CASES}
    for s in [(1, 3, 512, 512, 128, 9, "T"), (4, 3, 512, 512, 128, 9, "T"), (2, 4, 64, 64, 512, 9, "T"),
              (16, 4, 64, 64, 320, 9, "T"), (16, 8, 64, 64, 320, 9, "F32"), (4, 8, 64, 64, 4, 1, "NCHW"),
              (2, 4, 64, 64, 4, 1, "NCHW"), (2, 4, 64, 64, 320, 9, "T"), (3, 4, 48, 48, 320, 9, "T"),
              (2, 8, 40, 64, 320, 9, "F32")]:
        assert s in shapes, s


def test_gn_chunk_query_for_shapes_outside_the_table(hip_lib):
    """dfw_conv_small_gn_chunks against the restated rule where the table has no case: channels per group that do not
    divide 128, Cout % 128 != 0, fp32 / NCHW output, a 4-wide shape."""
    from diffews_amd import _lib as L
    import ctypes as C
    for kw, gn in [(dict(Cout=384, H=16, W=16), 32), (dict(Cout=320, H=16, W=16), 32), (dict(Cout=128, H=16, W=16, mode="F32"), 32),
                   (dict(Cout=128, H=16, W=12), 32), (dict(Cout=128, H=16, W=16), 32), (dict(Cout=128, H=16, W=16), 128),
                   (dict(Cout=256, H=2, W=64), 2)]:
        c = bp.Cs("probe", 2, 3, kw["H"], kw["W"], kw["Cout"], mode=kw.get("mode", "T"), gn=gn)
        a = bp.args_of(c, BF16, L)
        a.gn_groups = gn
        assert L.lib().dfw_conv_small_gn_chunks(C.byref(a)) == predict(c, gn_groups=gn)[3], kw


# ------------------------------------------------------------------------------------------------ kernel emulation

def fma_chain(win, w, taps):
    """The accumulators of conv_small8w_kernel: win = the scaled, zero-padded fp32 input window [B, Cin, H + 2p, W + 2p],
    w fp32 [Cout, taps, Cin] -> fp32 [B, H, W, Cout], one fused multiply-add per (ky, c, kx) in the kernel's order (a row
    outside the image is skipped there and adds an exact zero here).  The FMA is evaluated in fp64 (the product of two
    fp32 numbers is exact there) and rounded to fp32."""
    k = 3 if taps == 9 else 1
    B, Cin, Hp, Wp = win.shape
    H, W = Hp - (k - 1), Wp - (k - 1)
    acc = torch.zeros(B, H, W, w.shape[0], dtype=F32)
    for ky in range(k):
        for c in range(Cin):
            for kx in range(k):
                col = win[:, c, ky:ky + H, kx:kx + W].to(F64)[..., None]
                acc = (col * w[:, ky * k + kx, c].to(F64) + acc.to(F64)).to(F32)
    return acc


def emulate(x, w, bias, taps, in_scale, out_scale, fault=None):
    """conv_small8w_kernel's fp32 result before the store [B, H, W, Cout].  fault = (kind, b, y, x0): the 8-pixel group
    at (image b, row y, columns x0 .. x0 + 7) computes with 'right_halo' dropped (as if `x0 + 8 < W` were false) or with
    'left_unscaled' (in_scale not applied to the left-halo scalar)."""
    p = 1 if taps == 9 else 0
    xin = x * torch.tensor(in_scale, dtype=F32)                       # one fp32 rounding, as in the kernel
    win = F.pad(xin, (p, p, p, p))
    acc = fma_chain(win, w, taps)
    if fault is not None:
        kind, b, y, x0 = fault
        assert taps == 9 and 0 < x0 and x0 + 8 < x.shape[3]
        g = win[b:b + 1, :, y:y + 3, x0:x0 + 10].clone()
        if kind == "right_halo":
            g[..., 9] = 0.0
        else:
            assert kind == "left_unscaled" and in_scale != 1.0
            g[..., 0] = F.pad(x, (p, p, p, p))[b, :, y:y + 3, x0]
        acc[b, y, x0:x0 + 8] = fma_chain(g, w, taps)[0, 0]
    bs = bias if bias is not None else torch.zeros(w.shape[0])
    return (acc + bs) * torch.tensor(out_scale, dtype=F32)


def emulate_sums(y, groups, iters, chunk_as_if_iters_1=None):
    """conv_small8w_kernel's fused GroupNorm sums of the stored NHWC y [B, H, W, N] -> fp32 [B, chunks, groups, 2]: each
    thread adds its 8 pixels x iters pixel groups in order (the squares by FMA), then one thread per group folds the 16
    pixel-group rows x its channels from LDS in order.  chunk_as_if_iters_1 = (b, c): workgroup c of image b computes its
    slot as if iters were 1 (slot c * iters): its own slot keeps the buffer's previous content (zero here)."""
    B, H, W, N = y.shape
    per_img, per_blk = H * (W // 8), 16 * iters
    assert per_img % per_blk == 0
    chunks, cpg = per_img // per_blk, N // groups
    r = y.to(F32).reshape(B, chunks, iters, 16, 8, N)                 # [image, chunk, it, pixel-group row, pixel, channel]
    gsum = torch.zeros(B, chunks, 16, N, dtype=F32)
    gsq = torch.zeros(B, chunks, 16, N, dtype=F32)
    for it in range(iters):
        for px in range(8):
            v = r[:, :, it, :, px]
            gsum = gsum + v
            gsq = (v.to(F64) * v.to(F64) + gsq.to(F64)).to(F32)
    gsum, gsq = gsum.view(B, chunks, 16, groups, cpg), gsq.view(B, chunks, 16, groups, cpg)
    a, a2 = torch.zeros(B, chunks, groups, dtype=F32), torch.zeros(B, chunks, groups, dtype=F32)
    for g2 in range(16):
        for c in range(cpg):
            a, a2 = a + gsum[:, :, g2, :, c], a2 + gsq[:, :, g2, :, c]
    part = torch.stack([a, a2], -1)
    if chunk_as_if_iters_1 is not None:
        b, c = chunk_as_if_iters_1
        assert iters > 1 and 0 < c * iters < chunks
        mine = part[b, c].clone()
        part[b, c] = 0.0
        part[b, c * iters] = mine
    return part


def cpu_inputs(case):
    xs, w, bias = bp.make_inputs(case, 1000 + bp.CASES.index(case), device="cpu")
    return torch.cat(xs), w, bias


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("cid", ["w8_c128", "t1_T", "w8_h1", "src3_gn", "src3_8w_f32"])
def test_emulation_of_the_8_wide_kernel_is_inside_the_bound(cid, dtype):
    case = bp.BY_ID[cid]
    assert predict(case)[0].startswith("conv_small8w")
    x, w, bias = cpu_inputs(case)
    v = emulate(x, w, bias, case.taps, case.in_scale, case.out_scale)
    out_dtype = dtype if case.mode == "T" else F32
    r, e = eb.conv_small_ref(x, w, bias, case.taps, case.in_scale, case.out_scale)
    worst = eb.check(v.to(out_dtype), r, e, out_dtype, where=eb.Where(case.Cout, case.H * case.W, case.W), label=cid)
    assert worst <= 1.0
    # the reference itself: torch's fp64 convolution of the same operands
    k = 3 if case.taps == 9 else 1
    w4 = w.view(case.Cout, k, k, case.Cin).permute(0, 3, 1, 2).double()
    lib = F.conv2d(x.double() * case.in_scale, w4, None if bias is None else bias.double(), padding=k // 2) * case.out_scale
    assert float((lib.permute(0, 2, 3, 1).reshape(r.shape) - r).abs().max()) < 1e-12
    if case.gn and case.mode == "T":
        _, iters, _, chunks = predict(case)
        assert chunks > 0
        y = v.to(dtype)
        assert eb.cs_chunk_check(y, emulate_sums(y, case.gn, iters), case.gn, iters, label=cid) <= 1.0


@pytest.fixture(scope="module")
def halo_fault_data():
    """The case with the most pixels (2^21: iters 8) and in_scale != 1: the emulated fp32 result, correct and with each
    fault in one pixel group, the fp64 reference, and the library convolution the old assertion compared with."""
    case = bp.BY_ID["it8_c8"]
    assert case.taps == 9 and case.in_scale == 0.5 and case.out_scale == 2.0 and predict(case)[1] == 8
    x, w, bias = cpu_inputs(case)
    b, y, x0 = 5, 301, 208                                                      # pixel group 26 of row 301, image 5
    good = emulate(x, w, bias, 9, case.in_scale, case.out_scale)
    bad = {}
    for kind in ("right_halo", "left_unscaled"):
        g = good.clone()
        sub = emulate(x[b:b + 1, :, y - 1:y + 2], w, bias, 9, case.in_scale, case.out_scale, fault=(kind, 0, 1, x0))
        g[b, y] = sub[0, 1]
        assert int((g != good).flatten(0, 2).any(-1).sum()) == 1                # one pixel of one group differs
        bad[kind] = g
    # the row's other pixels came out of the sub-problem unchanged
    w4 = w.view(case.Cout, 3, 3, case.Cin).permute(0, 3, 1, 2).contiguous()
    old_ref = F.conv2d(x * 0.5, w4, bias, padding=1) * 2.0                      # test_conv_small's reference
    refs = [eb.conv_small_ref(x[i:i + 1], w, bias, 9, case.in_scale, case.out_scale) for i in range(case.batch)]
    return case, good, bad, old_ref, refs, (b, y, x0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("kind,px", [("right_halo", 7), ("left_unscaled", 0)])
def test_halo_fault_in_one_pixel_group_passes_global_l2_and_fails_per_element(halo_fault_data, kind, px, dtype):
    from test_ops_gpu import TOL, rel
    case, good, bad, old_ref, refs, (b, y, x0) = halo_fault_data
    where = eb.Where(case.Cout, case.H * case.W, case.W)
    yg, yb = good.to(dtype), bad[kind].to(dtype)
    for i, (r, e) in enumerate(refs):
        assert eb.check(yg[i], r, e, dtype, where=where, label="no fault") <= 1.0
    assert rel(yg.permute(0, 3, 1, 2), old_ref) < TOL[dtype]
    assert rel(yb.permute(0, 3, 1, 2), old_ref) < TOL[dtype], rel(yb.permute(0, 3, 1, 2), old_ref)     # the gap
    for i, (r, e) in enumerate(refs):
        if i != b:
            assert eb.check(yb[i], r, e, dtype, where=where) <= 1.0
    with pytest.raises(AssertionError, match=rf"image 0 pixel \({y},{x0 + px}\)"):
        eb.check(yb[b], *refs[b], dtype, where=where, label=kind)
    # ... and only there
    r, e = refs[b]
    ratio = ((yb[b].double().reshape(r.shape) - r).abs() / (eb.U[dtype] * r.abs() + e + eb.FLOOR[dtype])).view(case.H, case.W, -1)
    outside = torch.nonzero(ratio.amax(-1) > 1.0).tolist()
    assert outside == [[y, x0 + px]], outside


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_chunk_index_fault_passes_groupnorm_comparison_and_fails_the_sum_check(dtype):
    """conv_small8w's `chunk` computed as if iters == 1, in one workgroup of the VAE encoder's conv_in at 512 x 512, B = 4
    (iters 4, 512 chunks per image).  The stored tensor here is the library convolution rounded to the storage dtype: the
    sum check concerns sums of whatever was stored.  Old assertion: groupnorm with the fused sums ~ groupnorm with its own
    statistics pass, rel < 1e-3 over the whole tensor (test_conv_small_fused_groupnorm_stats)."""
    from test_ops_gpu import rel
    case = bp.BY_ID["vae_in_b4"]
    _, iters, _, chunks = predict(case)
    assert iters == 4 and chunks == 512 and case.gn == 32
    x, w, bias = cpu_inputs(case)
    w4 = w.view(case.Cout, 3, 3, case.Cin).permute(0, 3, 1, 2).contiguous()
    y = F.conv2d(x, w4, bias, padding=1).permute(0, 2, 3, 1).to(dtype).contiguous()
    good = emulate_sums(y, case.gn, iters)
    for i in range(case.batch):
        assert eb.cs_chunk_check(y[i:i + 1], good[i:i + 1], case.gn, iters, label="no fault") <= 1.0
    b, c = 2, 77
    bad = emulate_sums(y[b:b + 1], case.gn, iters, chunk_as_if_iters_1=(0, c))
    part = good.clone()
    part[b] = bad[0]
    assert int((part != good).any(-1).any(-1).sum()) == 2                       # slots c and c * iters of image b

    def groupnorm(img, p):          # GroupNorm + SiLU of one image from partial sums [chunks, groups, 2] (gamma 1, beta 0)
        n = img.shape[0] * img.shape[1] * (case.Cout // case.gn)
        s = p.double().sum(0)
        mean = s[:, 0] / n
        rstd = (s[:, 1] / n - mean * mean + 1e-6).rsqrt()
        v = (img.float().view(-1, case.gn, case.Cout // case.gn) - mean.float()[None, :, None]) * rstd.float()[None, :, None]
        return F.silu(v)
    plain = torch.stack([groupnorm(y[i], good[i]) for i in range(case.batch)])
    fused = plain.clone()
    fused[b] = groupnorm(y[b], part[b])
    assert not torch.equal(fused[b], plain[b])
    assert rel(fused, plain) < 1e-3, rel(fused, plain)                          # the gap
    with pytest.raises(AssertionError, match=rf"image {b}, chunk ({c}|{c * iters}) "):
        eb.cs_chunk_check(y, part, case.gn, iters, label="chunk index")
    for i in range(case.batch):
        if i != b:
            assert eb.cs_chunk_check(y[i:i + 1], part[i:i + 1], case.gn, iters) <= 1.0


# ------------------------------------------------------------------------------------------------ segmentation reference

def test_segmentation_reference_equals_the_kernel_expression_for_all_byte_triples():
    """seg_count_kernel decides `((lut[u0] + lut[u1]) + lut[u2]) / 3.0f > thr` with lut[b] = (float)b / 255.0f; the
    reference of tests/test_glue_exact_gpu.py decides torch's fp32 `mean(dim=1) > thr`.  Equal for all 2^24 triples, as
    values and as decisions at the thresholds the GPU test uses."""
    import test_glue_exact_gpu as glue
    planes = glue.triple_planes()
    lut = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    p = planes.numpy()
    kern = ((lut[p[0]] + lut[p[1]]) + lut[p[2]]) / np.float32(3.0)
    assert kern.dtype == np.float32
    mean = planes[None].float().div(255).mean(dim=1)[0].numpy()
    assert int((kern != mean).sum()) == 0
    m123 = np.float32(float(torch.tensor([10, 20, 30], dtype=torch.uint8).float().div(255).mean()))
    assert int((kern == m123).sum()) > 0                                        # a threshold some mean equals exactly
    for thr in [np.float32(0.25), np.float32(254.0) / np.float32(255.0) * np.float32(0.25), np.float32(0.5),
                np.float32(glue.F32_04), m123, np.float32(1 / 3), np.float32(85.0) / np.float32(255.0)]:
        assert int(((kern > thr) != (torch.from_numpy(mean) > float(thr)).numpy()).sum()) == 0
    # the counting form against the histc form of test_seg_postprocess_bit_exact on a small image
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 9, 7, generator=g) * 2.4 - 1.2
    gt = glue.gt_pattern((2, 9, 7))
    u8 = torch.from_numpy(glue.seg_u8_ref(x))
    got = glue.seg_counts_ref(u8, gt, 0.25)
    for b in range(2):
        pred = u8[b].float().div(255)[None]
        pm = (pred.mean(dim=1) > pred.max() * 0.25).float()[0]
        g_ = gt[b].float()
        pm[g_ == 255] = 255
        inter = torch.histc(pm[pm == g_], bins=2, min=0, max=1)
        union = torch.histc(pm, bins=2, min=0, max=1) + torch.histc(g_, bins=2, min=0, max=1) - inter
        assert got[b] == [int(inter[0]), int(inter[1]), int(union[0]), int(union[1])]
    assert bool((gt == 255).any())
