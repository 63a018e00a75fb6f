"""Integer, rounding and layout kernels of csrc/misc.hip and csrc/backward.hip, compared exactly.

seg_postprocess (seg_u8_kernel, seg_count_kernel) and meter_update are integer work: bit-exact against a host restatement
at every quantisation boundary, for all 2^24 byte triples that decide `mean > thr`, on the scalar paths (H W % 4 != 0,
buffers that are not 4 / 16-byte aligned) and past both grid caps.  The conversions (to_storage, split_storage,
nchw_to_nhwc, loss_grad, to_f32) are one IEEE rounding each: bit-equal to torch's CPU conversion on every tie pattern of
every exponent, overflow, subnormals, the underflow threshold, signed zeros, infinities and NaN, and on a tensor long
enough for a second trip of the grid-stride loop.  transpose, concat_channels, slice_channels, zero_stuff2x, zeros,
linear_wt, conv3x3_wd and weight_relayout_batch move bits: equal to the torch expression at tile-edge shapes.
timestep_embedding is compared per element with the diffusers formula in fp64 within a derived bound.
tests/test_boundary_plans_cpu.py proves without a GPU that the segmentation reference used here agrees with the kernel's
fp32 expression for all 2^24 byte triples.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
TNAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
F32 = torch.float32
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FLOOR = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -25}
F32_04 = float(torch.tensor(0.4, dtype=F32))          # the fixed threshold travels as an fp32 number


@pytest.fixture(scope="module")
def env(hip_lib):
    from diffews_amd import ops, ops_bwd, _lib
    return ops, ops_bwd, _lib


# ------------------------------------------------------------------------------------------------ segmentation

def seg_u8_ref(x):
    """The host restatement of test_seg_postprocess_bit_exact: fp32 x [B, 3, H, W] -> uint8 numpy."""
    return ((x.clip(-1, 1) * 0.5 + 0.5) * 255).clip(0, 255).numpy().astype(np.uint8)


def seg_counts_ref(u8, gt, r_threshold=0.25, threshold=0.0, batch_max=False):
    """uint8 image(s) [B, 3, H, W] (tensor) + gt [B, H, W] in {0, 1, 255} -> [[inter0, inter1, union0, union1]] per image:
    to_tensor (byte / 255 in fp32), channel mean, `> max * r_threshold` (max per image or over the batch) or `> threshold`,
    ignore index 255 dropped from every histogram, union = pred + gt - inter (what the histc form of
    test_seg_postprocess_bit_exact counts, vectorised)."""
    pred = u8.float().div(255)
    mean = pred.mean(dim=1)
    if r_threshold > 0:
        mx = pred.max().expand(pred.shape[0]) if batch_max else pred.amax(dim=(1, 2, 3))
        pm = mean > (mx * r_threshold)[:, None, None]
    else:
        pm = mean > threshold
    valid = gt != 255
    out = []
    for b in range(u8.shape[0]):
        p, g, v = pm[b], gt[b] == 1, valid[b]
        cnt = lambda m: int((m & v).sum())
        i0, i1 = cnt(~p & ~g), cnt(p & g)
        out.append([i0, i1, cnt(~p) + cnt(~g) - i0, cnt(p) + cnt(g) - i1])
    return out


def triple_planes(limit=255):
    """uint8 [3, 4096, 4096]: pixel i holds the byte triple (i & 255, (i >> 8) & 255, i >> 16), each clipped to limit."""
    i = torch.arange(1 << 24, dtype=torch.int32)
    p = torch.stack([i & 255, (i >> 8) & 255, i >> 16]).clamp_(max=limit).to(torch.uint8)
    return p.view(3, 4096, 4096)


def bytes_to_x(u8):
    """fp32 values in the middle of each byte's quantisation interval."""
    return ((u8.double() + 0.5) / 255 * 2 - 1).float()


def gt_pattern(shape):
    i = torch.arange(math.prod(shape), dtype=torch.int64)
    g = (((i >> 3) ^ (i >> 11) ^ (i >> 17)) & 1).to(torch.uint8)
    g[i % 97 == 0] = 255
    return g.view(shape)


def test_seg_quantisation_boundaries(env):
    ops = env[0]
    b = torch.arange(0, 257, dtype=torch.float64)
    x0 = (b / 255 * 2 - 1).float()                                   # around the preimage of every b - 1 | b boundary
    vals = [x0]
    lo = hi = x0
    for _ in range(3):
        lo, hi = torch.nextafter(lo, torch.full_like(lo, -2)), torch.nextafter(hi, torch.full_like(hi, 2))
        vals += [lo, hi]
    extra = torch.tensor([-0.0, 0.0, 1.0, -1.0, 1.0000001, -1.0000001, 1.5, -1.5, 1e30, -1e30, math.inf, -math.inf,
                          1e-45, -1e-45, 0.999999, -0.999999], dtype=F32)
    v = torch.cat(vals + [extra])
    H, W = 25, 27                                                     # H W % 4 != 0: scalar path; 64 x 32: vector path
    for (h, w_) in [(H, W), (64, 32)]:
        n = 3 * h * w_
        x = v.repeat(-(-n // v.numel()))[:n].view(1, 3, h, w_).contiguous()
        u8, _ = ops.seg_postprocess(x.cuda())
        ref = seg_u8_ref(x)
        assert np.array_equal(u8.cpu().numpy(), ref), (h, w_)
        assert set(np.unique(ref).tolist()) == set(range(256))


def test_seg_counts_all_byte_triples(env):
    """One 4096 x 4096 image whose planes enumerate all 2^24 byte triples: every `mean > thr` decision the kernel can take."""
    ops = env[0]
    gt = gt_pattern((1, 4096, 4096))
    mean10_20_30 = float(torch.tensor([10, 20, 30], dtype=torch.uint8).float().div(255).mean())
    for limit, runs in [(255, [dict(r_threshold=0.25), dict(r_threshold=0.5), dict(r_threshold=0.0, threshold=F32_04),
                               dict(r_threshold=0.0, threshold=0.5), dict(r_threshold=0.0, threshold=mean10_20_30),
                               dict(r_threshold=0.0, threshold=float(torch.tensor(1 / 3, dtype=F32))),
                               dict(r_threshold=0.0, threshold=float(torch.tensor(85.0).div(255)))]),
                        (254, [dict(r_threshold=0.25)]), (129, [dict(r_threshold=0.25)]), (3, [dict(r_threshold=0.25)])]:
        planes = triple_planes(limit)[None]
        x = bytes_to_x(planes)
        xg, gg = x.cuda(), gt.cuda()
        for kw in runs:
            u8, counts = ops.seg_postprocess(xg, gg, **kw)
            assert torch.equal(u8.cpu(), planes), (limit, kw)
            assert int(u8.max()) == limit
            assert counts.cpu().tolist() == seg_counts_ref(planes, gt, **kw), (limit, kw)


@pytest.mark.parametrize("B,H,W", [(3, 7, 9), (4, 5, 5), (2, 512, 512), (3, 40, 56)], ids=lambda v: str(v))
def test_seg_scalar_paths_caps_and_gt_forms(env, B, H, W):
    """H W % 4 != 0 with B >= 3 (scalar loops; image bases of u8 / gt at odd offsets), 512 x 512 (past the 128- and
    64-block grid caps), gt with 255, all-255 gt, no gt, garbage in counts_out / scratch, batch_max with the maximum in the
    last image, and buffers that are not 4 / 16-byte aligned (the pointer halves of the vector-path conditions)."""
    ops = env[0]
    g = torch.Generator().manual_seed(B * 1000 + H)
    x = torch.rand(B, 3, H, W, generator=g) * 2.4 - 1.2
    for b in range(B - 1):
        x[b] *= 0.3 + 0.1 * b                                         # the batch maximum sits in the last image
    gt = gt_pattern((B, H, W))
    u8_ref = torch.from_numpy(seg_u8_ref(x))
    xg, gg = x.cuda(), gt.cuda()
    for kw in [dict(r_threshold=0.25), dict(r_threshold=0.25, batch_max=True), dict(r_threshold=0.0, threshold=F32_04)]:
        counts_out = torch.full((B, 4), -12345678901, dtype=torch.int64, device="cuda")
        scratch = torch.full((B,), 0x7fffffff, dtype=torch.int32, device="cuda")
        u8, counts = ops.seg_postprocess(xg, gg, counts_out=counts_out, scratch=scratch, **kw)
        assert torch.equal(u8.cpu(), u8_ref) and counts.data_ptr() == counts_out.data_ptr()
        assert counts.cpu().tolist() == seg_counts_ref(u8_ref, gt, **kw), kw
    assert int(u8_ref[-1].max()) > int(u8_ref[:-1].max())
    # all-255 gt: nothing counted; no gt: no counts, counts buffer never touched
    _, counts = ops.seg_postprocess(xg, torch.full_like(gg, 255))
    assert counts.cpu().tolist() == [[0, 0, 0, 0]] * B
    u8, none = ops.seg_postprocess(xg)
    assert none is None and torch.equal(u8.cpu(), u8_ref)
    # misaligned x (4 bytes), u8 (1 byte) and gt (1 byte) views
    n = x.numel()
    xb = torch.empty(n + 4, dtype=F32, device="cuda")
    xv = xb[1:n + 1].view(B, 3, H, W)
    xv.copy_(xg)
    ub = torch.full((n + 4,), 77, dtype=torch.uint8, device="cuda")
    gb = torch.empty(B * H * W + 4, dtype=torch.uint8, device="cuda")
    gv = gb[1:B * H * W + 1].view(B, H, W)
    gv.copy_(gg)
    assert xv.data_ptr() % 16 == 4 and gv.data_ptr() % 4 == 1
    u8, counts = ops.seg_postprocess(xv, gv, u8_out=ub[1:n + 1].view(B, 3, H, W))
    assert torch.equal(u8.cpu(), u8_ref) and int(ub[0]) == 77 and bool((ub[n + 1:] == 77).all())
    assert counts.cpu().tolist() == seg_counts_ref(u8_ref, gt)


@pytest.mark.parametrize("B,nclass", [(37, 5), (6, 1), (64, 20), (1, 3)])
def test_meter_update_exact(env, B, nclass):
    """Class ids -1 and nclass ignored, repeated ids, counts near 2^40, B not a multiple of 32, nclass = 1: int64-equal to
    index_add_ on the CPU."""
    ops = env[0]
    g = torch.Generator().manual_seed(B)
    counts = torch.randint((1 << 40) - 1000, (1 << 40) + 1000, (B, 4), generator=g, dtype=torch.int64)
    cls = torch.randint(-1, nclass + 1, (B,), generator=g, dtype=torch.int64)
    cls[0] = -1 if B > 1 else 0
    cls[-1] = nclass if B > 2 else cls[-1]
    ib = torch.randint(0, 1 << 33, (2, nclass), generator=g, dtype=torch.int64)
    ub = torch.randint(0, 1 << 33, (2, nclass), generator=g, dtype=torch.int64)
    ibg, ubg = ib.cuda(), ub.cuda()
    ops.meter_update(counts.cuda(), cls.cuda(), ibg, ubg)
    ok = (cls >= 0) & (cls < nclass)
    ib.index_add_(1, cls[ok], counts[ok, 0:2].t().contiguous())
    ub.index_add_(1, cls[ok], counts[ok, 2:4].t().contiguous())
    assert torch.equal(ibg.cpu(), ib) and torch.equal(ubg.cpu(), ub)
    assert int(ok.sum()) < B or B == 1


# ------------------------------------------------------------------------------------------------ conversions

def rounding_probe(dtype, n=1 << 18):
    """fp32 [n]: for every finite non-negative value v of `dtype` (all exponents, subnormals, zero, the largest finite):
    v, the midpoint of v and its successor (a tie; past the largest finite value: the overflow threshold) and the fp32
    neighbours of that midpoint, both signs; then 65504, 65519, 65520, 1e6, +-0, +-inf, NaN, fp32 subnormals; padded with
    normal random numbers."""
    top = 0x7C00 if dtype == torch.float16 else 0x7F80
    v = torch.arange(0, top, dtype=torch.int32).to(torch.int16).view(dtype).double()
    nxt = torch.cat([v[1:], (2 * v[-1] - v[-2])[None]])
    mid = ((v + nxt) / 2).float()
    assert bool((mid.double() == (v + nxt) / 2).all())               # every midpoint is an fp32 number
    inf = torch.full_like(mid, math.inf)
    pos = torch.cat([v.float(), mid, torch.nextafter(mid, -inf), torch.nextafter(mid, inf)])
    extra = torch.tensor([65504.0, 65519.0, 65520.0, 1e6, -1e6, 0.0, -0.0, math.inf, -math.inf, math.nan, 1e-45, -1e-45,
                          1e-40, 5.9e-8, 2.98e-8, 2.99e-8, 6.1e-5, 3.4e38, -3.4e38], dtype=F32)
    out = torch.cat([pos, -pos, extra])
    assert out.numel() <= n
    pad = torch.randn(n - out.numel(), generator=torch.Generator().manual_seed(7))
    return torch.cat([out, pad])


def assert_bits_equal(got, want, label, where=None):
    """16-bit or fp32 tensors equal bit for bit, NaNs compared by isnan (not by payload)."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, label
    it = torch.int16 if got.element_size() == 2 else torch.int32
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    same = (got.contiguous().view(it) == want.contiguous().view(it)) | (nan_g & nan_w)
    if where is not None:
        same = same | ~where
    if not bool(same.all()):
        idx = torch.nonzero(~same.flatten())[:6, 0].tolist()
        raise AssertionError(f"{label}: {int((~same).sum())} of {same.numel()} elements differ, first at {idx}: got "
                             f"{[float(got.flatten()[i]) for i in idx]} want {[float(want.flatten()[i]) for i in idx]}")


def is_f32_subnormal(x):
    return (x != 0) & (x.abs() < 2.0 ** -126)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_fp32_to_storage_roundings_exact(env, dtype):
    """to_storage, split_storage, nchw_to_nhwc and loss_grad round to nearest even exactly like torch's CPU conversion.
    bf16 subnormal outputs come from fp32-subnormal inputs; the kernels are compiled in hipcc's default mode, which keeps
    fp32 subnormals, so those are held to the same bit-equality (asserted separately so that a flush would be named)."""
    ops, ob, _ = env
    x = rounding_probe(dtype)
    sub = is_f32_subnormal(x)
    xg = x.cuda()
    want = x.to(dtype)
    y = ops.to_storage(xg, dtype)
    assert_bits_equal(y, want, "to_storage (normal fp32 inputs)", where=~sub)
    assert_bits_equal(y, want, "to_storage (fp32-subnormal inputs)", where=sub)
    hi, lo = ops.split_storage(xg, dtype)
    assert_bits_equal(hi, want, "split_storage hi (normal fp32 inputs)", where=~sub)
    assert_bits_equal(hi, want, "split_storage hi (fp32-subnormal inputs)", where=sub)
    fin = torch.isfinite(want.float())
    want_lo = (x - want.float()).to(dtype)
    lo_sub = is_f32_subnormal(x - want.float()) | sub
    assert_bits_equal(lo, want_lo, "split_storage lo (normal)", where=fin & ~lo_sub)
    assert_bits_equal(lo, want_lo, "split_storage lo (fp32-subnormal difference)", where=fin & lo_sub)
    # nchw_to_nhwc: [2, 4, 128, 256] -> [2, 128, 256, 8], channels 4 .. 7 zero; scale 1 and 0.5 (exact in fp32)
    x4 = x.view(2, 4, 128, 256)
    for scale in (1.0, 0.5):
        y = ob.nchw_to_nhwc(x4.cuda(), dtype, cp=8, scale=scale).cpu()
        w4 = (x4 * scale).to(dtype).permute(0, 2, 3, 1)
        s4 = is_f32_subnormal(x4 * scale).permute(0, 2, 3, 1) | sub.view(2, 4, 128, 256).permute(0, 2, 3, 1)
        assert_bits_equal(y[..., :4], w4, f"nchw_to_nhwc scale {scale} (normal)", where=~s4)
        assert_bits_equal(y[..., :4], w4, f"nchw_to_nhwc scale {scale} (fp32-subnormal)", where=s4)
        assert bool((y[..., 4:].view(torch.int16) == 0).all())
        # loss_grad: the same rounding into channels 0 .. 3 of a zeroed [B, H, W, 8] and back to fp32 NCHW
        nchw = torch.full((2, 4, 128, 256), 9.0, dtype=F32, device="cuda")
        d = ob.loss_grad(x4.cuda(), dtype, scale=scale, dpred_nchw_out=nchw).cpu()
        assert_bits_equal(d[..., :4], w4, f"loss_grad scale {scale} (normal)", where=~s4)
        assert_bits_equal(d[..., :4], w4, f"loss_grad scale {scale} (fp32-subnormal)", where=s4)
        assert bool((d[..., 4:].view(torch.int16) == 0).all())
        assert_bits_equal(nchw, d[..., :4].permute(0, 3, 1, 2).float().contiguous(), f"loss_grad nchw scale {scale}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_conversions_past_the_grid_cap(env, dtype):
    """n > 8192 x 256 x 8 elements: the grid-stride loops of convert_f32 / split_f32 / to_f32 take a second trip."""
    ops, ob, _ = env
    n = 8192 * 256 * 8 + 4096 + 8
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(n, generator=g, device="cuda") * 37.0
    want = x.cpu().to(dtype)
    y = ops.to_storage(x, dtype)
    assert_bits_equal(y, want, "to_storage")
    assert float(y[-1]) == float(want[-1])
    hi, lo = ops.split_storage(x, dtype)
    assert_bits_equal(hi, want, "split hi")
    assert_bits_equal(lo, (x.cpu() - want.float()).to(dtype), "split lo")
    out = torch.full((n,), 5.0, dtype=F32, device="cuda")
    ob.to_f32(y, out, scale=0.25)
    assert_bits_equal(out, want.float() * 0.25, "to_f32")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_storage_to_fp32_every_pattern(env, dtype):
    """to_f32: out = x.float() * scale in fp32 for all 65536 bit patterns of the storage dtype."""
    _, ob, _ = env
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    for scale in (1.0, 0.25, 1.0 / 3.0):
        out = torch.full((65536,), 5.0, dtype=F32, device="cuda")
        ob.to_f32(x.cuda(), out, scale=scale)
        want = x.float() * torch.tensor(scale, dtype=F32)
        sub = is_f32_subnormal(want)
        assert_bits_equal(out, want, f"to_f32 scale {scale} (normal results)", where=~sub)
        assert_bits_equal(out, want, f"to_f32 scale {scale} (fp32-subnormal results)", where=sub)


# ------------------------------------------------------------------------------------------------ layout kernels

def pattern16(shape, dtype, seed):
    """Distinct-looking 16-bit values (finite), so that a misplaced element shows."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_transpose_exact(env, dtype):
    ops = env[0]
    for R in (1, 63, 64, 65, 130):
        for Cc in (1, 63, 64, 65, 130):
            x = pattern16((3, R, Cc), dtype, R * 1000 + Cc)
            assert torch.equal(ops.transpose(x.cuda()).cpu(), x.transpose(1, 2).contiguous()), (R, Cc)


@pytest.mark.parametrize("dtype", DTYPES + [F32], ids=["bf16", "f16", "f32"])
def test_concat_slice_zero_stuff_exact(env, dtype):
    """concat_channels with Ca / 8 and Cb / 8 odd (16-bit) and as a byte copy of fp32 rows, with more 16-byte pieces than
    the 4096 x 256 threads of the capped grid; slice_channels and zero_stuff2x (16-bit only) likewise."""
    ops, ob, _ = env
    Ca, Cb = (12, 20) if dtype == F32 else (24, 40)
    for rows in (5, 140000):
        a, b = torch.randn(rows, Ca).to(dtype), torch.randn(rows, Cb).to(dtype)
        assert torch.equal(ops.concat_channels(a.cuda(), b.cuda()).cpu(), torch.cat([a, b], -1)), rows
    a4, b4 = torch.randn(2, 3, 5, Ca).to(dtype), torch.randn(2, 3, 5, Cb).to(dtype)
    assert torch.equal(ops.concat_channels(a4.cuda(), b4.cuda()).cpu(), torch.cat([a4, b4], -1))
    if dtype == F32:
        return
    for rows, lda, c0, Cc in [(7, 104, 24, 64), (140000, 104, 24, 64), (33, 64, 0, 64), (33, 64, 56, 8)]:
        a = pattern16((rows, lda), dtype, rows)
        assert torch.equal(ob.slice_channels(a.cuda(), c0, Cc).cpu(), a[:, c0:c0 + Cc].contiguous()), (rows, lda, c0, Cc)
    for B, H, W, Cc in [(3, 5, 7, 24), (2, 64, 64, 320), (1, 1, 1, 8)]:
        a = pattern16((B, H, W, Cc), dtype, H)
        want = torch.zeros(B, 2 * H, 2 * W, Cc, dtype=dtype)
        want[:, ::2, ::2] = a
        got = ob.zero_stuff2x(a.cuda()).cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (B, H, W, Cc)


def test_zero_fill_guards_and_cap(env):
    """dfw_zero on the middle of a sentinel-filled buffer (neighbours untouched), past the 4096 x 256 x 16-byte cap, and
    ops.zeros for sizes that need padding to 16 bytes."""
    ops, _, L = env
    for nbytes in (16, 4096 + 16, 4096 * 256 * 16 + 4096 + 16):
        buf = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        L.check(L.lib().dfw_zero(buf.data_ptr() + 32, nbytes, None), "dfw_zero")
        torch.cuda.synchronize()
        assert bool((buf[:32] == 0x5A).all()) and bool((buf[32 + nbytes:] == 0x5A).all()), nbytes
        assert int(buf[32:32 + nbytes].max()) == 0 and int(buf[32 + nbytes - 1]) == 0, nbytes
    for shape, dt in [((3, 5), torch.bfloat16), ((1,), F32), ((7, 3, 1), torch.int64), ((4096, 257, 5), torch.float16)]:
        z = ops.zeros(shape, dt)
        assert tuple(z.shape) == shape and z.dtype == dt and int((z != 0).sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_weight_relayouts_exact(env, dtype):
    """linear_wt (W^T), conv3x3_wd (W'[ci][8 - tap][co] = W[co][tap][ci]) and the one-launch table form for
    R, C in {8, 56, 64, 72, 136, 1288}."""
    _, ob, _ = env
    dims = (8, 56, 64, 72, 136, 1288)
    entries, wants = [], []
    for i, N in enumerate(dims):
        for j, K in enumerate(dims):
            w = pattern16((N, K), dtype, N * 10000 + K)
            assert torch.equal(ob.linear_wt(w.cuda()).cpu(), w.t().contiguous()), (N, K)
            if (i + j) % 3 == 0:
                entries.append(("T", w.cuda(), torch.zeros(K, N, dtype=dtype, device="cuda")))
                wants.append(w.t().contiguous())
    for cout, cin in [(8, 56), (56, 8), (64, 64), (72, 136), (136, 72), (1288, 8), (8, 1288), (320, 64)]:
        w = pattern16((cout, 9 * cin), dtype, cout * 7 + cin)
        want = w.view(cout, 9, cin).flip(1).permute(2, 1, 0).reshape(cin, 9 * cout).contiguous()
        assert torch.equal(ob.conv3x3_wd(w.cuda(), cout).cpu(), want), (cout, cin)
        entries.append(("D", w.cuda(), torch.zeros(cin, 9 * cout, dtype=dtype, device="cuda")))
        wants.append(want)
    table = ob.relayout_table(entries, "cuda")
    ob.weight_relayout_batch(table)
    for (kind, w, y), want in zip(entries, wants):
        assert torch.equal(y.cpu(), want), (kind, tuple(w.shape))


# ------------------------------------------------------------------------------------------------ timestep embedding

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_timestep_embedding_per_element(env, dtype):
    """Every element against the diffusers formula in fp64: with half = dim / 2 and d = half - freq_shift,
    a_j = -ln(10000) j / d, f_j = exp(a_j), emb[b] = [sin(t_b f), cos(t_b f)], halves swapped by flip_sin_to_cos.

    Bound  |y - r| <= u_T |r| + (|t f| (3 |ln f| + 5) + 4) 2^-24 + floor_T,  derived, not fitted.  Every fp32 rounding is
    taken at its worst relative size u = 2^-24, an `n ulp` library function at n 2^-23 = 2 n u:
      * the exponent argument -9.2103..f * (float)j / d carries three roundings (the constant, the product, the
        quotient): relative error 3 u, absolute 3 u |ln f|, which expf turns into a relative error 3 u |ln f| of f;
      * expf within 2 ulp: 4 u;   * the product t * f: u.     So arg = t f is off by at most |t f| (3 |ln f| + 5) u;
      * sin and cos have slope <= 1: the same absolute error in the result;   * sinf / cosf within 2 ulp of a value
        <= 1: 4 u.
    The rounding of the result to the 16-bit output is u_T |r|, which dominates; the test is there for flip, freq_shift,
    the half - shift divisor and the row / column indexing at B > 3."""
    ops = env[0]
    ts = [0.0, 0.5, 1.0, 500.0, 999.0]
    t = torch.tensor([ts[i % 5] for i in range(16)], dtype=F32)
    t[5:10] = torch.tensor([999.0, 0.5, 500.0, 0.0, 1.0])          # rows differ from their neighbours in any period
    worst = 0.0
    for dim in (32, 128, 320, 1280):
        for flip in (True, False):
            for shift in (0.0, 1.0):
                y = ops.timestep_embedding(t.cuda(), dim, dtype, flip_sin_to_cos=flip, freq_shift=shift).cpu().double()
                half = dim // 2
                a = -math.log(10000.0) * torch.arange(half, dtype=torch.float64) / (half - shift)
                arg = t.double()[:, None] * torch.exp(a)[None, :]
                sn, cs = torch.sin(arg), torch.cos(arg)
                r = torch.cat([cs, sn], -1) if flip else torch.cat([sn, cs], -1)
                e = (arg.abs() * (3 * a.abs()[None, :] + 5) + 4) * 2.0 ** -24
                bound = U[dtype] * r.abs() + torch.cat([e, e], -1) + FLOOR[dtype]
                ratio = (y - r).abs() / bound
                w = float(ratio.max())
                if not w <= 1.0:
                    b, j = [int(v) for v in torch.nonzero(ratio == ratio.max())[0]]
                    raise AssertionError(f"timestep_embedding dim {dim} flip {flip} shift {shift}: row {b} (t = {float(t[b])}), "
                                         f"column {j}: y = {float(y[b, j])}, ref = {float(r[b, j])}, ratio {w:.3g}")
                worst = max(worst, w)
    print(f"BNDRATIO timestep_embedding T {TNAME[dtype]} all {worst:.4f}")
