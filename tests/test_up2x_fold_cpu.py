"""CPU tests (no GPU) of the folded nearest-2x upsample conv: the algebra of packing.fold_up2x, its pack order, the host-only
queries of dfw_conv_up2x, and that dfw_gemm's own plan of the unfolded (ups = 1) convs did not move.

Nearest-2x upsampling followed by a 3x3 conv (padding 1) equals, per output parity (py, px), a 2x2 conv on the
low-resolution input: tap (ty, tx) reads source pixel (y + ty - 1 + py, x + tx - 1 + px) with the sum of the 3x3 weights
w[ky][kx], ky in S(py, ty), kx in S(px, tx); S(0,0) = {0}, S(0,1) = {1,2}, S(1,0) = {0,1}, S(1,1) = {2}."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from diffews_amd import packing

S = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}     # the tap sets S(parity, tap), restated here (not imported)
F64 = torch.float64


def folded_conv(x, wf, cout):
    """x [B, Cin, H, W] fp64, wf [Cout, 16*Cin] -> [B, Cout, 2H, 2W]: four 2x2 convs on x scattered to the parities."""
    B, cin, H, W = x.shape
    w = wf.view(cout, 2, 2, 2, 2, cin)
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros(B, cout, 2 * H, 2 * W)
    for py in range(2):
        for px in range(2):
            k = w[:, py, px].permute(0, 3, 1, 2)                     # [Cout, Cin, ty, tx]
            # source offset ty - 1 + py: the window of output (y, x) starts at padded (y + py, x + px)
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], k)
    return out


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 4)])
def test_fold_equals_upsample_then_conv(H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    B, cin, cout = 2, 3, 4
    x = torch.randn(B, cin, H, W, dtype=F64, generator=g)
    w = torch.randn(cout, cin, 3, 3, dtype=F64, generator=g)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    wf = packing.fold_up2x(packing.pack_conv3x3(w))
    assert wf.dtype == F64 and wf.shape == (cout, 16 * cin)
    got = folded_conv(x, wf, cout)
    err = (got - ref).abs().max() / ref.abs().max()
    assert err <= 1e-12, float(err)


def test_pack_order_is_parity_tap_channel():
    cout, cin = 2, 3
    for ky in range(3):
        for kx in range(3):
            w = torch.zeros(cout, cin, 3, 3)
            w[:, :, ky, kx] = torch.arange(1, cout * cin + 1, dtype=torch.float32).view(cout, cin)
            wf = packing.fold_up2x(packing.pack_conv3x3(w)).view(cout, 2, 2, 2, 2, cin)
            for py in range(2):
                for px in range(2):
                    for ty in range(2):
                        for tx in range(2):
                            want = w[:, :, ky, kx] if (ky in S[(py, ty)] and kx in S[(px, tx)]) else torch.zeros(cout, cin)
                            assert torch.equal(wf[:, py, px, ty, tx], want), (ky, kx, py, px, ty, tx)


def test_fold_sums_in_fp32_and_rounds_once():
    g = torch.Generator().manual_seed(7)
    w = torch.randn(4, 8, 3, 3, generator=g)
    wp = packing.pack_conv3x3(w)
    for dt in (torch.bfloat16, torch.float16):
        wf = packing.fold_up2x(wp, dt)
        assert wf.dtype == dt and wf.is_contiguous()
        assert torch.equal(wf, packing.fold_up2x(wp).to(dt))
        # corner slot (py, px, ty, tx) = (0, 0, 1, 1) holds the four-weight sum w[1,1] + w[1,2] + w[2,1] + w[2,2]
        four = (w[:, :, 1, 1].double() + w[:, :, 1, 2].double() + w[:, :, 2, 1].double() + w[:, :, 2, 2].double())
        got = wf.view(4, 2, 2, 2, 2, 8)[:, 0, 0, 1, 1].double()
        u = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11           # round to nearest at 8 / 11 significand bits
        mag = (w[:, :, 1, 1].abs() + w[:, :, 1, 2].abs() + w[:, :, 2, 1].abs() + w[:, :, 2, 2].abs()).double()
        assert ((got - four).abs() <= u * four.abs() + 2.0 ** -21 * mag).all()       # one storage rounding + three fp32 adds


# ------------------------------------------------------------------------------------------------ host queries

def _args(L, base, B=1, Hi=16, Wi=16, Cin=64, Cout=128, dtype=None, gn=0):
    a = L.ConvUp2xArgs()
    a.x = a.W = a.y = base
    a.x_elems, a.w_elems = B * Hi * Wi * Cin, Cout * 16 * Cin
    a.B, a.Hi, a.Wi, a.Cin, a.Cout, a.ldx, a.ldy = B, Hi, Wi, Cin, Cout, Cin, Cout
    a.dtype = L.BF16 if dtype is None else dtype
    a.gn_groups = gn
    return a


def _name(h, a):
    buf = C.create_string_buffer(b"untouched", 64)
    rc = h.dfw_conv_up2x_kernel_name(C.byref(a), buf, 64)
    return rc, buf.value.decode()


@pytest.fixture(scope="module")
def base():
    buf = C.create_string_buffer(4096)
    yield (C.addressof(buf) + 255) & ~255
    del buf


def test_queries_on_eligible_shapes(hip_lib, base):
    from diffews_amd import _lib as L
    assert hip_lib.dfw_version() >= 111
    assert _name(hip_lib, _args(L, base)) == (0, "gemm8_kernel<bf16,256,128,64,up2x>")
    assert _name(hip_lib, _args(L, base, B=2, Wi=32, Cin=128, Cout=256, dtype=L.F16)) == (0, "gemm8_kernel<f16,256,256,64,up2x>")
    assert _name(hip_lib, _args(L, base, Hi=32, Cout=192)) == (0, "gemm8_kernel<bf16,256,128,64,up2x>")
    # the model's shapes: VAE decoder 256^2 -> 512^2, UNet 32^2 -> 64^2
    assert _name(hip_lib, _args(L, base, B=4, Hi=256, Wi=256, Cin=256, Cout=256))[1] == "gemm8_kernel<bf16,256,256,64,up2x>"
    assert _name(hip_lib, _args(L, base, B=8, Hi=32, Wi=32, Cin=640, Cout=640))[1] == "gemm8_kernel<bf16,256,128,64,up2x>"
    # chunks = 4 parities x low-resolution tiles x wave rows (2 on the 256-wide tile, 4 on the 128-wide one)
    assert hip_lib.dfw_conv_up2x_gn_chunks(C.byref(_args(L, base, gn=32))) == 4 * 1 * 4
    assert hip_lib.dfw_conv_up2x_gn_chunks(C.byref(_args(L, base, B=2, Wi=32, Cin=128, Cout=256, gn=32))) == 4 * 2 * 2
    assert hip_lib.dfw_conv_up2x_gn_chunks(C.byref(_args(L, base, B=4, Hi=256, Wi=256, Cin=256, Cout=256, gn=32))) == 4 * 256 * 2
    assert hip_lib.dfw_conv_up2x_gn_chunks(C.byref(_args(L, base, gn=0))) == 0
    assert hip_lib.dfw_conv_up2x_gn_chunks(C.byref(_args(L, base, gn=1))) == 0        # 128 channels per group: not inside a wave tile
    assert hip_lib.dfw_conv_up2x_gn_chunks(C.byref(_args(L, base, gn=3))) == 0


@pytest.mark.parametrize("kw", [dict(Hi=8), dict(Wi=24), dict(Cin=32, ldx=64), dict(Cin=96), dict(Cout=32), dict(Cout=160), dict(ldx=68),
                                dict(ldy=132), dict(ldy=64)])
def test_ineligible_shapes_are_eshape_everywhere(hip_lib, base, kw):
    from diffews_amd import _lib as L
    ld = {k: kw.pop(k) for k in ("ldx", "ldy") if k in kw}
    a = _args(L, base, **kw)
    for k, v in ld.items():
        setattr(a, k, v)
    a.x_elems, a.w_elems = 1 << 24, 1 << 24
    assert _name(hip_lib, a) == (-2, "")
    assert hip_lib.dfw_conv_up2x(C.byref(a), None) == -2                               # rejected before any launch
    a.gn_groups = 32
    assert hip_lib.dfw_conv_up2x_gn_chunks(C.byref(a)) == 0


def test_null_misaligned_and_short_arguments_are_rejected(hip_lib, base):
    from diffews_amd import _lib as L
    assert hip_lib.dfw_conv_up2x(None, None) == -1
    assert hip_lib.dfw_conv_up2x_gn_chunks(None) == 0
    assert hip_lib.dfw_conv_up2x_kernel_name(C.byref(_args(L, base)), None, 64) == -1
    buf = C.create_string_buffer(64)
    assert hip_lib.dfw_conv_up2x_kernel_name(None, buf, 64) == -1
    for field in ("x", "W", "y"):
        a = _args(L, base)
        setattr(a, field, None)
        assert _name(hip_lib, a) == (-1, "") and hip_lib.dfw_conv_up2x(C.byref(a), None) == -1, field
        a = _args(L, base)
        setattr(a, field, base + 8)
        assert _name(hip_lib, a) == (-2, "") and hip_lib.dfw_conv_up2x(C.byref(a), None) == -2, field
    for field in ("B", "Hi", "Wi", "Cin", "Cout", "x_elems", "w_elems"):
        a = _args(L, base)
        setattr(a, field, 0)
        assert hip_lib.dfw_conv_up2x(C.byref(a), None) == -1, field
    a = _args(L, base)
    a.dtype = 2
    assert hip_lib.dfw_conv_up2x(C.byref(a), None) == -1
    a = _args(L, base)
    a.x_elems -= 1                                                                     # x shorter than B x Hi x Wi x Cin
    assert hip_lib.dfw_conv_up2x(C.byref(a), None) == -1
    a = _args(L, base)
    a.w_elems = 128 * 9 * 64                                                           # the unfolded pack is too short
    assert hip_lib.dfw_conv_up2x(C.byref(a), None) == -1
    a = _args(L, base)
    a.x_elems = 1 << 30                                                                # 2 GiB of 16-bit elements
    assert hip_lib.dfw_conv_up2x(C.byref(a), None) == -3
    a = _args(L, base, gn=1)
    a.gn_partial = base                                                                # sums asked for groups the kernel cannot emit
    assert hip_lib.dfw_conv_up2x(C.byref(a), None) == -2
    a = _args(L, base)
    a.gn_partial = base                                                                # a buffer without a group count
    assert hip_lib.dfw_conv_up2x(C.byref(a), None) == -1


# ------------------------------------------------------------------------------------------------ dfw_gemm's plan stays

@pytest.mark.parametrize("shape,want", [
    ((4, 256, 256, 256, 256, 32), ("gemm8_kernel<bf16,256,256,64,conv>", 2048, 0)),        # VAE decoder 256^2 -> 512^2
    ((8, 32, 32, 640, 640, 0), ("gemm8_kernel<bf16,256,128,64,conv>", 0, 0)),              # UNet 32^2 -> 64^2
    ((8, 8, 8, 1280, 1280, 0), ("gemm_kernel<bf16,128,128,conv>+splitk", 0, 20971520)),    # UNet 8^2 -> 16^2 (stays unfolded)
])
def test_dfw_gemm_plans_of_the_ups_rows_are_unchanged(hip_lib, base, shape, want):
    """Kernel name, GroupNorm chunk count and split-K workspace bytes of the unfolded route, as the library answered before the
    fold had an entry point (next to tests/test_gemm_plan_goldens_cpu.py's grid)."""
    from diffews_amd import _lib as L
    L.configure()
    B, Hi, Wi, Cin, Cout, gn = shape
    a = L.GemmArgs()
    a.A = a.W = a.C = base
    Ho, Wo = 2 * Hi, 2 * Wi
    a.a_elems, a.w_elems = B * Hi * Wi * Cin, Cout * 9 * Cin
    a.M, a.N, a.K, a.lda, a.ldc = B * Ho * Wo, Cout, 9 * Cin, Cin, Cout
    a.taps, a.Cin, a.Hi, a.Wi, a.Ho, a.Wo = 9, Cin, Hi, Wi, Ho, Wo
    a.stride, a.pad, a.ups, a.rows_per_img = 1, 1, 1, Ho * Wo
    a.out_scale, a.batch, a.dtype, a.gn_groups = 1.0, 1, L.BF16, gn
    buf = C.create_string_buffer(64)
    assert hip_lib.dfw_gemm_kernel_name(C.byref(a), buf, 64) == 0
    got = (buf.value.decode(), hip_lib.dfw_gemm_gn_chunks(C.byref(a)), hip_lib.dfw_gemm_workspace_bytes(C.byref(a)))
    assert got == want
