"""The staged epilogue of the persistent walks (conv_patch_kernel, conv_patch8_kernel, gemm8_kernel) with its operands present
and absent.

The epilogue loads bias and row bias once per tile and the residual one 32-row round ahead of its use, all through buffer
descriptors that are EMPTY for a null pointer, so that the same straight-line code serves every operand combination.  What
can go wrong: a null operand that does not read as zero, a residual taken from another round's rows, rows past M of a
ragged Linear tile.  The checks are exact where the arithmetic is the same by construction:

  * an absent residual and an all-zero residual give the same bits (x + 0.f either way); likewise an absent bias / row bias
    and zeros (the bias values here are never -0.f, the one value for which `b + 0.f` is not `b`);
  * the fused GroupNorm partial sums of those pairs are equal too;

and against an fp32 reference with test_ops_gpu.py's tolerance (output rounding + accumulation order) for the full
combination, on the first and last image: a residual fetched from the wrong round would be off by O(1).

Shapes: the smallest eligible ones (the *_eligible rules of the kernel files) at which a walk can go wrong: fewer workgroups
than CUs (192 tiles), a ragged second round (288 / 320), a third round (544), two n-tiles per m-tile (N = 512), the
256 x 160 tile, the up2x and gathering forms of gemm8_kernel, and Linear shapes with a ragged last m-tile.

The GEGLU epilogue, which dfw_gemm also accepts on a conv3x3, is checked on gemm8_kernel's conv forms (test_conv_geglu_epilogue).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = torch.bfloat16
TOL = 4e-3                     # test_ops_gpu.py's bf16 figure: output rounding 2^-9 (rms ~0.6x) + fp32 accumulation order


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


def _kernel_name(ops, fn):
    """Name of the GEMM kernel the library plans for the call made inside fn (as in test_ops_gpu.py)."""
    names = []
    ops.gemm_hook = lambda name, flops, e0, e1, shape=None: names.append(name)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops.gemm_hook = None
    return names


def _rand(shape, seed, scale=1.0, dtype=DT):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(dtype)


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _same(a, b):
    assert torch.equal(a, b)
    sa, sb = getattr(a, "_gn_stats", None), getattr(b, "_gn_stats", None)
    assert (sa is None) == (sb is None)
    if sa is not None:
        assert torch.equal(sa[0], sb[0])


CONV_CASES = [
    # kernel, images, H = W, Cin, Cout
    ("conv_patch_kernel<bf16,512,128>", 6, 128, 64, 128),      # 192 tiles: fewer workgroups than CUs
    ("conv_patch_kernel<bf16,512,128>", 9, 128, 64, 128),      # 288: ragged second round
    ("conv_patch_kernel<bf16,512,128>", 17, 128, 64, 128),     # 544: three rounds
    ("conv_patch8_kernel<bf16,256,256>", 12, 64, 64, 256),     # 192
    ("conv_patch8_kernel<bf16,256,256>", 20, 64, 64, 256),     # 320
    ("conv_patch8_kernel<bf16,256,256>", 10, 64, 64, 512),     # 320, ntn = 2
    ("conv_patch8_kernel<bf16,256,160>", 6, 64, 64, 320),      # 192 (10 channels per group: no fused sums)
    ("conv_patch8_kernel<bf16,256,160>", 10, 64, 64, 320),     # 320
    ("gemm8_kernel<bf16,256,256,64,conv>", 5, 256, 64, 256),   # stride 2: 320 tiles of the gathering form
]


@pytest.mark.parametrize("kernel,B,H,Cin,Cout", CONV_CASES)
def test_conv_epilogue_operands(ops, kernel, B, H, Cin, Cout):
    from diffews_amd.packing import pack_conv3x3
    stride = 2 if kernel.endswith("conv>") else 1
    Ho = H // stride
    x = _rand((B, H, H, Cin), 1)
    w4 = _rand((Cout, Cin, 3, 3), 2, (9 * Cin) ** -0.5)
    w = pack_conv3x3(w4.cpu()).cuda()
    bias, rb = _rand((Cout,), 3, dtype=torch.float32), _rand((B, Cout), 4, dtype=torch.float32)
    res = _rand((B, Ho, Ho, Cout), 5)
    conv = lambda **kw: ops.conv3x3(x, w, Cout, stride=stride, pad=1, gn_groups=32, **kw)
    out = []
    assert _kernel_name(ops, lambda: out.append(conv(bias=bias, rowbias=rb, residual=res, out_scale=0.5))) == [kernel]
    full = out[0]
    for i in {0, B - 1}:
        ref = F.conv2d(x[i:i + 1].float().permute(0, 3, 1, 2), w4.float(), bias, stride=stride, padding=1) + rb[i][None, :, None, None]
        ref = (ref.permute(0, 2, 3, 1) + res[i:i + 1].float()) * 0.5
        assert rel(full[i:i + 1], ref) < TOL
    zres, zb, zrb = torch.zeros_like(res), torch.zeros_like(bias), torch.zeros_like(rb)
    _same(conv(), conv(bias=zb, rowbias=zrb, residual=zres))
    _same(conv(bias=bias), conv(bias=bias, residual=zres))
    _same(conv(bias=bias, residual=res), conv(bias=bias, rowbias=zrb, residual=res))
    _same(conv(rowbias=rb, residual=res), conv(bias=zb, rowbias=rb, residual=res))
    plain = conv()
    ref0 = F.conv2d(x[:1].float().permute(0, 3, 1, 2), w4.float(), None, stride=stride, padding=1).permute(0, 2, 3, 1)
    assert rel(plain[:1], ref0) < TOL


def test_up2x_epilogue_operands(ops):
    """gemm8_kernel's up2x form (bias and fused sums only): 4 x 5 x 16 = 320 parity tiles, a ragged second round."""
    from diffews_amd.packing import fold_up2x, pack_conv3x3
    B, Hi, Cin, Cout = 5, 64, 64, 256
    x = _rand((B, Hi, Hi, Cin), 1)
    w4 = _rand((Cout, Cin, 3, 3), 2, (9 * Cin) ** -0.5)
    wp = pack_conv3x3(w4.cpu())
    wf, wp = fold_up2x(wp).cuda(), wp.cuda()
    bias = _rand((Cout,), 3, dtype=torch.float32)
    conv = lambda b: ops.conv3x3_stream(x, wp, Cout, bias=b, w_up2x=wf, ups=True, gn_groups=32)
    out = []
    assert _kernel_name(ops, lambda: out.append(conv(bias))) == ["gemm8_kernel<bf16,256,256,64,up2x>"]
    _same(conv(None), conv(torch.zeros_like(bias)))
    up = F.interpolate(x[-1:].float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    ref = F.conv2d(up, w4.float(), bias, padding=1).permute(0, 2, 3, 1)
    assert rel(out[0][-1:], ref) < 2 * TOL          # + the fold's one weight rounding (test_up2x_fold_gpu.py bounds it per element)


@pytest.mark.parametrize("M,N,K,kernel", [(50000, 512, 320, "gemm8_kernel<bf16,256,256,64,lin>"),      # 196 x 2 tiles, 80 rows in the last
                                          (33000, 320, 320, "gemm8_kernel<bf16,256,160,64,lin>"),      # 129 x 2, 232 rows in the last
                                          (49000, 384, 320, "gemm8_kernel<bf16,256,128,64,lin>")])     # 192 x 3, 104 rows in the last
def test_linear_epilogue_operands(ops, M, N, K, kernel):
    """gemm8_kernel's Linear form: rows past M of the last m-tile must not be read or stored (the output is allocated
    exactly, a canary row block behind the residual stays out of the result), operands absent == zeros."""
    x, w = _rand((M, K), 1), _rand((N, K), 2, K ** -0.5)
    bias = _rand((N,), 3, dtype=torch.float32)
    res_buf = _rand((M + 256, N), 4)
    res_buf[M:] = float("nan")                       # what a read past M would pick up
    res = res_buf[:M]
    out = []
    assert _kernel_name(ops, lambda: out.append(ops.linear(x, w, bias=bias, residual=res))) == [kernel]
    ref = x.float() @ w.float().t() + bias + res.float()
    assert rel(out[0], ref) < TOL
    assert torch.equal(ops.linear(x, w), ops.linear(x, w, bias=torch.zeros_like(bias), residual=torch.zeros_like(res)))
    assert torch.equal(ops.linear(x, w, bias=bias), ops.linear(x, w, bias=bias, residual=torch.zeros_like(res)))
    rpi = 1000
    rb = _rand(((M + rpi - 1) // rpi, N), 5, dtype=torch.float32)
    y = ops.linear(x, w, bias=bias, residual=res, rowbias=rb, rows_per_img=rpi)
    assert rel(y, ref + rb.repeat_interleave(rpi, 0)[:M]) < TOL


@pytest.mark.parametrize("B,H,Cin,Cout,stride,kernel", [(5, 256, 64, 256, 2, "gemm8_kernel<bf16,256,256,64,conv>"),     # 320 tiles, stride 2
                                                        (20, 64, 64, 256, 1, "gemm8_kernel<bf16,256,256,64,conv>"),     # what the patch kernels decline
                                                        (20, 64, 64, 384, 1, "gemm8_kernel<bf16,256,128,64,conv>")])    # 320 x 3 tiles of 256 x 128
def test_conv_geglu_epilogue(ops, B, H, Cin, Cout, stride, kernel):
    """dfw_gemm accepts GEGLU on a conv3x3 (taps = 9, no Python wrapper: called through the binding): the conv forms of
    gemm8_kernel must write the gated Cout / 2 columns (rows of ldc = Cout / 2) and nothing behind the last row.  W rows are
    interleaved in 64-row groups, 32 value rows then 32 gate rows; output column 32 g + c = (a + bias_a) * gelu(gate + bias_g)."""
    import ctypes as C
    from diffews_amd import _lib as L
    from diffews_amd.packing import pack_conv3x3
    Ho = H // stride
    M, half = B * Ho * Ho, Cout // 2
    x = _rand((B, H, H, Cin), 1)
    w4 = _rand((Cout, Cin, 3, 3), 2, (9 * Cin) ** -0.5)
    w = pack_conv3x3(w4.cpu()).cuda()
    bias = _rand((Cout,), 3, dtype=torch.float32)
    buf = torch.full((M + 64, half), 7.0, dtype=DT, device="cuda")          # 64 canary rows behind the output
    a = L.GemmArgs()
    a.A, a.W, a.C, a.bias = x.data_ptr(), w.data_ptr(), buf.data_ptr(), bias.data_ptr()
    a.a_elems, a.w_elems = x.numel(), w.numel()
    a.M, a.N, a.K, a.lda, a.ldc = M, Cout, 9 * Cin, Cin, half
    a.taps, a.Cin, a.Hi, a.Wi, a.Ho, a.Wo = 9, Cin, H, H, Ho, Ho
    a.stride, a.pad, a.rows_per_img = stride, 1, Ho * Ho
    a.out_scale, a.batch, a.dtype, a.geglu = 1.0, 1, L.BF16, 1
    name = C.create_string_buffer(64)
    L.check(L.lib().dfw_gemm_kernel_name(C.byref(a), name, 64), "dfw_gemm_kernel_name")
    assert name.value.decode() == kernel
    L.check(L.lib().dfw_gemm(C.byref(a), torch.cuda.current_stream().cuda_stream), "dfw_gemm")
    torch.cuda.synchronize()
    assert bool((buf[M:] == 7.0).all()), "rows behind the output were written"
    y = buf[:M].view(B, Ho, Ho, half)
    for i in {0, B - 1}:
        v = F.conv2d(x[i:i + 1].float().permute(0, 3, 1, 2), w4.float(), bias, stride=stride, padding=1).permute(0, 2, 3, 1)
        v = v.reshape(Ho, Ho, Cout // 64, 2, 32)
        ref = (v[..., 0, :] * F.gelu(v[..., 1, :])).reshape(1, Ho, Ho, half)
        assert rel(y[i:i + 1], ref) < TOL
