"""The boundary convs (csrc/misc.hip: conv_small_kernel, conv_small4_kernel, conv_small8w_kernel<T, 9|1>) in both storage
dtypes, checked element by element.

Every output element is compared with an fp64 reference computed from the fp32 x and w the kernel reads
(elementwise_bound.conv_small_ref: `taps` shifted products over the zero-padded NCHW input, in_scale on the input, bias,
out_scale last) within

    |y - r| <= u_T |r| + C_ACC 2^-24 (sqrt(K) |x in_scale|.|w| + |bias|) |out_scale| + floor_T,   K = taps * Cin

with u_T of the output (storage dtype for OUT_T, fp32 for OUT_F32 and NCHW fp32); `-s` prints the worst err / bound ratio
of every case (lines starting with BNDRATIO).  The fused GroupNorm sums of conv_small8w are compared per (image, chunk,
group) with fp64 sums of the stored output (elementwise_bound.cs_chunk_check).  tests/test_boundary_plans_cpu.py imports
the case table and proves, without a GPU, that it reaches every kernel x taps x output mode the dispatcher can produce,
iters in {1, 2 .. 7, 8}, a last workgroup that leaves the pixel-group loop early and a partly live 128-channel block.

Shapes: the product's own (VAE encoder conv_in 3 -> 128 at 512 x 512 with B = 1 and 4, decoder conv_in 4 -> 512 at
64 x 64, UNet conv_in 4 -> 320 and conv_in_ref 8 -> 320 at 64 x 64 with B = 16 and into batch slices of one buffer, the
1 x 1 quant_conv head / post_quant_conv with the VAE scaling factor, the training step's conv_out data gradient, the
latents of 384 x 384 and 320 x 512 inputs) and the edges: W in {4, 8, 10, 12, 13, 20}, H = 1, Cin in {1, 3, 4, 5, 8},
Cout in {3, 4, 8, 64, 128, 320, 512}, no bias, an input view that is not 16-byte aligned, two and three source tensors
whose boundaries fall inside a workgroup's pixels, NCHW channel slices and NHWC batch slices of sentinel-filled buffers.
"""
import ctypes as C
import re
from dataclasses import dataclass

import pytest
import torch

import elementwise_bound as eb

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
TNAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
F32 = torch.float32
SENTINEL = 3.0
VAE_SCALE = 0.18215


@dataclass
class Cs:
    id: str
    B: object                 # int, or a tuple of batch sizes: the batch is read in place from that many tensors
    Cin: int
    H: int
    W: int
    Cout: int
    taps: int = 9
    mode: str = "T"           # 'T' NHWC storage dtype, 'F32' NHWC fp32, 'NCHW' NCHW fp32
    bias: bool = True
    in_scale: float = 1.0
    out_scale: float = 1.0
    gn: int = 0               # GroupNorm groups whose partial sums are requested
    gn_slice: bool = False    # gn_part= images 1 .. B of a [B + 2] partial-sum buffer
    misalign: bool = False    # x starts 4 bytes past a 16-byte boundary
    wide: tuple = None        # NCHW: (channels of the destination tensor, first channel written)
    batch_slice: tuple = None  # NHWC: (images of the destination buffer, first image written)

    @property
    def batch(self):
        return sum(self.B) if isinstance(self.B, tuple) else self.B


CASES = [
    # ---- conv_small8w_kernel: the product's shapes
    Cs("vae_in_b1", 1, 3, 512, 512, 128, gn=32),                              # iters 1, 2048 chunks, cpg 4
    Cs("vae_in_b4", 4, 3, 512, 512, 128, gn=32, gn_slice=True),               # iters 4, 512 chunks per image
    Cs("vae_in_b2_f32", 2, 3, 512, 512, 128, mode="F32"),                     # iters 2
    Cs("dec_in", 2, 4, 64, 64, 512, gn=32, gn_slice=True),                    # cpg 16
    Cs("unet_in_b16", 16, 4, 64, 64, 320),                                    # third 128-block: 64 live channels
    Cs("unet_in_ref_b16_f32", 16, 8, 64, 64, 320, mode="F32"),
    Cs("unet_in_ref_slice", 5, 8, 64, 64, 320, batch_slice=(9, 3)),
    Cs("unet_in_slice_f32", 4, 4, 64, 64, 320, mode="F32", batch_slice=(9, 0)),
    Cs("dgrad_conv_out", 2, 4, 64, 64, 320, bias=False),
    Cs("lat_384", 3, 4, 48, 48, 320),
    Cs("lat_320x512_f32", 2, 8, 40, 64, 320, mode="F32"),
    # ---- conv_small8w_kernel: iters, early exit, edges
    Cs("it8_c8", 8, 4, 512, 512, 8, in_scale=0.5, out_scale=2.0),             # iters 8, one live octet of 16
    Cs("it3_t1_c8_f32", 3, 8, 512, 512, 8, taps=1, mode="F32", in_scale=0.5, out_scale=2.0),
    Cs("early_exit", 3, 3, 500, 520, 64),                                     # iters 2, nq = 97500 = 3046 * 32 + 28
    Cs("gn_cpg8_it2", 2, 4, 256, 512, 256, gn=32),                            # iters 2, cpg 8
    Cs("gn_straddle", 3, 3, 5, 24, 128, gn=32),                               # 15 pixel groups per image: no fused sums
    Cs("w8_h1", 5, 5, 1, 8, 64),
    Cs("w8_c128", 2, 1, 9, 8, 128, in_scale=VAE_SCALE, out_scale=3.0),
    Cs("t1_T", 2, 8, 16, 24, 128, taps=1, in_scale=0.5, out_scale=2.0),
    Cs("t1_c512_nobias", 1, 3, 4, 16, 512, taps=1, bias=False),
    Cs("src2_8w", (3, 2), 3, 8, 24, 128),                                     # 24 pixel groups per image, 16 per workgroup
    Cs("src3_8w_f32", (1, 3, 2), 4, 8, 24, 320, mode="F32"),
    Cs("src3_gn", (2, 1, 3), 3, 16, 16, 128, gn=32),
    # ---- conv_small4_kernel
    Cs("w4_w12_t9", 2, 3, 20, 12, 64),
    Cs("w4_w4_f32", 3, 4, 5, 4, 128, mode="F32"),
    Cs("w4_w20_t1", 2, 8, 6, 20, 320, taps=1, in_scale=0.5, out_scale=2.0),
    Cs("w4_t1_f32", 1, 5, 3, 12, 8, taps=1, mode="F32"),
    Cs("w4_c512", 1, 4, 3, 12, 512, bias=False),
    Cs("w4_nchw_t9_c3", 2, 4, 9, 16, 3, mode="NCHW", wide=(8, 2)),            # W % 8 == 0, NCHW: the 4-wide kernel
    Cs("w4_nchw_t9_c8_b1", 1, 8, 6, 12, 8, mode="NCHW", wide=(16, 8)),
    Cs("quant_head", 4, 8, 64, 64, 4, taps=1, mode="NCHW", wide=(8, 4), out_scale=VAE_SCALE),
    Cs("post_quant", 2, 4, 64, 64, 4, taps=1, mode="NCHW", in_scale=1.0 / VAE_SCALE),
    Cs("src2_w4", (1, 2), 3, 5, 12, 64),
    Cs("src3_nchw", (2, 1, 1), 8, 6, 12, 3, taps=1, mode="NCHW", wide=(8, 4)),
    # ---- conv_small_kernel
    Cs("sc_w10_t9", 2, 3, 7, 10, 64),
    Cs("sc_w13_t1_f32", 3, 5, 6, 13, 8, taps=1, mode="F32", in_scale=0.5, out_scale=2.0),
    Cs("sc_w13_t9_f32_c320", 1, 1, 5, 13, 320, mode="F32", bias=False),
    Cs("sc_w10_t1", 2, 8, 3, 10, 128, taps=1),
    Cs("sc_c512", 1, 4, 3, 10, 512),
    Cs("sc_nchw_t9_c3", 2, 4, 9, 10, 3, mode="NCHW", wide=(8, 2)),
    Cs("sc_nchw_t1_c4", 1, 8, 5, 13, 4, taps=1, mode="NCHW"),
    Cs("sc_unaligned_w16", 2, 3, 6, 16, 64, misalign=True),
    Cs("sc_h1", 2, 4, 1, 7, 8),
    Cs("src2_sc", (2, 3), 4, 7, 10, 8),
]
BY_ID = {c.id: c for c in CASES}


def args_of(case, dtype, L):
    """The dfw_conv_small_args ops.conv_small builds for this case, without tensors (x carries only its alignment)."""
    a = L.ConvSmallArgs()
    a.x = 20 if case.misalign else 16
    a.B, a.Cin, a.H, a.Wd, a.Cout, a.taps, a.ldy = case.batch, case.Cin, case.H, case.W, case.Cout, case.taps, case.Cout
    a.in_scale, a.out_scale = case.in_scale, case.out_scale
    a.out_mode = {"T": L.OUT_T, "F32": L.OUT_F32, "NCHW": L.OUT_NCHW_F32}[case.mode]
    a.dtype = L.BF16 if dtype == torch.bfloat16 else L.F16
    a.gn_groups = case.gn if case.mode == "T" else 0
    return a


def planned(case, dtype, L):
    """(kernel name with taps, iters, 'GXxGY', fused-sum chunks per image) from the library's host-only queries."""
    a = args_of(case, dtype, L)
    buf = C.create_string_buffer(96)
    L.check(L.lib().dfw_conv_small_kernel_name(C.byref(a), buf, 96), "dfw_conv_small_kernel_name")
    m = re.fullmatch(r"(\S+?)(?: iters=(\d+))? grid=(\d+x\d+)", buf.value.decode())
    assert m, buf.value
    return m.group(1), int(m.group(2) or 1), m.group(3), L.lib().dfw_conv_small_gn_chunks(C.byref(a))


@pytest.fixture(scope="module")
def env(hip_lib):
    from diffews_amd import ops, _lib
    return ops, _lib


def make_inputs(case, seed, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    sizes = case.B if isinstance(case.B, tuple) else (case.B,)
    xs = []
    for b in sizes:
        n = b * case.Cin * case.H * case.W
        buf = torch.empty(n + 4, dtype=F32, device=device)
        x = buf[1:n + 1] if case.misalign else buf[:n]
        x.copy_(torch.randn(n, generator=g, device=device))          # non-zero on every border
        xs.append(x.view(b, case.Cin, case.H, case.W))
    K = case.taps * case.Cin
    w = torch.randn(case.Cout, case.taps, case.Cin, generator=g, device=device) * K ** -0.5
    bias = torch.randn(case.Cout, generator=g, device=device) if case.bias else None
    return xs, w, bias


def run(ops, case, dtype, xs, w, bias, chunks):
    """-> (y, the sentinel-filled buffer y is a view of or None, gn_part buffer or None)."""
    B, full, part_full, out, gn_part = case.batch, None, None, None, None
    dev = w.device
    if case.mode == "NCHW" and case.wide:
        full = torch.full((B, case.wide[0], case.H, case.W), SENTINEL, dtype=F32, device=dev)
        out = full[:, case.wide[1]:case.wide[1] + case.Cout]
    elif case.batch_slice:
        full = torch.full((case.batch_slice[0], case.H, case.W, case.Cout), SENTINEL,
                          dtype=F32 if case.mode == "F32" else dtype, device=dev)
        out = full[case.batch_slice[1]:case.batch_slice[1] + B]
    if case.gn_slice:
        part_full = torch.full((B + 2, chunks, case.gn, 2), SENTINEL, dtype=F32, device=dev)
        gn_part = part_full[1:1 + B]
    y = ops.conv_small(xs if len(xs) > 1 else xs[0], w, bias, case.Cout, case.taps, dtype, nchw_f32_out=case.mode == "NCHW",
                       in_scale=case.in_scale, out_scale=case.out_scale, gn_groups=case.gn, out=out, gn_part=gn_part,
                       out_f32=case.mode == "F32")
    return y, full, part_full


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_conv_small_per_element(env, case, dtype):
    ops, L = env
    kernel, iters, grid, chunks = planned(case, dtype, L)
    xs, w, bias = make_inputs(case, 1000 + CASES.index(case))
    if case.misalign:
        assert xs[0].data_ptr() % 16 == 4
    y, full, part_full = run(ops, case, dtype, xs, w, bias, chunks)
    torch.cuda.synchronize()
    B, H, W, Cout = case.batch, case.H, case.W, case.Cout
    out_dtype = dtype if case.mode == "T" else F32
    # rows / channels outside the destination view keep their sentinel
    if full is not None:
        keep = torch.ones_like(full, dtype=torch.bool)
        if case.mode == "NCHW":
            keep[:, case.wide[1]:case.wide[1] + Cout] = False
        else:
            keep[case.batch_slice[1]:case.batch_slice[1] + B] = False
        assert bool((full[keep] == SENTINEL).all()), f"{case.id}: wrote outside the destination view"
    # several sources == the same call on their concatenation, bit for bit
    xcat = torch.cat(xs) if len(xs) > 1 else xs[0]
    if len(xs) > 1:
        y1, _, p1 = run(ops, case, dtype, [xcat.contiguous()], w, bias, chunks)
        assert torch.equal(y, y1), f"{case.id}: {len(xs)} sources differ from their torch.cat"
    worst = 0.0
    for b in range(B):
        r, e = eb.conv_small_ref(xcat[b:b + 1], w, bias, case.taps, case.in_scale, case.out_scale)
        yb = y[b].permute(1, 2, 0) if case.mode == "NCHW" else y[b]
        where = eb.Where(Cout, H * W, W)
        worst = max(worst, eb.check(yb, r, e, out_dtype, label=f"{case.id} {kernel}",
                                    where=lambda i, b=b: where(i).replace("image 0", f"image {b}", 1)))
    print(f"BNDRATIO {kernel} {case.mode} {TNAME[dtype]} {case.id} iters={iters} grid={grid} {worst:.4f}")
    if case.gn:
        stats = getattr(y, "_gn_stats", None)
        if chunks == 0:
            assert stats is None, f"{case.id}: fused sums for a shape whose workgroups straddle images"
            return
        assert stats is not None and stats[1] == chunks and stats[2] == case.gn, f"{case.id}: no fused sums"
        part = stats[0]
        if len(xs) > 1:
            assert torch.equal(part, y1._gn_stats[0])
        if part_full is not None:
            assert part.data_ptr() == part_full[1].data_ptr()
            assert bool((part_full[0] == SENTINEL).all()) and bool((part_full[-1] == SENTINEL).all())
        ws = eb.cs_chunk_check(y, part, case.gn, iters, label=case.id)
        print(f"BNDRATIO {kernel} gn_sums {TNAME[dtype]} {case.id} iters={iters} chunks={chunks} {ws:.4f}")
