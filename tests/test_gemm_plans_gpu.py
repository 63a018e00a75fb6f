"""Plan matrix of dfw_gemm and dfw_gemm_tn: every kernel instantiation in both storage dtypes, checked element by element.

Each case names the kernel the planner must pick for it -- asserted here through ops.gemm_hook (forward) and the
dfw_gemm_tn_kernel_name query on the arguments ops_bwd.gemm_tn passes (weight gradients), and without a GPU by
tests/test_gemm_plans_cpu.py, which also proves that the cases together reach every instantiation -- plus the dfw_config
override that steers the planner there at a small size.  Every output element of every image is compared with an fp64
reference within its rounding bound (tests/elementwise_bound.py); `-s` prints the planned kernel and the worst
err / bound ratio of every case.

Edges the cases carry where the kernel's eligibility allows them: ragged M (last tile of 1 row, of BM - 1 rows), ragged N
(N % 128 == 64), the minimum and an odd K-tile count, row-bias images that end inside a tile (rows_per_img not a multiple
of the tile height, ld_rowbias > N), conv maps with H*W % 64 != 0 and B = 3 on gemm_kernel, every epilogue operand,
batched bmm_nt with ragged M, the W_blocked weight copy on both conv_patch tiles, and at least one case per persistent
kernel with more tiles than workgroups (each workgroup walks several tiles).

Fused GroupNorm sums: every epilogue that emits them (conv_patch, conv_patch8, gemm8 and gemm_big conv tiles, 16-bit and
fp32 output) sums the values it STORES -- the staged 16-bit values it then copies out (gemm8.hip / conv_patch*.hip: the
statistics loop reads the staging buffer), or the fp32 values it writes (GnRegSums) -- so each (image, chunk, group)
slot is compared with the fp64 sums of the returned y over exactly the pixels of that chunk.

Output views (ops.linear(out=wide[:, 4:4 + N]): ldc % 8 == 4 and C 8 bytes past a 16-byte boundary) on the gemm8
256 x 256 / 256 x 128, gemm_big and gemm_kernel shapes: the gemm8 and gemm_big epilogues store 16-byte chunks of output
rows; 8-byte alignment was verified for them on the MI355X by these cases (exact per-element results, the columns
around the view untouched), so their eligibility keeps no alignment guard (conv_patch8 and gemm8's 256 x 160 tile,
which have one, plan their fallbacks).
"""
import contextlib
import ctypes as C
import math
import re
from dataclasses import dataclass

import pytest
import torch

import elementwise_bound as eb

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
TNAME = {torch.bfloat16: "bf16", torch.float16: "f16"}

# dfw_config overrides: gemm_kernel with a forced tile and no big kernels; gemm_big with a forced configuration, gemm8
# off and any tile count; the default planner with any tile count
GK = dict(big_kernels=0, conv_patch=0)
BIG = dict(k8=0, conv_patch=0, big_min_tiles=1)
ANY = dict(big_min_tiles=1)


@dataclass
class Fwd:
    id: str
    op: str                  # linear | conv | bmm
    shape: tuple             # linear (M, N, K); conv (B, H, W, Cin, Cout, stride, pad, ups); bmm (Bt, M, N, K)
    expect: str              # planned kernel, {T} = bf16 | f16
    cfg: dict
    bias: bool = False
    rowbias: int = 0         # linear: rows per row-bias image (conv: always Ho*Wo when > 0); 0: no row bias
    res: str = ""            # residual: "" none, "T" storage dtype, "F32" the fp32 residual stream
    out: str = "T"           # T | F32 | NCHW (fp32 NCHW)
    scale: float = 1.0
    colscale: tuple = None
    act: str = None          # None | "silu"
    geglu: bool = False
    splitk: int = None
    gn: int = 0              # GroupNorm groups of the fused sums (conv)
    wblk: bool = False       # conv: also pass the blocked weight copy (W_blocked)
    view: bool = False       # linear: write into out = wide[:, 4:4 + N] of a wider buffer


def F(id, op, shape, expect, cfg, **kw):
    return Fwd(id, op, shape, expect, dict(cfg), **kw)


FWD_CASES = [
    # ---- gemm_kernel (gemm.hip), forced tiles, big kernels off; splitk=1 fixes the split-K plan
    F("gk128x128_lin", "linear", (1025, 320, 64), "gemm_kernel<{T},128,128,lin>", dict(GK, gemm_bm=128, gemm_bn=128),
      bias=True, rowbias=100, res="T", scale=0.75, colscale=(64, 0.5), splitk=1),
    F("gk128x64_lin_rf32", "linear", (1279, 192, 192), "gemm_kernel<{T},128,64,lin>", dict(GK, gemm_bm=128, gemm_bn=64),
      bias=True, rowbias=300, res="F32", scale=0.5, splitk=1),
    F("gk64x64_lin_silu", "linear", (8193, 640, 320), "gemm_kernel<{T},64,64,lin>", dict(GK, gemm_bm=64, gemm_bn=64),
      bias=True, rowbias=1000, scale=0.5, act="silu", splitk=1),
    F("gk64x64_lin_rf32_f32", "linear", (257, 64, 128), "gemm_kernel<{T},64,64,lin>", dict(GK, gemm_bm=64, gemm_bn=64),
      bias=True, res="F32", out="F32", splitk=1),
    F("gk128x128_lin_rf32_f32", "linear", (300, 256, 640), "gemm_kernel<{T},128,128,lin>",
      dict(GK, gemm_bm=128, gemm_bn=128), rowbias=150, res="F32", out="F32", splitk=1),
    F("gk128x128_geglu", "linear", (260, 512, 128), "gemm_kernel<{T},128,128,lin>", GK, bias=True, geglu=True),
    F("gk_splitk_silu", "linear", (96, 128, 1280), "gemm_kernel<{T},128,64,lin>+splitk", dict(GK, gemm_bm=128, gemm_bn=64),
      bias=True, rowbias=32, res="T", scale=0.5, act="silu", splitk=5),
    F("gk_splitk_rf32", "linear", (200, 192, 1024), "gemm_kernel<{T},64,64,lin>+splitk", dict(GK, gemm_bm=64, gemm_bn=64),
      bias=True, res="F32", out="F32", splitk=3),
    F("gk128x128_conv", "conv", (3, 13, 19, 64, 192, 1, 1, False), "gemm_kernel<{T},128,128,conv>",
      dict(GK, gemm_bm=128, gemm_bn=128), bias=True, rowbias=1, res="T", scale=0.75, splitk=1),
    F("gk128x64_conv_s2_rf32", "conv", (3, 26, 38, 64, 64, 2, 1, False), "gemm_kernel<{T},128,64,conv>",
      dict(GK, gemm_bm=128, gemm_bn=64), bias=True, rowbias=1, res="F32", out="F32", splitk=1),
    F("gk64x64_conv_ups_nchw", "conv", (3, 7, 10, 128, 128, 1, 1, True), "gemm_kernel<{T},64,64,conv>",
      dict(GK, gemm_bm=64, gemm_bn=64), bias=True, rowbias=1, out="NCHW", scale=0.5, splitk=1),
    F("gk64x64_conv_pad0_rf32", "conv", (3, 26, 38, 64, 128, 2, 0, False), "gemm_kernel<{T},64,64,conv>",
      dict(GK, gemm_bm=64, gemm_bn=64), res="F32", splitk=1),
    F("gk128x64_conv_silu", "conv", (3, 13, 19, 192, 64, 1, 1, False), "gemm_kernel<{T},128,64,conv>",
      dict(GK, gemm_bm=128, gemm_bn=64), bias=True, act="silu", splitk=1),
    F("gk128x128_conv_rf32", "conv", (3, 13, 19, 64, 128, 1, 1, False), "gemm_kernel<{T},128,128,conv>",
      dict(GK, gemm_bm=128, gemm_bn=128), bias=True, rowbias=1, res="F32", out="F32", splitk=1),
    F("gk64x64_conv_persistent", "conv", (4, 64, 64, 64, 320, 1, 1, False), "gemm_kernel<{T},64,64,conv>",
      dict(GK, gemm_bm=64, gemm_bn=64), bias=True, rowbias=1, res="T", splitk=1),
    F("gk_conv_splitk", "conv", (2, 8, 8, 256, 128, 1, 1, False), "gemm_kernel<{T},128,128,conv>+splitk",
      dict(GK, gemm_bm=128, gemm_bn=128), bias=True, rowbias=1, res="T", splitk=3),
    # ---- gemm_big (gemm_big.hip): forced configurations, gemm8 off
    F("big256x256_lin", "linear", (769, 512, 128), "gemm_big_kernel<{T},256,256,32,lin>",
      dict(BIG, big_bm=256, big_bn=256, big_bk=32), bias=True, rowbias=300, res="T", scale=0.75, colscale=(128, 0.5)),
    F("big512x128_lin", "linear", (1023, 320, 192), "gemm_big_kernel<{T},512,128,32,lin>",
      dict(BIG, big_bm=512, big_bn=128, big_bk=32), bias=True, rowbias=200, res="T"),
    F("big256x128x64_lin_persistent", "linear", (33279, 192, 256), "gemm_big_kernel<{T},256,128,64,lin>",
      dict(BIG, big_bm=256, big_bn=128, big_bk=64), bias=True, rowbias=1000, res="T", scale=0.5),
    F("big256x128x32_lin", "linear", (513, 384, 128), "gemm_big_kernel<{T},256,128,32,lin>",
      dict(BIG, big_bm=256, big_bn=128, big_bk=32), bias=True, colscale=(64, 2.0)),
    F("big256x128x64_geglu", "linear", (700, 1024, 256), "gemm_big_kernel<{T},256,128,64,lin>",
      dict(BIG, big_bm=256, big_bn=128, big_bk=64), bias=True, geglu=True),
    F("big256x256_conv_gn", "conv", (3, 16, 16, 64, 256, 1, 1, False), "gemm_big_kernel<{T},256,256,32,conv>",
      dict(BIG, big_bm=256, big_bn=256, big_bk=32), bias=True, rowbias=1, res="T", scale=0.5, gn=32),
    F("big512x128_conv_s2_gn", "conv", (3, 64, 32, 64, 192, 2, 1, False), "gemm_big_kernel<{T},512,128,32,conv>",
      dict(BIG, big_bm=512, big_bn=128, big_bk=32), bias=True, rowbias=1, gn=24),
    F("big256x128x64_conv_ups_gn", "conv", (3, 8, 16, 64, 128, 1, 1, True), "gemm_big_kernel<{T},256,128,64,conv>",
      dict(BIG, big_bm=256, big_bn=128, big_bk=64), bias=True, res="T", gn=32),
    F("big256x128x32_conv_pad0", "conv", (3, 32, 32, 128, 64, 2, 0, False), "gemm_big_kernel<{T},256,128,32,conv>",
      dict(BIG, big_bm=256, big_bn=128, big_bk=32), bias=True, rowbias=1, res="T", splitk=1),
    F("big256x256_lin_f32o", "linear", (513, 256, 128), "gemm_big_kernel<{T},256,256,32,lin>", BIG,
      bias=True, rowbias=200, res="F32", out="F32", scale=0.5),
    F("big512x128_lin_f32o", "linear", (1000, 384, 192), "gemm_big_kernel<{T},512,128,32,lin>", BIG,
      bias=True, res="F32", out="F32"),
    F("big256x256_conv_f32o_gn", "conv", (3, 16, 16, 64, 256, 1, 1, False), "gemm_big_kernel<{T},256,256,32,conv>", BIG,
      bias=True, rowbias=1, res="F32", out="F32", gn=32),
    F("big512x128_conv_f32o_gn", "conv", (3, 32, 16, 64, 128, 1, 1, False), "gemm_big_kernel<{T},512,128,32,conv>", BIG,
      bias=True, res="T", out="F32", gn=16),
    # ---- gemm8 (gemm8.hip): the default planner at any tile count
    F("g8_256x256_lin", "linear", (769, 512, 128), "gemm8_kernel<{T},256,256,64,lin>", ANY,
      bias=True, rowbias=300, res="T", scale=0.75, colscale=(128, 0.5)),
    F("g8_256x256_lin_persistent", "linear", (16641, 1024, 192), "gemm8_kernel<{T},256,256,64,lin>", {},
      bias=True, rowbias=5000, res="T"),
    F("g8_256x256_geglu", "linear", (1000, 512, 128), "gemm8_kernel<{T},256,256,64,lin>", ANY, bias=True, geglu=True),
    F("g8_256x128_lin_persistent", "linear", (10241, 1344, 320), "gemm8_kernel<{T},256,128,64,lin>", ANY,
      bias=True, rowbias=3000, res="T", colscale=(320, 0.25)),
    F("g8_256x128_lin_ragged", "linear", (767, 192, 256), "gemm8_kernel<{T},256,128,64,lin>",
      dict(ANY, big_bm=256, big_bn=128, big_bk=64), bias=True, res="T", scale=0.5),
    F("g8_256x256_conv_ups_gn", "conv", (3, 8, 8, 64, 256, 1, 1, True), "gemm8_kernel<{T},256,256,64,conv>", ANY,
      bias=True, rowbias=1, res="T", gn=32),
    F("g8_256x128_conv_pad0_gn", "conv", (3, 32, 32, 128, 128, 2, 0, False), "gemm8_kernel<{T},256,128,64,conv>", ANY,
      bias=True, rowbias=1, scale=0.5, gn=16, splitk=1),
    F("g8_256x160_lin", "linear", (511, 320, 128), "gemm8_kernel<{T},256,160,64,lin>", ANY,
      bias=True, rowbias=300, res="T", colscale=(64, 0.25)),
    F("g8_256x160_lin_persistent", "linear", (32769, 320, 320), "gemm8_kernel<{T},256,160,64,lin>", {},
      bias=True, res="T", scale=0.5),
    # ---- conv_patch (conv_patch.hip): >= 192 tiles whatever the config; mode 2 adds the 256 x 256 tile
    F("cp512x128_persistent_gn", "conv", (3, 128, 128, 64, 384, 1, 1, False), "conv_patch_kernel<{T},512,128>", {},
      bias=True, rowbias=1, res="T", scale=0.5, gn=48),
    F("cp512x128_wblk", "conv", (2, 128, 192, 64, 256 + 128, 1, 1, False), "conv_patch_kernel<{T},512,128>", {},
      bias=True, res="T", wblk=True),
    F("cp256x256_gn", "conv", (3, 128, 128, 64, 256, 1, 1, False), "conv_patch_kernel<{T},256,256>", dict(conv_patch=2),
      bias=True, rowbias=1, res="T", gn=32),
    F("cp256x256_wblk", "conv", (3, 128, 128, 64, 256, 1, 1, False), "conv_patch_kernel<{T},256,256>",
      dict(conv_patch=2), bias=True, rowbias=1, wblk=True),
    F("cp512x128_f32o_gn", "conv", (3, 128, 256, 64, 128, 1, 1, False), "conv_patch_kernel<{T},512,128>", {},
      bias=True, rowbias=1, res="F32", out="F32", gn=32),
    F("cp256x256_f32o_gn", "conv", (3, 128, 128, 64, 256, 1, 1, False), "conv_patch_kernel<{T},256,256>",
      dict(conv_patch=2), bias=True, res="F32", out="F32", scale=0.5, gn=32),
    # ---- conv_patch8 (conv_patch8.hip)
    F("cp8_256x256_persistent_gn", "conv", (5, 128, 128, 64, 256, 1, 1, False), "conv_patch8_kernel<{T},256,256>", {},
      bias=True, rowbias=1, res="T", scale=0.5, gn=32),
    F("cp8_256x128_gn", "conv", (2, 128, 128, 64, 256, 1, 1, False), "conv_patch8_kernel<{T},256,128>", {},
      bias=True, res="T", gn=32),
    F("cp8_256x128_ragged_gn", "conv", (3, 32, 32, 128, 192, 1, 1, False), "conv_patch8_kernel<{T},256,128>",
      dict(conv_patch=4, big_min_tiles=1), bias=True, rowbias=1, gn=24),
    F("cp8_256x160", "conv", (3, 32, 32, 64, 320, 1, 1, False), "conv_patch8_kernel<{T},256,160>", ANY,
      bias=True, rowbias=1, res="T", scale=0.75),
    # ---- batched bmm_nt, M not a tile multiple
    F("bmm_gemm8", "bmm", (3, 300, 256, 128), "gemm8_kernel<{T},256,256,64,lin>", ANY, scale=0.5),
    F("bmm_gk_f32", "bmm", (4, 100, 64, 192), "gemm_kernel<{T},64,64,lin>", dict(GK, gemm_bm=64, gemm_bn=64),
      out="F32", scale=0.125),
    # ---- output views: ldc % 8 == 4, C 8 bytes past a 16-byte boundary, on the planner's pick
    F("view_g8_256x256", "linear", (769, 512, 128), "gemm8_kernel<{T},256,256,64,lin>", ANY, bias=True, res="T", view=True),
    F("view_g8_256x128", "linear", (513, 1344, 320), "gemm8_kernel<{T},256,128,64,lin>", ANY, bias=True, view=True),
    F("view_big256x128x64", "linear", (700, 384, 256), "gemm_big_kernel<{T},256,128,64,lin>",
      dict(BIG, big_bm=256, big_bn=128, big_bk=64), bias=True, res="T", view=True),
    F("view_gk", "linear", (300, 192, 128), "gemm_kernel<{T},128,64,lin>", dict(GK, gemm_bm=128, gemm_bn=64),
      bias=True, splitk=1, view=True),
    F("view_g8_256x160_fallback", "linear", (511, 320, 128), "gemm_kernel<{T},128,64,lin>",
      dict(ANY, gemm_bm=128, gemm_bn=64), bias=True, splitk=1, view=True),
]


@dataclass
class Tn:
    id: str
    op: str                  # lin | conv
    shape: tuple             # lin (M, N, Kc); conv (B, H, W, Kc = Cin, N = Cout, stride, pad, ups)
    expect: str              # planned kernel, {T} = bf16 | f16
    accumulate: bool = False
    scale: float = 1.0


TN_CASES = [
    Tn("tn_lin_1x1", "lin", (1000, 320, 320), "gemm_tn_ring_kernel<{T},1,1,lin>+split"),
    Tn("tn_lin_1x2", "lin", (1000, 320, 640), "gemm_tn_ring_kernel<{T},1,2,lin>+split"),
    Tn("tn_lin_2x1", "lin", (1000, 640, 320), "gemm_tn_ring_kernel<{T},2,1,lin>+split"),
    Tn("tn_lin_2x2", "lin", (520, 1280, 1280), "gemm_tn_ring_kernel<{T},2,2,lin>"),
    Tn("tn_lin_split", "lin", (32768, 320, 320), "gemm_tn_ring_kernel<{T},1,1,lin>+split"),
    Tn("tn_lin_2x2_acc_split", "lin", (16384, 640, 640), "gemm_tn_ring_kernel<{T},2,2,lin>+split", True, 0.5),
    Tn("tn_conv_1x1", "conv", (2, 16, 16, 320, 320, 1, 1, False), "gemm_tn_ring_kernel<{T},1,1,conv>"),
    Tn("tn_conv_1x2", "conv", (2, 16, 16, 640, 320, 1, 1, False), "gemm_tn_ring_kernel<{T},1,2,conv>"),
    Tn("tn_conv_2x1", "conv", (2, 16, 16, 320, 640, 1, 1, False), "gemm_tn_ring_kernel<{T},2,1,conv>"),
    Tn("tn_conv_2x2", "conv", (2, 8, 8, 1280, 1280, 1, 1, False), "gemm_tn_ring_kernel<{T},2,2,conv>"),
    Tn("tn_conv_s2_split", "conv", (4, 64, 64, 320, 320, 2, 1, False), "gemm_tn_ring_kernel<{T},1,1,conv>+split"),
    Tn("tn_conv_pad0_acc_split", "conv", (2, 32, 32, 128, 128, 2, 0, False), "gemm_tn_ring_kernel<{T},1,1,conv>+split",
       True, 2.0),
    Tn("tn_conv_ups_acc_split", "conv", (4, 32, 32, 640, 640, 1, 1, True), "gemm_tn_ring_kernel<{T},2,2,conv>+split",
       True, 0.25),
    Tn("tn_reg_tiny", "conv", (2, 4, 4, 320, 320, 1, 1, False), "gemm_tn_kernel<{T}>"),
    Tn("tn_reg_s2", "conv", (3, 8, 12, 64, 128, 2, 1, False), "gemm_tn_kernel<{T}>"),
    Tn("tn_reg_pad0_acc", "conv", (2, 8, 8, 128, 64, 2, 0, False), "gemm_tn_kernel<{T}>", True, 0.5),
    Tn("tn_reg_ups", "conv", (2, 2, 3, 128, 64, 1, 1, True), "gemm_tn_kernel<{T}>"),
    Tn("tn_reg_split", "conv", (512, 2, 2, 128, 128, 1, 1, False), "gemm_tn_kernel<{T}>+split"),
]


def expected(case, dtype):
    return case.expect.replace("{T}", TNAME[dtype])


def name_matches(name, want):
    """want may end in '+split' (any split count > 1, which the TN cost model chooses)."""
    if want.endswith("+split"):
        return re.fullmatch(re.escape(want) + r"[0-9]+", name) is not None and not name.endswith("+split1")
    return name == want


@contextlib.contextmanager
def configured(L, cfg):
    L.configure()
    try:
        if cfg:
            L.configure(**cfg)
        yield
    finally:
        L.configure()


# ---- inputs and calls (device "cpu" + fill=False: host-only planning in tests/test_gemm_plans_cpu.py)

def _conv_out_hw(H, W, stride, pad, ups):
    if ups:
        return 2 * H, 2 * W
    if stride == 1:
        return H, W
    return ((H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1) if pad else (H // 2, W // 2)


def fwd_dims(case):
    """(M, N, K, rows_per_img, Ho, Wo, imgs) of the GEMM a case runs."""
    if case.op == "linear":
        M, N, K = case.shape
        return M, N, K, case.rowbias, 0, 0, (-(-M // case.rowbias) if case.rowbias else 1)
    if case.op == "bmm":
        Bt, M, N, K = case.shape
        return Bt * M, N, K, 0, 0, 0, 1
    B, H, W, Cin, Cout, stride, pad, ups = case.shape
    Ho, Wo = _conv_out_hw(H, W, stride, pad, ups)
    return B * Ho * Wo, Cout, 9 * Cin, Ho * Wo, Ho, Wo, B


def make_fwd_inputs(case, dtype, device, seed=0, fill=True):
    g = torch.Generator(device=device).manual_seed(seed) if fill else None

    def rnd(shape, dt=dtype, scale=1.0):
        if not fill:
            return torch.empty(shape, dtype=dt, device=device)
        return (torch.randn(shape, generator=g, device=device, dtype=torch.float32) * scale).to(dt)

    M, N, K, rpi, Ho, Wo, imgs = fwd_dims(case)
    inp = {}
    if case.op == "linear":
        inp["x"], inp["w"] = rnd((M, K)), rnd((N, K), scale=K ** -0.5)
    elif case.op == "bmm":
        Bt, Mb, _, _ = case.shape
        inp["x"], inp["w"] = rnd((Bt, Mb, K)), rnd((Bt, N, K), scale=K ** -0.5)
    else:
        B, H, W, Cin = case.shape[:4]
        inp["x"], inp["w"] = rnd((B, H, W, Cin)), rnd((N, K), scale=K ** -0.5)
        if case.wblk:
            from diffews_amd.packing import block_conv3x3
            inp["w_blk"] = block_conv3x3(inp["w"])
    if case.bias:
        inp["bias"] = rnd((N,), torch.float32, 0.5)
    if case.rowbias:
        inp["rowbias"] = rnd((imgs, N + 64), torch.float32, 0.5)[:, :N]      # ld_rowbias > N
    if case.res:
        inp["res"] = rnd((M, N), torch.float32 if case.res == "F32" else dtype)
        if case.op == "conv":
            inp["res"] = inp["res"].view(M // (Ho * Wo), Ho, Wo, N)
    if case.view:
        inp["wide"] = torch.full((M, N + 12), math.nan, dtype=dtype, device=device)
    return inp


def run_fwd(ops, case, inp):
    kw = dict(bias=inp.get("bias"), rowbias=inp.get("rowbias"), out_scale=case.scale)
    if case.op == "bmm":
        return ops.bmm_nt(inp["x"], inp["w"], out_f32=case.out == "F32", out_scale=case.scale)
    if case.op == "linear":
        N = case.shape[1]
        out = inp["wide"][:, 4:4 + N] if case.view else None
        return ops.linear(inp["x"], inp["w"], residual=inp.get("res"), rows_per_img=case.rowbias,
                          act=1 if case.act == "silu" else 0, geglu=case.geglu, out=out, out_f32=case.out == "F32",
                          splitk=case.splitk, colscale=case.colscale, **kw)
    _, _, _, _, cout, stride, pad, ups = case.shape
    return ops.conv3x3(inp["x"], inp["w"], cout, stride=stride, pad=pad, ups=ups, residual=inp.get("res"),
                       out_nchw_f32=case.out == "NCHW", out_f32=case.out == "F32", splitk=case.splitk, gn_groups=case.gn,
                       act=1 if case.act == "silu" else 0, w_blk=inp.get("w_blk"), **kw)


def tile_of(name):
    """(BM, BN) of a planned forward kernel name."""
    nums = [int(v) for v in re.findall(r"[<,](\d+)", name)]
    return nums[0], nums[1]


def make_tn_inputs(case, dtype, device, seed=0, fill=True):
    g = torch.Generator(device=device).manual_seed(seed) if fill else None

    def rnd(shape, dt=dtype):
        if not fill:
            return torch.empty(shape, dtype=dt, device=device)
        return torch.randn(shape, generator=g, device=device, dtype=torch.float32).to(dt)

    if case.op == "lin":
        M, N, Kc = case.shape
        inp = {"dy": rnd((M, N)), "x": rnd((M, Kc)), "taps": 1, "geom": None}
    else:
        B, H, W, Kc, N, stride, pad, ups = case.shape
        Ho, Wo = _conv_out_hw(H, W, stride, pad, ups)
        inp = {"dy": rnd((B * Ho * Wo, N)), "x": rnd((B, H, W, Kc)), "taps": 9, "geom": (H, W, Ho, Wo, stride, pad, ups)}
    if case.accumulate:
        inp["out"] = rnd((1, N, inp["taps"], Kc), torch.float32)
    return inp


def run_tn(ops_bwd, case, inp):
    N = case.shape[1] if case.op == "lin" else case.shape[4]
    Kc = case.shape[2] if case.op == "lin" else case.shape[3]
    out = inp["out"].clone() if case.accumulate else None
    return ops_bwd.gemm_tn(inp["dy"], inp["x"], n=N, kc=Kc, out=out, taps=inp["taps"], geom=inp["geom"],
                           accumulate=case.accumulate, scale=case.scale)


@contextlib.contextmanager
def tn_names(L, launch=True):
    """Record the plan of every dfw_gemm_tn call made inside (dfw_gemm_tn_kernel_name on the very arguments passed);
    launch=False: plan only, no device work (the call returns success without launching)."""
    real, names = L.lib(), []

    class _Lib:
        def __getattr__(self, k):
            return getattr(real, k)

        def dfw_gemm_tn(self, pa, stream):
            buf = C.create_string_buffer(96)
            L.check(real.dfw_gemm_tn_kernel_name(pa, buf, 96), "dfw_gemm_tn_kernel_name")
            names.append(buf.value.decode())
            return real.dfw_gemm_tn(pa, stream) if launch else 0

    saved = L.lib
    L.lib = lambda: _Lib()
    try:
        yield names
    finally:
        L.lib = saved


# ---- GPU runs

@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c.id for c in FWD_CASES])
def test_forward_plan(ops, case, dtype):
    from diffews_amd import _lib as L
    want = expected(case, dtype)
    inp = make_fwd_inputs(case, dtype, "cuda", seed=sum(map(ord, case.id)))
    M, N, K, rpi, Ho, Wo, imgs = fwd_dims(case)
    names = []
    with configured(L, case.cfg):
        if case.gn:     # poison the allocator's block the partial sums will get: a slot never written stays NaN
            bm, bn = tile_of(want)
            chunks = (Wo // 16) * (Ho // (bm // 16)) * (8 // (bn // 64))
            torch.full((imgs * chunks * case.gn * 2,), math.nan, device="cuda")
        ops.gemm_hook = lambda name, *a: names.append(name)
        try:
            y = run_fwd(ops, case, inp)
        finally:
            ops.gemm_hook = None
    torch.cuda.synchronize()
    assert names == [want], names
    if case.op == "linear":
        S, A = eb.gemm_ref(inp["x"], inp["w"])
    elif case.op == "bmm":
        S, A = eb.gemm_ref(inp["x"][0], inp["w"][0])
        parts = [eb.gemm_ref(inp["x"][b], inp["w"][b]) for b in range(1, inp["x"].shape[0])]
        S, A = torch.cat([S] + [p[0] for p in parts]), torch.cat([A] + [p[1] for p in parts])
    else:
        _, _, _, _, _, stride, pad, ups = case.shape
        S, A = eb.conv_ref(inp["x"], inp["w"], stride, pad, ups)
    r, e = eb.epilogue_ref(S, A, K, bias=inp.get("bias"), rowbias=inp.get("rowbias"), rows_per_img=rpi,
                           residual=inp.get("res"), out_scale=case.scale, colscale=case.colscale, act=case.act,
                           geglu=case.geglu, splits=case.splitk or 1)
    out_dt = dtype if case.out == "T" else torch.float32
    yv = y.permute(0, 2, 3, 1) if case.out == "NCHW" else y
    bm, bn = tile_of(want)
    where = eb.Where(r.shape[1], rows_per_img=rpi if case.op != "bmm" else 0, Wo=Wo, tile=(bm, bn),
                     patch=case.op == "conv" and Wo % 16 == 0 and Ho % (bm // 16) == 0,
                     batch_rows=case.shape[1] if case.op == "bmm" else 0)
    worst = eb.check(yv, r, e, out_dt, where=where, label=f"{case.id} {want}")
    msg = f"{case.id:30s} {want:40s} worst err/bound {worst:.3f}"
    if case.view:
        wide = inp["wide"]
        assert torch.isnan(wide[:, :4]).all() and torch.isnan(wide[:, 4 + N:]).all(), "stores outside the output view"
    if case.gn:
        st = getattr(y, "_gn_stats", None)
        assert st is not None, f"{want} returned no fused GroupNorm sums"
        gw = eb.gn_chunk_check(yv.reshape(imgs, Ho, Wo, N), st[0], case.gn, bm, bn, label=f"{case.id} {want}")
        msg += f"  gn sums err/tol {gw:.3f}"
    print(msg)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", TN_CASES, ids=[c.id for c in TN_CASES])
def test_tn_plan(hip_lib, case, dtype):
    from diffews_amd import _lib as L, ops_bwd
    want = expected(case, dtype)
    inp = make_tn_inputs(case, dtype, "cuda", seed=sum(map(ord, case.id)))
    with tn_names(L) as names:
        out = run_tn(ops_bwd, case, inp)
    torch.cuda.synchronize()
    assert len(names) == 1 and name_matches(names[0], want), (names, want)
    name = names[0]
    splits = int(name.split("+split")[1]) if "+split" in name else 1
    dy = inp["dy"].to(eb.F64)
    cols = [inp["x"].reshape(-1, inp["x"].shape[-1]).to(eb.F64)] if case.op == "lin" else \
        eb.conv_taps(inp["x"], *inp["geom"][4:])[2]
    S = torch.stack([dy.t() @ c for c in cols], 1)                 # [N, taps, Kc]
    A = torch.stack([dy.abs().t() @ c.abs() for c in cols], 1)
    r = case.scale * S
    e = eb.C_ACC * 2.0 ** -24 * math.sqrt(dy.shape[0]) * abs(case.scale) * A * math.sqrt(splits)
    if case.accumulate:
        pre = inp["out"][0].to(eb.F64)
        r, e = r + pre, e + eb.C_ACC * 2.0 ** -24 * pre.abs() * math.sqrt(splits)
    nsa, nsb = (int(v) for v in re.findall(r",(\d)", name)[:2]) if "ring" in name else (1, 1)
    taps, Kc = r.shape[1], r.shape[2]

    def where(flat):
        n, rem = divmod(int(flat), taps * Kc)
        t, k = divmod(rem, Kc)
        return f"out channel {n}, tap {t}, in channel {k}, tile ({n // (128 * nsa)}, {k // (128 * nsb)})"

    worst = eb.check(out[0], r, e, torch.float32, where=where, label=f"{case.id} {name}")
    print(f"{case.id:30s} {name:40s} worst err/bound {worst:.3f}")
