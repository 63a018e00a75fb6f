"""Tile stamps of the persistent conv walks (the stamp tables of profiles/tile_phase_timing.md are this script's output).

    python profiles/tile_phase.py [--lib PATH] [--md FILE]

Builds the library with -DDFW_TILE_STAMPS into a scratch directory (or takes a prebuilt one from --lib), runs the step's conv
shapes that walk >= 4 tile rounds on the full grid and with the grid cut to 32 and 8 workgroups (the same tiles per
workgroup, uniform random bf16), and prints per configuration: the tile period, the K-walk and epilogue durations of wave 0
(median over workgroups and tiles; the epilogue's end is the issue of its last store), the spread of the epilogue-start
times across workgroups in the first, middle and last round, and the shader clock (s_memtime ticks per s_memrealtime us).
Full-grid minus small-grid epilogue, in CYCLES, is what contention between workgroups adds to the per-tile fixed cost.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# kernel, Cin, Cout, tile rounds on 256 workgroups in the step, residual; all of BASELINE configs[1] (r04_shapes.txt, up2x_timing.md)
STAMP_SHAPES = [
    ("patch512", 128, 128, 24, True),    # VAE 512^2 x 12 images, N = 128
    ("patch512", 128, 128, 24, False),
    ("patch512", 128, 128, 8, True),     # VAE decoder 512^2 x 4
    ("patch8", 256, 256, 12, True),      # VAE 256^2 x 12
    ("patch8", 256, 256, 12, False),
    ("patch8", 512, 512, 6, True),       # VAE 128^2 x 12, two n-tiles
    ("patch8", 256, 256, 4, True),       # VAE decoder 256^2 x 4
    ("up2x", 256, 256, 16, False),       # VAE decoder 256^2 -> 512^2
    ("up2x", 512, 512, 8, False),        # VAE decoder 128^2 -> 256^2
]


def build_stamped(dst):
    from diffews_amd import build as b
    objs = [os.path.join(dst, src.replace(".hip", ".o")) for src in b.SOURCES]
    for i in range(0, len(objs), 8):             # eight compiles at a time
        procs = [subprocess.Popen([os.environ.get("HIPCC", "hipcc"), *b.FLAGS, "-DDFW_TILE_STAMPS", "-c", os.path.join(b.CSRC, src), "-o", obj])
                 for src, obj in zip(b.SOURCES[i:i + 8], objs[i:i + 8])]
        if any(p.wait() for p in procs):
            raise SystemExit("hipcc failed")
    lib = os.path.join(dst, "libdiffews_hip_stamps.so")
    subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs])
    return lib


def rand(shape, seed, scale=1.0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand(shape, generator=g, device="cuda") * 2 - 1) * scale).to(torch.bfloat16)


def make_call(kind, Cin, Cout, m_tiles, residual):
    """A call of m_tiles m-tiles (256 output pixels; patch512: 512) on 128-pixel-wide images: (callable, kernel-name getter)."""
    import torch
    from diffews_amd import ops, packing
    rows8 = m_tiles // 8 if kind != "up2x" else m_tiles // 16        # image rows of tiles (8 tiles per row; up2x: 4 blocks x 4 parities)
    B = next(b for b in range(1, rows8 + 1) if rows8 % b == 0 and rows8 // b <= 16)
    ph = 32 if kind == "patch512" else 16
    H, W = ph * (rows8 // B), 128 if kind != "up2x" else 64
    x = rand((B, H, W, Cin), 1)
    w = packing.pack_conv3x3(rand((Cout, Cin, 3, 3), 2, (9 * Cin) ** -0.5).cpu())
    bias = rand((Cout,), 3).float()
    if kind == "up2x":
        wf, w = packing.fold_up2x(w).cuda(), w.cuda()
        return lambda: ops.conv3x3_stream(x, w, Cout, bias=bias, w_up2x=wf, ups=True, gn_groups=32)
    w = w.cuda()
    res = rand((B, H, W, Cout), 4) if residual else None
    return lambda: ops.conv3x3(x, w, Cout, bias=bias, residual=res, gn_groups=32)


def kernel_of(call):
    import torch
    from diffews_amd import ops
    names = []
    ops.gemm_hook = lambda name, *a, **k: names.append(name)
    try:
        call()
        torch.cuda.synchronize()
    finally:
        ops.gemm_hook = None
    return names[-1]


def stamps_mode(args):
    lib_path = args.lib or build_stamped(tempfile.mkdtemp(prefix="dfw_stamps_"))
    os.environ["DFW_LIB"] = lib_path
    import numpy as np
    import torch
    from diffews_amd import _lib
    h = _lib.lib()
    h.dfw_debug_tile_stamps.restype = C.c_int32
    h.dfw_debug_tile_stamps.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    want = {"patch512": "conv_patch_kernel<bf16,512,128>", "patch8": "conv_patch8_kernel<bf16,256,256>", "up2x": "gemm8_kernel<bf16,256,256,64,up2x>"}
    out = ["| kernel | Cin | N | res | rounds | grid | tile period us | K walk us | epilogue us (median / p90) | epilogue cycles | "
           "epilogue-start spread us, round 0 / mid / last | clock MHz |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]

    def run(kind, Cin, Cout, r, residual, grid):
        ntn = max(1, Cout // 256)
        m_tiles = grid * r // ntn
        _lib.configure(big_min_tiles=1)
        call = make_call(kind, Cin, Cout, m_tiles, residual)
        if kernel_of(call) != want[kind]:
            out.append(f"| {kind} | {Cin} | {Cout} | {int(residual)} | {r} | {grid} | not eligible at this size | | | | | |")
            return
        buf = torch.zeros(256 * r * 4, dtype=torch.int64, device="cuda")
        call()
        torch.cuda.synchronize()
        assert h.dfw_debug_tile_stamps(buf.data_ptr(), r, grid if grid < 256 else 0) == 0
        call()
        torch.cuda.synchronize()
        assert h.dfw_debug_tile_stamps(None, 0, 0) == 0
        s = buf.cpu().numpy().reshape(256, r, 4)[:grid].astype(np.float64)
        assert (s[:, :, 1] > 0).all(), "a workgroup wrote no stamp"
        clk = np.median((s[:, -1, 1] - s[:, 0, 1]) / ((s[:, -1, 3] - s[:, 0, 3]) * 10e-9)) / 1e6      # s_memtime ticks per us
        period = np.median(np.diff(s[:, :, 1], axis=1)) / clk
        kwalk = np.median(s[:, :, 1] - s[:, :, 0]) / clk
        epi = (s[:, :, 2] - s[:, :, 1]).ravel() / clk
        spread = [(s[:, j, 3].max() - s[:, j, 3].min()) * 0.01 for j in (0, r // 2, r - 1)]
        out.append(f"| {kind} | {Cin} | {Cout} | {int(residual)} | {r} | {grid} | {period:.1f} | {kwalk:.1f} | {np.median(epi):.2f} / "
                   f"{np.percentile(epi, 90):.2f} | {np.median(epi) * clk:.0f} | {spread[0]:.1f} / {spread[1]:.1f} / {spread[2]:.1f} | {clk:.0f} |")
        print(out[-1], flush=True)

    for kind, Cin, Cout, r, residual in STAMP_SHAPES:
        for grid in (256, 32, 8):
            run(kind, Cin, Cout, r, residual, grid)
    _lib.configure()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="a prebuilt -DDFW_TILE_STAMPS library (default: build one into a scratch directory)")
    ap.add_argument("--md", default=None, help="also write the table to this file")
    a = ap.parse_args()
    rows = stamps_mode(a)
    if a.md:
        with open(a.md, "w") as f:
            f.write("\n".join(rows) + "\n")
