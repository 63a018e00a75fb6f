"""CPU tests of tiled segmentation: the window plan's geometry over a sweep, the properties of the host reference
(tests/tiles_ref.py) the GPU tests compare against, the constructed input that separates the per-window maximum from the
merged image's, and the C ABI of dfw_tiles_cut / dfw_tiles_merge (header, ctypes mirror, host-side validation: no launch,
no GPU).  Every comparison is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import nway_ref
import tiles_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _plan(*a, **k):
    from diffews_amd.input_pipeline import TilePlan
    return TilePlan(*a, **k)


# ------------------------------------------------------------------------------------------------ the plan

@pytest.mark.parametrize("S", [8, 16, 64])
def test_plan_geometry_over_a_sweep(S):
    """Every L in S..4S+3 and overlap in 0..S/2: origins ascend from 0 to L - S at most S - overlap apart, their number is
    the formula's, every pixel is covered and every covered pixel has positive weight (all ramps the plan allows at the
    ends of their range); the plan's origins are the reference's."""
    for L in range(S, 4 * S + 4):
        for ov in range(0, S // 2 + 1):
            p = _plan((L, S), (S, S), ov)
            o = p.ys
            assert p.xs == [0] and p.nx == 1 and p.ny == len(o) and p.T == len(o)
            n = 1 if L == S else 1 + -(-(L - S) // (S - ov))
            assert len(o) == n, (S, L, ov)
            assert o[0] == 0 and o[-1] == L - S, (S, L, ov)
            d = np.diff(o)
            assert (d > 0).all() and (d <= S - ov).all(), (S, L, ov, o)
            assert o == tr.origins(L, S, ov)
            assert _plan((S, L), (S, S), ov).xs == o          # the other axis runs through the same rule
            assert p.ramp == max(1, ov)
            for ramp in {1, max(1, ov), S // 2}:
                w1 = tr.axis_weights(S, ramp)
                assert (w1 > 0).all() and w1.max() == ramp
                cover = np.zeros(L, np.int64)
                for y in o:
                    cover[y:y + S] += w1
                assert (cover > 0).all(), (S, L, ov, ramp)
    p = _plan((3 * S + 1, 2 * S + 5), (S, S), S // 4)
    assert p.T == p.ny * p.nx and [p.origin(t) for t in range(p.T)] == tr.windows(p.ys, p.xs)
    assert p.window_bytes(3) == 3 * 3 * S * S * p.T


def test_plan_rejects_what_it_cannot_tile():
    with pytest.raises(ValueError, match="segment_stream"):
        _plan((7, 64), (8, 8), 0)
    with pytest.raises(ValueError, match="segment_stream"):
        _plan((64, 7), (8, 8), 0)
    with pytest.raises(ValueError, match="overlap"):
        _plan((64, 64), (8, 8), 5)
    with pytest.raises(ValueError, match="overlap"):
        _plan((64, 64), (8, 16), 5)                            # half the SHORT side
    with pytest.raises(ValueError, match="overlap"):
        _plan((64, 64), (8, 8), -1)
    for ramp in (0, 5):
        with pytest.raises(ValueError, match="ramp"):
            _plan((64, 64), (8, 8), 2, ramp=ramp)
    assert _plan((8 + 4 * 63, 8), (8, 8), 4).ny == 64         # exactly 64 origins pass
    with pytest.raises(ValueError, match="at most 64"):
        _plan((8 + 4 * 63 + 1, 8), (8, 8), 4)
    with pytest.raises(ValueError, match="at most 64"):
        _plan((8, 8 + 4 * 63 + 1), (8, 8), 4)
    p = _plan((19, 37), (8, 16), 2, ramp=4)                    # non-square tile, explicit ramp
    assert (p.tile_h, p.tile_w, p.ramp, p.ys, p.xs) == (8, 16, 4, [0, 5, 11], [0, 10, 21])


# ------------------------------------------------------------------------------------------------ the reference

CASES = [((8, 8), (8, 8), 0), ((8, 9), (8, 8), 4), ((13, 29), (8, 8), 3), ((23, 8), (8, 8), 2), ((19, 37), (8, 16), 4),
         ((88, 150), (64, 64), 8)]


def _ramps(p):
    return sorted({1, max(1, p.overlap), min(p.tile_h, p.tile_w) // 2})


@pytest.mark.parametrize("hw,tile,ov", CASES, ids=[f"{c[1][0]}x{c[1][1]}-on-{c[0][0]}x{c[0][1]}" for c in CASES])
def test_reference_properties(hw, tile, ov):
    """One window is the identity; windows cut from ONE byte image merge back to exactly that image for every ramp (a
    weighted mean of equal values); constant windows give a constant image; the maxima are the merged bytes'."""
    rs = np.random.RandomState(hw[0] * 100 + hw[1])
    p = _plan(hw, tile, ov)
    img = rs.randint(0, 256, (2, 3) + hw).astype(np.uint8)
    for ramp in _ramps(p):
        win = np.ascontiguousarray(np.moveaxis(tr.cut(img, p.ys, p.xs, tile), 0, 1))     # [N, T, 3, th, tw]
        assert win.shape == (2, p.T, 3) + tile
        got, mx = tr.merge(win, hw, p.ys, p.xs, ramp)
        assert np.array_equal(got, img), (hw, tile, ramp)
        assert mx.tolist() == img.reshape(2, -1).max(1).tolist()
        for v in (0, 1, 127, 255):
            got, mx = tr.merge(np.full_like(win, v), hw, p.ys, p.xs, ramp)
            assert (got == v).all() and mx.tolist() == [v, v]
    one = rs.randint(0, 256, (3, 1, 3) + tile).astype(np.uint8)
    got, mx = tr.merge(one, tile, [0], [0], 1)
    assert np.array_equal(got, one[:, 0]) and mx.tolist() == one.reshape(3, -1).max(1).tolist()


def test_reference_rounds_half_up():
    """Two windows of 8 x 8 on 8 x 9 overlap in columns 1..7; with ramp 1 the merged byte is the mean of the two, and an odd
    sum rounds UP: (255 + 0 + 1) // 2 = 128, (1 + 0 + 1) // 2 = 1, never 127 / 0."""
    p = _plan((8, 9), (8, 8), 0)
    assert p.xs == [0, 1]
    win = np.zeros((1, 2, 3, 8, 8), np.uint8)
    win[0, 0] = 255
    got, mx = tr.merge(win, (8, 9), p.ys, p.xs, 1)
    assert (got[0, :, :, 0] == 255).all() and (got[0, :, :, 1:8] == 128).all() and (got[0, :, :, 8] == 0).all()
    win[0, 0] = 1
    got, _ = tr.merge(win, (8, 9), p.ys, p.xs, 1)
    assert (got[0, :, :, 1:8] == 1).all()


def test_dim_window_separates_the_two_maximum_rules():
    """Two windows side by side, one whose bytes never exceed 10 and one that reaches 200.  The dynamic threshold taken PER
    WINDOW (r_threshold * that window's maximum) calls pixels of the dim window foreground; taken once on the merged image
    (r_threshold * 200 / 255) it calls none of them, and keeps the bright window's object."""
    p = _plan((8, 16), (8, 8), 0)
    assert (p.ys, p.xs) == ([0], [0, 8])
    rs = np.random.RandomState(3)
    win = np.zeros((1, 2, 3, 8, 8), np.uint8)
    win[0, 0] = rs.randint(0, 11, (3, 8, 8))
    win[0, 0, :, 0, 0] = 10
    win[0, 1, :, 2:6, 2:6] = 200
    per_window = nway_ref.labels(torch.from_numpy(win))                        # B = the two windows, each its own maximum
    assert int(per_window[0].sum()) >= 1                                       # noise foreground in the dim window
    merged, mx = tr.merge(win, (8, 16), p.ys, p.xs, p.ramp)
    assert mx.tolist() == [200]
    lab = nway_ref.labels(torch.from_numpy(merged)[:, None])[0]                # [8, 16], one maximum for the image
    assert int(lab[:, :8].sum()) == 0
    assert torch.equal(lab[:, 8:], per_window[1]) and int(lab[:, 8:].sum()) == 16


# ------------------------------------------------------------------------------------------------ the C ABI

def test_header_ctypes_and_symbols(hip_lib):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int dfw_tiles_cut(const dfw_tile_plan* plan, const uint8_t* img, const float* lut, float* out, int32_t first, "
            "int32_t count, dfw_stream_t stream);") in flat
    assert ("int dfw_tiles_merge(const dfw_tile_plan* plan, const uint8_t* win, int32_t N, uint8_t* out, uint32_t* mx, "
            "dfw_stream_t stream);") in flat
    i32, vp = C.c_int32, C.c_void_p
    assert L.SYMBOLS["dfw_tiles_cut"] == (i32, [C.POINTER(L.TilePlan), vp, vp, vp, i32, i32, vp])
    assert L.SYMBOLS["dfw_tiles_merge"] == (i32, [C.POINTER(L.TilePlan), vp, i32, vp, vp, vp])
    for name in ("dfw_tiles_cut", "dfw_tiles_merge"):
        assert getattr(hip_lib, name) is not None
    assert hip_lib.dfw_version() >= 108


def test_tile_plan_struct_matches_header_and_compiler(tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\}\s*dfw_tile_plan;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        names += [re.sub(r"\[\d+\]", "", x) for x in decl.replace(",", " ").split() if x != "int32_t"]
    assert names == [f[0] for f in L.TilePlan._fields_] == ["img_h", "img_w", "tile_h", "tile_w", "ny", "nx", "ramp", "ys", "xs"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\nint main(){printf("%zu %d", sizeof(dfw_tile_plan), '
                   '(int)DFW_TILE_MAX_ORIGINS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [C.sizeof(L.TilePlan), 64]
    from diffews_amd.input_pipeline import TilePlan
    assert TilePlan.MAX_ORIGINS == 64 and C.sizeof(L.TilePlan) == 4 * (7 + 128)
    c = TilePlan((19, 37), (8, 16), 2, ramp=3).c_struct()
    assert (c.img_h, c.img_w, c.tile_h, c.tile_w, c.ny, c.nx, c.ramp) == (19, 37, 8, 16, 3, 3, 3)
    assert list(c.ys[:3]) == [0, 5, 11] and list(c.xs[:3]) == [0, 10, 21] and not any(c.ys[3:]) and not any(c.xs[3:])


def _valid_args(N=2):
    """Fully valid dfw_tiles_cut / dfw_tiles_merge calls on host memory (never launched: every test below breaks one
    thing): tile 8 x 16 on 19 x 37, three windows per axis."""
    from diffews_amd.input_pipeline import TilePlan
    p = TilePlan((19, 37), (8, 16), 2)
    keep = dict(img=np.zeros((19, 37, 3), np.uint8), lut=np.zeros(256, np.float32), q=np.zeros((p.T, 3, 8, 16), np.float32),
                win=np.zeros((N, p.T, 3, 8, 16), np.uint8), out=np.zeros((N, 3, 19, 37), np.uint8), mx=np.zeros(N, np.uint32))
    ptr = {k: v.ctypes.data for k, v in keep.items()}
    cut = dict(plan=p.c_struct(), img=ptr["img"], lut=ptr["lut"], out=ptr["q"], first=0, count=p.T)
    merge = dict(plan=p.c_struct(), win=ptr["win"], N=N, out=ptr["out"], mx=ptr["mx"])
    return cut, merge, keep


def _cut(lib, a):
    return lib.dfw_tiles_cut(C.byref(a["plan"]) if a["plan"] is not None else None, a["img"], a["lut"], a["out"], a["first"],
                             a["count"], None)


def _merge(lib, a):
    return lib.dfw_tiles_merge(C.byref(a["plan"]) if a["plan"] is not None else None, a["win"], a["N"], a["out"], a["mx"], None)


def _break_plan(name):
    def f(p):
        if name == "ny=0": p.ny = 0
        elif name == "ny=65": p.ny = 65
        elif name == "nx=0": p.nx = 0
        elif name == "nx=65": p.nx = 65
        elif name == "first origin not 0": p.ys[0] = 1
        elif name == "last origin not image - tile": p.xs[2] = 20
        elif name == "last origin past the image": p.ys[2] = 12
        elif name == "origins not ascending": p.xs[1] = 0
        elif name == "origins descending": p.ys[1] = 12
        elif name == "a gap wider than the tile": p.ys[1] = 2          # 2 -> 11: 9 rows apart, tile_h = 8
        elif name == "a gap wider than the tile (x)": p.xs[1] = 4      # 4 -> 21: 17 columns apart, tile_w = 16
        elif name == "ramp=0": p.ramp = 0
        elif name == "ramp above half the short side": p.ramp = 5
        elif name == "tile taller than the image": p.tile_h = 20
        elif name == "tile_w=0": p.tile_w = 0
        elif name == "img_h=0": p.img_h = 0
        elif name == "one window on an image larger than the tile": p.ny = 1
        else: raise KeyError(name)
    return f


PLAN_BREAKS = ["ny=0", "ny=65", "nx=0", "nx=65", "first origin not 0", "last origin not image - tile",
               "last origin past the image", "origins not ascending", "origins descending", "a gap wider than the tile",
               "a gap wider than the tile (x)", "ramp=0", "ramp above half the short side", "tile taller than the image",
               "tile_w=0", "img_h=0", "one window on an image larger than the tile"]


def test_tiles_validate_on_the_host_before_any_launch(hip_lib):
    """Each break of one field of an otherwise valid call returns DFW_EINVAL from the host-side checks (these buffers are
    host memory and the stream is null: nothing may be launched)."""
    for field in ("plan", "img", "lut", "out"):
        cut, _, keep = _valid_args()
        cut[field] = None
        assert _cut(hip_lib, cut) == EINVAL, field
    for field in ("plan", "win", "out", "mx"):
        _, merge, keep = _valid_args()
        merge[field] = None
        assert _merge(hip_lib, merge) == EINVAL, field
    for name in PLAN_BREAKS:
        cut, merge, keep = _valid_args()
        _break_plan(name)(cut["plan"])
        _break_plan(name)(merge["plan"])
        assert _cut(hip_lib, cut) == EINVAL, name
        assert _merge(hip_lib, merge) == EINVAL, name
    for first, count in ((-1, 1), (0, 0), (0, -3), (0, 10), (9, 1), (5, 5), (2 ** 31 - 1, 2)):
        cut, _, keep = _valid_args()
        cut["first"], cut["count"] = first, count
        assert _cut(hip_lib, cut) == EINVAL, (first, count)
    for N in (0, -1, 255, 1000):
        _, merge, keep = _valid_args()
        merge["N"] = N
        assert _merge(hip_lib, merge) == EINVAL, N


def test_merge_refuses_a_plan_whose_sums_are_not_proven_to_fit(hip_lib):
    """The merge sums in 32 bits and launches only where 511 * (windows over a pixel) * ramp^2 < 2^32: three 4096-row windows
    1024 apart with ramp 2048 are refused (DFW_ERANGE, on the host); with ramp 1024 the bound holds and the next check is
    reached (a null mx: DFW_EINVAL comes first, so this call cannot launch either)."""
    from diffews_amd import _lib as L
    p = L.TilePlan()
    p.img_h, p.img_w, p.tile_h, p.tile_w, p.ny, p.nx, p.ramp = 6144, 4096, 4096, 4096, 3, 1, 2048
    p.ys[:3] = [0, 1024, 2048]
    buf = np.zeros(16, np.uint8).ctypes.data
    assert hip_lib.dfw_tiles_merge(C.byref(p), buf, 1, buf, buf, None) == -3
    assert hip_lib.dfw_tiles_merge(C.byref(p), buf, 1, buf, None, None) == EINVAL
