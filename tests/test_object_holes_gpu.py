"""GPU tests of the hole-filling stage (ops.seg_holes, csrc/seg_holes.hip) against tests/holes_ref.py, exact.

The tile of the union-find is 32 x 64 (dfw_seg_components_tile); the shapes are the smallest at which each path can go
wrong: one tile, holes across a vertical, a horizontal and a four-tile border, W % 4 != 0, H or W below 3, regions that
touch the frame at one side or one pixel only, and the first pixel at x = 0 behind an object pixel.  Every case is a batch
of two different images at both connectivities, launched into guarded buffers pre-filled with a byte pattern.  The second
grid-stride trip of the flatten pass is reached at 2049 x 2048 and 2120 x 2048 on a mosaic of cells whose holes are decided
cell by cell with the per-pixel search.  The merge pass wraps only above about 22 M pixels, which no test of a few seconds
reaches (as for dfw_seg_components); the three kernels behind the flatten pass do not loop over a capped grid."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import boundary_ref as br
import components_ref as cr
import holes_ref as hr
import match_ref as mr
import mosaic_ref as mo
import object_rounds_cases as oc
import rle_ref as rr

pytestmark = pytest.mark.gpu

SENT = 0xA5
FILL = 0x5A
NLAB = 3
u8, i32 = torch.uint8, torch.int32


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def tile(hip_lib):
    th, tw = C.c_int32(), C.c_int32()
    assert hip_lib.dfw_seg_components_tile(C.byref(th), C.byref(tw)) == 0
    assert (th.value, tw.value) == (32, 64)                               # the coordinates below are written for this tile
    return th.value, tw.value


class _Guarded:
    """A tensor inside a flat allocation with `pad` sentinel elements (0xA5 bytes / -7 words) on either side, itself
    pre-filled with `fill` bytes."""

    def __init__(self, shape, dtype, pad, fill=None):
        n = int(np.prod(shape))
        self.sent = SENT if dtype == u8 else -7
        self.flat = torch.full((n + 2 * pad,), self.sent, dtype=dtype, device="cuda")
        self.t = self.flat[pad:pad + n].view(shape)
        self.pad, self.n = pad, n
        if fill is not None:
            self.t.view(u8).fill_(fill)

    def check(self, name):
        assert (self.flat[:self.pad] == self.sent).all() and (self.flat[self.pad + self.n:] == self.sent).all(), f"wrote outside {name}"


def _put(g, a):
    g.t.copy_(torch.from_numpy(np.array(a)))
    return g


KEYS = ("ids", "labels", "holes", "stats", "counts")


def _launch(ops, labels, ids, conn, max_area=None, stats=None, gt=None, fill=FILL, off=0, bufs=None, repeat=1):
    """ops.seg_holes on numpy maps into guarded, pre-filled buffers -> (numpy results, the buffers).  off: words by which
    ids, both id outputs and the workspace lie off a 16-byte boundary, and 3 * off bytes by which the byte maps do."""
    B, H, W = labels.shape
    wpad, bpad = 4 + off, 64 + 3 * off
    if bufs is None:
        bufs = dict(labels=_Guarded((B, H, W), u8, bpad), ids=_Guarded((B, H, W), i32, wpad),
                    ids_out=_Guarded((B, H, W), i32, wpad, fill), labels_out=_Guarded((B, H, W), u8, bpad, fill),
                    holes=_Guarded((B, 2), i32, 4, fill), ws=_Guarded((ops.seg_holes_workspace(B, H, W),), u8, 64 + 4 * off, fill))
        if stats is not None:
            bufs["stats"] = _Guarded(stats.shape, i32, 4)
            bufs["stats_out"] = _Guarded(stats.shape, i32, 4, fill)
        if gt is not None:
            bufs["gt"] = _Guarded((B, H, W), u8, bpad)
            bufs["counts"] = _Guarded((B, 2, NLAB + 1), torch.int64, 2, fill)
        assert bufs["ids_out"].t.data_ptr() % 16 == 4 * off % 16 and bufs["ws"].t.data_ptr() % 16 == 4 * off % 16
    _put(bufs["labels"], labels)
    _put(bufs["ids"], ids)
    if stats is not None:
        _put(bufs["stats"], stats)
    if gt is not None:
        _put(bufs["gt"], gt)
    g = {k: v.t for k, v in bufs.items()}
    for _ in range(repeat):
        ops.seg_holes(g["labels"], g["ids"], g["ids_out"], g["labels_out"], g["holes"], g["ws"], stats=g.get("stats"),
                      stats_out=g.get("stats_out"), gt=g.get("gt"), counts=g.get("counts"), connectivity=conn, max_area=max_area,
                      nlabels=NLAB if gt is not None else None)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert np.array_equal(g["labels"].cpu().numpy(), labels) and np.array_equal(g["ids"].cpu().numpy(), ids), "an input was modified"
    if stats is not None:
        assert np.array_equal(g["stats"].cpu().numpy(), stats), "stats was modified"
    got = dict(ids=g["ids_out"], labels=g["labels_out"], holes=g["holes"], stats=g.get("stats_out"), counts=g.get("counts"))
    return {k: (None if v is None else v.cpu().numpy()) for k, v in got.items()}, bufs


def _same(got, want, what):
    for k in KEYS:
        if got[k] is None:
            continue
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), \
            (what, k, int((got[k] != want[k]).sum()), got["holes"].tolist(), want["holes"].tolist())


def _gt(shape, rs):
    """0..NLAB, some 255 (ignore) and some bytes above NLAB that have no bin."""
    g = rs.randint(0, NLAB + 1, shape).astype(np.uint8)
    g[rs.rand(*shape) < 0.05] = 255
    g[rs.rand(*shape) < 0.05] = NLAB + 2
    return g


def _check(ops, labels, conn, max_area=None, min_area=0, cap=64, with_gt=True, what="", expect=None, **kw):
    """labels -> the objects by the flood fill -> seg_holes against the reference.  expect: the holes table to find."""
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    comp = cr.components(labels, conn, min_area, cap)
    gt = _gt(labels.shape, np.random.RandomState(labels.shape[1] * 1000 + labels.shape[2])) if with_gt else None
    want = hr.holes(comp["filtered"], comp["ids"], conn, max_area, comp["stats"], gt, NLAB)
    if expect is not None:
        assert want["holes"].tolist() == expect, (what, want["holes"].tolist())
    got, bufs = _launch(ops, comp["filtered"], comp["ids"], conn, max_area, comp["stats"], gt, **kw)
    _same(got, want, (what, conn, max_area))
    return got, want, comp, bufs


def _noise(H, W, density, rs, classes=2):
    return ((rs.rand(H, W) < density) * rs.randint(1, classes + 1, (H, W))).astype(np.uint8)


def _solid(H, W, cls=1, margin=1):
    lab = np.zeros((H, W), np.uint8)
    lab[margin:H - margin, margin:W - margin] = cls
    return lab


# ------------------------------------------------------------------------------------------------ the smallest shapes

@pytest.mark.parametrize("conn", (4, 8))
def test_three_by_three_and_maps_without_an_interior(ops, tile, conn):
    hole = np.ones((3, 3), np.uint8)
    hole[1, 1] = 0
    other = np.full((3, 3), 2, np.uint8)
    other[1, 1], other[0, 0] = 0, 0                                       # the corner is open; at conn 4 the centre leaks to it
    got, want, _, _ = _check(ops, np.stack([hole, other]), conn, what="3x3", expect=[[1, 1], [1, 1]] if conn == 8 else [[1, 1], [0, 0]])
    assert (got["labels"][0] == 1).all() and got["stats"][0, 0, 1] == 9 and got["stats"][0, 0, 7] == 1
    rs = np.random.RandomState(2)
    for H, W in ((1, 1), (1, 9), (2, 9), (9, 1), (9, 2), (2, 2), (1, 64), (33, 1), (2, 68)):
        labs = np.stack([_noise(H, W, 0.6, rs), _noise(H, W, 0.6, rs)])
        got, want, comp, _ = _check(ops, labs, conn, what=(H, W), expect=[[0, 0], [0, 0]])
        assert np.array_equal(got["ids"], comp["ids"]) and np.array_equal(got["labels"], labs)


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("shape", [(37, 71), (40, 72), (33, 65), (67, 133)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_maps_against_the_reference(ops, tile, conn, shape):
    """Dense noise of two classes, full of holes of every kind, on one, two and nine tiles, W % 4 == 0 and not."""
    H, W = shape
    rs = np.random.RandomState(H * W + conn)
    labs = np.stack([_noise(H, W, 0.85, rs), _noise(H, W, 0.7, rs, 1)])
    for max_area, min_area in ((None, 0), (2, 0), (None, 3)):
        got, want, _, _ = _check(ops, labs, conn, max_area, min_area, cap=2048, what=shape)
        assert want["holes"][:, 0].sum() > 0                                # the maps do have holes that are filled


# ------------------------------------------------------------------------------------------------ tile borders

def _holes_at(H, W, boxes, cls=1):
    lab = _solid(H, W, cls)
    for y0, x0, y1, x1 in boxes:
        lab[y0:y1, x0:x1] = 0
    return lab


BORDER_BOXES = {"inside one tile": (5, 5, 9, 12), "across x = 63 | 64": (10, 60, 13, 69), "across y = 31 | 32": (29, 20, 36, 24),
                "over the four-tile corner": (30, 61, 35, 67)}


@pytest.mark.parametrize("conn", (4, 8))
def test_holes_inside_and_across_tiles(ops, tile, conn):
    H, W = 70, 140
    for name, box in BORDER_BOXES.items():
        labs = np.stack([_holes_at(H, W, [box]), _holes_at(H, W, [box, (50, 100, 52, 139)], 2)])     # image 1: one leaks at x = W - 1
        got, _, _, _ = _check(ops, labs, conn, what=name, expect=[[1, 1], [1, 1]])
        area = (box[2] - box[0]) * (box[3] - box[1])
        assert got["stats"][0, 0, 7] == area and (got["labels"][0, 1:-1, 1:-1] == 1).all()
    every = list(BORDER_BOXES.values())
    labs = np.stack([_holes_at(H, W, every), _holes_at(H, W, every[::2], 3)])
    _check(ops, labs, conn, what="all four", expect=[[4, 4], [2, 2]])
    _check(ops, labs, conn, 27, what="all four, max_area", expect=[[1, 4], [0, 2]])      # areas 28, 27, 28, 30 / 28, 28


def test_two_halves_joined_by_one_diagonal(ops, tile):
    """Background in the corner of tile (0, 0) and in the opposite corner of tile (1, 1), touching only over the diagonal
    (31, 63) - (32, 64): one region for 4-connected objects (the background joins over 8), two for 8-connected ones."""
    a, b = (20, 50, 32, 64), (32, 64, 41, 76)
    labs = np.stack([_holes_at(64, 128, [a, b]), _holes_at(64, 128, [a, b, (0, 70, 33, 71)], 2)])    # image 1: b is open
    got4, _, _, _ = _check(ops, labs, 4, what="diagonal", expect=[[1, 1], [0, 0]])
    got8, _, _, _ = _check(ops, labs, 8, what="diagonal", expect=[[2, 2], [1, 1]])
    assert got4["stats"][0, 0, 7] == got8["stats"][0, 0, 7] == 12 * 14 + 9 * 12
    _check(ops, labs, 4, 12 * 14 + 9 * 12 - 1, what="diagonal, one pixel too large", expect=[[0, 1], [0, 0]])
    _check(ops, labs, 8, 12 * 14 - 1, what="diagonal, the smaller half", expect=[[1, 2], [0, 1]])


@pytest.mark.parametrize("conn", (4, 8))
def test_a_ring_around_one_hole_over_many_tiles(ops, tile, conn):
    """100 x 200 with a ring three pixels wide: the hole's 94 x 194 pixels reach the owner's row from 28 tiles."""
    ring = np.zeros((104, 208), np.uint8)
    ring[2:102, 4:204] = 2
    ring[5:99, 7:201] = 0
    broken = ring.copy()
    broken[50, 201:204] = 0                                                # image 1: the ring is cut, the hole is open
    got, _, _, _ = _check(ops, np.stack([ring, broken]), conn, what="ring", expect=[[1, 1], [0, 0]])
    assert got["stats"][0, 0].tolist() == [2, 100 * 200, 2, 4, 102, 204, 2 * 208 + 4, 94 * 194]
    assert (got["ids"][0, 2:102, 4:204] == 1).all() and np.array_equal(got["labels"][1], broken)
    _check(ops, np.stack([ring, broken]), conn, 94 * 194 - 1, what="ring, max_area", expect=[[0, 1], [0, 0]])
    _check(ops, np.stack([ring, broken]), conn, 94 * 194, what="ring, max_area", expect=[[1, 1], [0, 0]])


# ------------------------------------------------------------------------------------------------ the frame

@pytest.mark.parametrize("conn", (4, 8))
def test_regions_that_touch_the_frame_stay(ops, tile, conn):
    """Each region touches the frame at one side or one pixel only.  (10, 0) is a first pixel on column 0 whose index - 1
    is (9, W - 1), an object pixel: read as an owner it would fill the region."""
    H, W = 40, 72
    full = np.ones((H, W), np.uint8)
    assert full[9, W - 1] == 1
    cuts = {"column 0": (10, 0, 11, 4), "last column": (20, W - 4, 21, W), "last row": (H - 3, 30, H, 31), "row 0": (0, 50, 2, 51),
            "the corner pixel": (H - 1, W - 1, H, W), "pixel (0, 0)": (0, 0, 1, 1), "an inner pixel of column 0": (H - 2, 0, H - 1, 1)}
    for name, (y0, x0, y1, x1) in cuts.items():
        one, both = full.copy(), full.copy()
        one[y0:y1, x0:x1] = 0
        both[y0:y1, x0:x1] = 0
        both[15:18, 30:33] = 0                                              # image 1 also has a real hole
        got, _, _, _ = _check(ops, np.stack([one, both]), conn, what=name, expect=[[0, 0], [1, 1]])
        assert np.array_equal(got["labels"][0], one)
    # a region that reaches the frame only through a diagonal step: open for 4-connected objects, closed for 8-connected
    diag = full.copy()
    diag[H - 2, W - 2] = diag[H - 1, W - 1] = 0
    left = full.copy()
    left[21, 1] = left[22, 0] = 0
    _check(ops, np.stack([diag, left]), conn, what="diagonal to the corner", expect=[[0, 0], [0, 0]] if conn == 4 else [[1, 1], [1, 1]])


# ------------------------------------------------------------------------------------------------ ownership

def test_two_owners_islands_and_ids_above_cap(ops, tile):
    from test_object_holes_cpu import SAME_CLASS
    two = np.zeros((12, 20), np.uint8)
    two[2:10, 2:10], two[2:10, 10:18] = 1, 2
    two[4:8, 6:14] = 0                                                     # one hole between an object of class 1 and one of class 2
    isl = _solid(12, 20)
    isl[3:9, 4:16] = 0
    isl[5:7, 8:10] = 2                                                     # an island of four pixels inside the hole
    _check(ops, np.stack([two, isl]), 8, what="two owners / island", expect=[[0, 1], [0, 1]])
    _check(ops, np.stack([two, isl]), 4, what="two owners / island", expect=[[0, 1], [0, 1]])
    got, _, _, _ = _check(ops, np.stack([two, isl]), 8, min_area=5, what="island removed first", expect=[[0, 1], [1, 1]])
    assert got["stats"][1, 0, 7] == 6 * 12 and (got["labels"][1, 1:-1, 1:-1] == 1).all()
    same = np.zeros((12, 20), np.uint8)
    same[3:8, 5:12] = SAME_CLASS
    _check(ops, np.stack([same, same[::-1].copy()]), 4, what="one class, two objects", expect=[[0, 1], [0, 1]])
    # the owner's id above cap: ids and labels are filled, its stats row does not exist
    lab = np.zeros((12, 20), np.uint8)
    lab[0, 0], lab[0, 2] = 3, 3                                            # ids 1 and 2
    lab[3:10, 3:17] = 1                                                    # id 3
    lab[5:7, 6:9] = 0
    got, want, comp, _ = _check(ops, np.stack([lab, lab[:, ::-1].copy()]), 8, cap=2, what="above cap", expect=[[1, 1], [1, 1]])
    assert np.array_equal(got["stats"], comp["stats"]) and (got["ids"][0, 5:7, 6:9] == 3).all() and (got["labels"][0, 5:7, 6:9] == 1).all()
    # without stats, and without a ground truth
    c = cr.components(np.stack([lab, isl]), 8, 0, 8)
    got, _ = _launch(ops, c["filtered"], c["ids"], 8)
    _same(got, hr.holes(c["filtered"], c["ids"], 8), "no stats, no gt")
    assert got["stats"] is None and got["counts"] is None and got["holes"].tolist() == [[1, 1], [0, 1]]
    # labels that the id map does not cover: the owner is 0
    got, _ = _launch(ops, c["filtered"], np.zeros_like(c["ids"]), 8)
    assert got["holes"].tolist() == [[0, 1], [0, 1]] and np.array_equal(got["labels"], c["filtered"]) and not got["ids"].any()


@pytest.mark.parametrize("conn", (4, 8))
def test_max_area_at_the_area(ops, tile, conn):
    lab = _holes_at(40, 80, [(4, 4, 7, 9), (20, 60, 22, 70), (30, 30, 31, 31)])         # 15, 20 and 1 pixels
    labs = np.stack([lab, lab[::-1].copy()])
    for max_area, filled in ((0, 0), (1, 1), (14, 1), (15, 2), (19, 2), (20, 3), (None, 3), (2 ** 31 - 1, 3)):
        _check(ops, labs, conn, max_area, what=("max_area", max_area), expect=[[filled, 3], [filled, 3]])


# ------------------------------------------------------------------------------------------------ buffers and launches

@pytest.mark.parametrize("off", (1, 2, 3))
def test_buffers_off_their_alignment(ops, tile, off):
    """ids, ids_out and the workspace 1 to 3 words behind a 16-byte boundary, the byte maps 3 to 9 bytes: the scalar paths
    at a width that would take the vector paths."""
    rs = np.random.RandomState(off)
    labs = np.stack([_noise(67, 136, 0.85, rs), _holes_at(67, 136, list(BORDER_BOXES.values()))])
    for conn in (4, 8):
        _check(ops, labs, conn, cap=2048, what=("off", off), off=off)


def test_poisoned_repeated_and_reused_launches(ops, tile):
    rs = np.random.RandomState(29)
    H, W = 65, 132
    labs = np.stack([_noise(H, W, 0.85, rs), _holes_at(H, W, list(BORDER_BOXES.values()))])
    for fill in (0xFF, 0x7B, 0x00):
        got, want, comp, bufs = _check(ops, labs, 8, cap=2048, what=hex(fill), fill=fill)
    gt = _gt(labs.shape, np.random.RandomState(H * 1000 + W))
    again, _ = _launch(ops, comp["filtered"], comp["ids"], 8, None, comp["stats"], gt, bufs=bufs, repeat=2)
    _same(again, want, "back to back")
    other = np.stack([_noise(H, W, 0.7, rs, 1), np.zeros((H, W), np.uint8)])           # the same buffers, another map
    c = cr.components(other, 4, 0, 2048)
    got, _ = _launch(ops, c["filtered"], c["ids"], 4, 3, c["stats"], gt, bufs=bufs)
    _same(got, hr.holes(c["filtered"], c["ids"], 4, 3, c["stats"], gt, NLAB), "reused buffers")


def test_hole_buffers_reused_over_two_inputs(ops, tile):
    from diffews_amd.objects import ComponentBuffers, HoleBuffers, fill_holes, label_objects, objects_to_host
    rs = np.random.RandomState(5)
    B, H, W, cap = 2, 45, 70, 512
    cb, hb = ComponentBuffers(B, H, W, cap), HoleBuffers(B, H, W, cap)
    gt = _gt((B, H, W), rs)
    gtd = torch.from_numpy(gt).cuda()
    for trial, min_area in enumerate((0, 4)):
        labs = np.stack([_noise(H, W, 0.85, rs), _noise(H, W, 0.75, rs, 1)])
        o = label_objects(torch.from_numpy(labs).cuda(), connectivity=8, min_area=min_area, buffers=cb)
        r = fill_holes(o, max_area=40, gt=gtd, nlabels=NLAB, buffers=hb)
        assert r["ids"] is hb.ids and r["n"] is o["n"] and r["counts"] is hb.counts(NLAB)
        comp = cr.components(labs, 8, min_area, cap)
        want = hr.holes(comp["filtered"], comp["ids"], 8, 40, comp["stats"], gt, NLAB)
        _same({k: r[k].cpu().numpy() for k in KEYS}, want, ("HoleBuffers", trial))
        assert want["holes"][:, 0].min() > 0
        objs, truncated = objects_to_host(r)
        assert not truncated and [o_[1] for o_ in objs[0]] == want["stats"][0, :len(objs[0]), 1].tolist()
    one = fill_holes({k: (None if v is None else v[1]) for k, v in o.items()}, max_area=40)          # [H, W]: no batch axis
    assert one["ids"].shape == (H, W) and one["holes"].shape == (2,) and one["counts"] is None
    assert np.array_equal(one["ids"].cpu().numpy(), want["ids"][1]) and one["holes"].tolist() == want["holes"][1].tolist()
    lists = {k: [v[0], v[1]] for k, v in o.items() if v is not None}
    per = fill_holes(lists, max_area=40)                                   # a list result: one call per item
    assert [h.tolist() for h in per["holes"]] == want["holes"].tolist() and per["counts"] == [None, None]
    assert np.array_equal(per["labels"][0].cpu().numpy(), want["labels"][0])
    with pytest.raises(ValueError, match="buffers were made for"):
        fill_holes(o, buffers=HoleBuffers(B, H, W, cap + 1))


def test_guarded_poisoned_bit_equal_launches(ops, tile):
    """tests/launch_guard.py over ops.seg_holes: the wrapper allocates nothing, so every buffer is the call's own --
    placed inputs, guarded outputs and workspace filled with 0xFF and with 0x7B -- and the outputs are bit-equal."""
    import launch_guard as lg
    rs = np.random.RandomState(41)
    labs = np.stack([_noise(66, 130, 0.85, rs), _holes_at(66, 130, list(BORDER_BOXES.values()))])
    comp = cr.components(labs, 8, 2, 300)
    gt = _gt(labs.shape, rs)
    dev = "cuda"
    lab_d, ids_d, st_d, gt_d = [torch.from_numpy(a).to(dev) for a in (comp["filtered"], comp["ids"], comp["stats"], gt)]
    B, H, W = labs.shape

    def call(run):
        out = dict(ids=run.empty(B, H, W, dtype=i32, device=dev), labels=run.empty(B, H, W, dtype=u8, device=dev),
                   holes=run.empty(B, 2, dtype=i32, device=dev), stats=run.empty(B, 300, 8, dtype=i32, device=dev),
                   counts=run.empty(B, 2, NLAB + 1, dtype=torch.int64, device=dev))
        ws = run.empty(ops.seg_holes_workspace(B, H, W), dtype=u8, device=dev)
        ops.seg_holes(run.place(lab_d), run.place(ids_d), out["ids"], out["labels"], out["holes"], ws, stats=run.place(st_d),
                      stats_out=out["stats"], gt=run.place(gt_d), counts=out["counts"], connectivity=8, max_area=50, nlabels=NLAB)
        return out
    lg.check_launches([ops], call)
    want = hr.holes(comp["filtered"], comp["ids"], 8, 50, comp["stats"], gt, NLAB)
    _same({k: v.cpu().numpy() for k, v in call(lg.Plain()).items()}, want, "plain")


def test_captured_launch_follows_the_inputs(ops, hip_lib, tile):
    """seg_components -> seg_holes in one torch.cuda.graph: no memset node, 8 + 6 kernel nodes, and each replay fills the
    holes of whatever the label tensor holds."""
    from diffews_amd.objects import ComponentBuffers, HoleBuffers
    rs = np.random.RandomState(31)
    B, H, W, cap = 2, 41, 136, 1024
    maps = [np.stack([_noise(H, W, 0.85, rs), _holes_at(H, W, list(BORDER_BOXES.values()))]),
            np.stack([_noise(H, W, 0.7, rs, 1), _noise(H, W, 0.9, rs)])]
    gt = _gt((B, H, W), rs)
    cb, hb = ComponentBuffers(B, H, W, cap), HoleBuffers(B, H, W, cap)
    lab = torch.zeros(B, H, W, dtype=u8, device="cuda")
    gtd, counts = torch.from_numpy(gt).cuda(), hb.counts(NLAB)

    def call():
        ops.seg_components(lab, cb.ids, cb.n, cb.ws, filtered=cb.labels, stats=cb.stats, connectivity=8, min_area=2)
        ops.seg_holes(cb.labels, cb.ids, hb.ids, hb.labels, hb.holes, hb.ws, stats=cb.stats, stats_out=hb.stats, gt=gtd,
                      counts=counts, connectivity=8, max_area=60, nlabels=NLAB)
    call()                                                                 # modules loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    nodes = C.c_int32()
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0
    assert nodes.value == 8 + 6
    graph.instantiate()
    for m in maps + maps[:1]:
        lab.copy_(torch.from_numpy(m))
        graph.replay()
        torch.cuda.synchronize()
        comp = cr.components(m, 8, 2, cap)
        want = hr.holes(comp["filtered"], comp["ids"], 8, 60, comp["stats"], gt, NLAB)
        _same(dict(ids=hb.ids.cpu().numpy(), labels=hb.labels.cpu().numpy(), holes=hb.holes.cpu().numpy(),
                   stats=hb.stats.cpu().numpy(), counts=counts.cpu().numpy()), want, "replay")
        assert want["holes"][:, 0].min() > 0


def test_the_chain_behind_the_filled_objects(ops, tile):
    """label_objects(min_area) -> fill_holes -> object_runs / match_objects / object_boundaries on a 96 x 160 map: the
    later stages take the filled result as it is, and give what their references give on the reference's filled maps."""
    from diffews_amd.objects import (MatchBuffers, RunBuffers, fill_holes, label_objects, match_objects, object_boundaries,
                                     object_runs)
    rs = np.random.RandomState(17)
    B, H, W, cap, min_area = 2, 96, 160, 256, 6
    truth = np.stack([mr.blobs(H, W, rs), mr.blobs(H, W, rs)])
    pred = truth.copy()
    pred[(rs.rand(B, H, W) < 0.04) & (pred > 0)] = 0                       # pinholes
    specks = rs.rand(B, H, W) < 0.01
    pred[specks] = 1 + (pred[specks] % NLAB)                               # specks of another class, inside objects and outside
    o = label_objects(torch.from_numpy(pred).cuda(), connectivity=8, min_area=min_area, max_components=cap)
    og = label_objects(torch.from_numpy(truth).cuda(), connectivity=8, max_components=cap)
    r = fill_holes(o, max_area=30)
    comp, cg = cr.components(pred, 8, min_area, cap), cr.components(truth, 8, 0, cap)
    want = hr.holes(comp["filtered"], comp["ids"], 8, 30, comp["stats"])
    _same({k: (None if r[k] is None else r[k].cpu().numpy()) for k in KEYS}, want, "chain")
    assert want["holes"][:, 0].min() > 20 and (want["holes"][:, 1] > want["holes"][:, 0]).all()
    assert int(comp["n"][:, 0].max()) <= cap
    runs = object_runs(r, order="column", buffers=RunBuffers(B, H, W, cap, 1 << 13, "column"))
    wr = rr.rle(want["ids"], cap, 1 << 13, "column")
    assert np.array_equal(runs["nruns"].cpu().numpy(), wr["nruns"]) and np.array_equal(runs["run_off"].cpu().numpy(), wr["run_off"])
    for b in range(B):
        assert np.array_equal(runs["runs"][b, :len(wr["runs"][b])].cpu().numpy(), wr["runs"][b])
    holed = rr.rle(comp["ids"], cap, 1 << 13, "column")
    assert (holed["nruns"][:, 1] > wr["nruns"][:, 1]).all()               # the holes did split runs
    m = match_objects(r, og, nlabels=NLAB, buffers=MatchBuffers(B, H, W, cap, cap, NLAB, 1 << 13, 1 << 12))
    wm = mr.match(want["ids"], cg["ids"], cap, cap, NLAB, 1 << 13, 1 << 12, pstats=want["stats"], gstats=cg["stats"])
    for k in ("n", "pair_off", "area", "match", "gmatch", "pq"):
        assert np.array_equal(m[k].cpu().numpy(), wm[k]), k
    for b in range(B):
        assert np.array_equal(m["pairs"][b, :len(wm["pairs"][b])].cpu().numpy(), wm["pairs"][b])
    bands = object_boundaries(r, d=3)
    for key in ("labels", "ids"):
        dist = br.dist_ref(want[key], 3)
        assert np.array_equal(bands[key]["dist"].cpu().numpy(), dist)
        assert np.array_equal(bands[key]["band"].cpu().numpy(), br.band_ref(want[key], dist, 3))
    assert (br.dist_ref(comp["filtered"], 3) == 1).sum() > (br.dist_ref(want["labels"], 3) == 1).sum()   # fewer contour pixels


# ------------------------------------------------------------------------------------------------ the flatten's second trip

HOLE_TEMPLATES = ("pinholes", "two classes", "ring", "ring island", "sparse")


def _hole_templates(rs, cell=(mo.CELL_H, mo.CELL_W)):
    """Cells with holes: dense noise of one and of two classes, a ring two pixels wide around one hole larger than a tile,
    the same with an island of another class inside (not filled), and sparse noise (mostly open background)."""
    H, W = cell
    ring = np.zeros((H, W), np.uint8)
    ring[1:H - 1, 1:W - 1] = 1
    ring[3:H - 3, 3:W - 3] = 0
    island = ring.copy()
    island[H // 2, W // 2] = 2
    return {"pinholes": (rs.rand(H, W) < 0.9).astype(np.uint8), "two classes": _noise(H, W, 0.85, rs), "ring": ring,
            "ring island": island, "sparse": _noise(H, W, 0.5, rs, 3)}


@functools.lru_cache(maxsize=None)
def _mosaic_case(H, W, conn):
    """labels [2, H, W], the mosaic's component tables, and the expected ids / labels / holes assembled from the per-pixel
    search of every distinct cell.  Cells are separated by background rows and columns that reach the frame, so a region is
    a cell's own -- enclosed exactly when it touches no row or column of the cell's frame, with all its border pixels in the
    cell -- or part of the exterior."""
    rs = np.random.RandomState(H + W + conn)
    labels, tables, exp_ids, exp_lab, exp_holes = [], [], [], [], []
    for b in range(2):
        temps = _hole_templates(rs)
        cells = mo.layout(H, W, rs, HOLE_TEMPLATES)
        lab, tab = mo.mosaic(H, W, cells, temps, conn)
        ids = mo.assemble(lab, tab, 0, 1)[0]
        eid, elab, nf, ne, done = ids.copy(), lab.copy(), 0, 0, {}
        for y, x, h, w, name in cells:
            key = (name, h, w)
            if key not in done:
                cell = mo.crop(temps[name], h, w)
                lids = cr.components_image(cell, conn, 0, 1)[0]
                done[key] = (lids,) + hr.holes_search(cell, lids, conn)[:3]
            lids, io, lo, (f, e) = done[key]
            nf, ne = nf + f, ne + e
            gids = ids[y:y + h, x:x + w]
            to_global = np.zeros(int(lids.max()) + 1, np.int32)
            to_global[lids[lids > 0]] = gids[lids > 0]
            eid[y:y + h, x:x + w] = to_global[io]
            elab[y:y + h, x:x + w] = lo
        labels.append(lab)
        tables.append(tab)
        exp_ids.append(eid)
        exp_lab.append(elab)
        exp_holes.append((nf, ne))
    return np.stack(labels), tuple(tables), np.stack(exp_ids), np.stack(exp_lab), np.array(exp_holes, np.int32)


@pytest.mark.parametrize("shape,conn", [((2049, 2048), 8), ((2120, 2048), 4)], ids=["2049x2048-conn8", "2120x2048-conn4"])
def test_vector_flatten_second_trip(ops, hip_lib, tile, shape, conn):
    """The grids of the three union-find passes are dfw_seg_components' (cc_merge_grid, cc_flatten_grid), so its rounds
    query describes them: at these sizes the four-pixels-a-thread flatten goes round twice.  Expected output from the
    per-cell search; then property 2 on the device: re-labelling labels_out gives ids_out, n and (column 7 zeroed) stats."""
    H, W = shape
    q = oc.components_rounds(hip_lib, H, W)
    assert q["flatten_vector"] == 1 and q["flatten"] == 2 and q["merge"] == 1
    labels, tables, exp_ids, exp_lab, exp_holes = _mosaic_case(H, W, conn)
    assert (exp_holes[:, 0] > 1000).all() and (exp_holes[:, 1] > exp_holes[:, 0]).all()
    cap = max(len(t["area"]) for t in tables) + 3
    comp = mo.components(labels, tables, 0, cap)
    # behind the first trip: regions that reach row `behind` from the tile row above it are open through the last rows alone
    # (their tile-local roots are flattened in the second trip); at 2120 rows whole holes lie behind it and are filled
    behind = oc.FLATTEN_BEHIND // W
    assert behind % 32 == 0 and ((labels[:, behind] == 0) & (labels[:, behind - 1] == 0)).any()
    assert H < behind + 32 or (exp_ids[:, behind:] != comp["ids"][:, behind:]).any()
    got, bufs = _launch(ops, comp["filtered"], comp["ids"], conn, None, comp["stats"])
    assert np.array_equal(got["holes"], exp_holes), (got["holes"].tolist(), exp_holes.tolist())
    assert np.array_equal(got["ids"], exp_ids) and np.array_equal(got["labels"], exp_lab)
    filled = np.stack([np.bincount(e[e != i], minlength=cap + 1)[1:] for e, i in zip(exp_ids, comp["ids"])])
    assert np.array_equal(got["stats"][:, :, 7], filled) and np.array_equal(got["stats"][:, :, 1], comp["stats"][:, :, 1] + filled)
    assert np.array_equal(got["stats"][:, :, [0, 2, 3, 4, 5, 6]], comp["stats"][:, :, [0, 2, 3, 4, 5, 6]])
    # property 2, device only
    from diffews_amd.objects import label_objects
    again = label_objects(bufs["labels_out"].t, connectivity=conn, max_components=cap)
    assert torch.equal(again["ids"], bufs["ids_out"].t) and again["n"].cpu().tolist() == comp["n"].tolist()
    zero7 = bufs["stats_out"].t.clone()
    zero7[:, :, 7] = 0
    assert torch.equal(again["stats"], zero7)
