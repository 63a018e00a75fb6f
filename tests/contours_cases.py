"""The inputs of tests/test_object_contours_gpu.py that are there for a SIZE -- a ring of a given length, a number of sort
passes, a second trip of a scan -- shared with tests/test_object_contours_cpu.py, which proves without a GPU, by the
library's own queries (dfw_seg_contours_block / _rounds), that every one reaches the size it claims.  Numpy and ctypes on
host-only entry points."""
import ctypes as C

import numpy as np


def block(lib):
    """(pixels of a scan block, edges of a block of the ring count)."""
    p, e = C.c_int32(), C.c_int32()
    assert lib.dfw_seg_contours_block(C.byref(p), C.byref(e)) == 0
    return p.value, e.value


def trips(lib, B, H, W, cap, max_edges):
    from diffews_amd import _lib
    out = _lib.SegContoursTrips()
    assert lib.dfw_seg_contours_rounds(B, H, W, cap, max_edges, C.byref(out)) == 0, (B, H, W, cap, max_edges)
    return {f[0]: getattr(out, f[0]) for f in out._fields_}


def up4(n):
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ one long ring

def row(n):
    """1 x n of one object: one ring of 2 n + 2 edges."""
    return np.ones((1, n), np.int32)


def serpentine(rows=8, W=32):
    """`rows` full rows joined in turn at the right and the left end: one ring, in a (2 rows - 1) x W map."""
    m = np.zeros((2 * rows - 1, W), np.int32)
    m[::2] = 1
    for y in range(1, 2 * rows - 1, 2):
        m[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return m


def long_rings(lib):
    """name -> (ids [H, W], edges of its one ring): lengths just below, at and above a power of two, the serpentine, and
    a ring longer than a block of the ring count."""
    _, E = block(lib)
    out = {"row31": (row(31), 64), "row32": (row(32), 66), "row30": (row(30), 62), "serpentine": (serpentine(), 528),
           "row-above-block": (row(E // 2 + 7), E + 16)}
    # the same around the next power of two above the block: 2 n + 2 = 2 E - 2, 2 E, 2 E + 2
    for d in (-2, -1, 0):
        out[f"row{E + d}"] = (row(E + d), 2 * (E + d) + 2)
    return out


# ------------------------------------------------------------------------------------------------ many rings

def checkerboard(H, W):
    """Every second pixel its own object, numbered in row-major order: 4-connected singletons, 4 edges each."""
    yy, xx = np.mgrid[:H, :W]
    on = (yy + xx) % 2 == 0
    ids = np.zeros((H, W), np.int32)
    ids[on] = np.arange(1, int(on.sum()) + 1)
    return ids


# (H, W, cap, sort passes): cap + 1 keys need that many bytes
SORT_CASES = [(22, 23, 255, 1), (22, 23, 256, 2), (512, 512, 131072, 3)]


# ------------------------------------------------------------------------------------------------ second trips of the scans

def singletons(n):
    """The first n objects of a checkerboard just large enough for them: n rings of 4 edges."""
    side = 1
    while (side * side + 1) // 2 < n:
        side += 1
    ids = checkerboard(side, side)
    ids[ids > n] = 0
    return ids


def second_trip_cases(lib):
    """name -> dict(ids [H, W], cap, max_edges, field): the smallest size, in the argument that drives it, at which the
    scan `field` of the rounds query goes round twice (a trip covers 1024 words), on a map whose last words are not zero
    wherever a map of that kind is affordable: the carry into the second trip then shows in the result.  ring_scan would
    need more than 1024 blocks of edges, two million of them; its map is small and only the trip count is reached."""
    P, E = block(lib)
    p, r = C.c_int32(), C.c_int32()
    assert lib.dfw_seg_rle_block(C.byref(p), C.byref(r)) == 0
    R = r.value                                            # ring rows per sort chunk
    wide = np.zeros((1024 * P // 2048 + 1, 2048), np.int32)
    wide[5:40, 7:90], wide[10:20, 20:30], wide[-3:, -9:] = 1, 0, 2
    odd = np.zeros((1024 * P // 2048 + 1, 2047), np.int32)
    odd[3:9, 3:11], odd[-1, -2:] = 1, 2
    small = np.zeros((64, 64), np.int32)
    small[3:30, 5:40], small[10:20, 10:20], small[40:, 50:] = 1, 0, 2
    return {
        # 1024 blocks of P pixels and a little: W a multiple of 4 (the vector path) in the first, odd in the second
        "block_scan": dict(ids=wide, cap=8, max_edges=4096, field="block_scan"),
        "block_scan-odd": dict(ids=odd, cap=8, max_edges=4096, field="block_scan"),
        "ring_scan": dict(ids=small, cap=8, max_edges=1024 * E + 4, field="ring_scan"),
        "table_scan": dict(ids=singletons(4 * R + 1), cap=4 * R + 1, max_edges=4 * (4 * R + 1), field="table_scan"),
        "offsets_scan": dict(ids=singletons(1024), cap=1024, max_edges=4096, field="offsets_scan"),
        "corners_scan": dict(ids=singletons(1025), cap=1025, max_edges=4100, field="corners_scan"),
    }


def blobs(H, W, rs, n=40):
    """Random discs, some with a disc cut out of them: a label map (uint8, classes 1..3) with objects, holes and
    islands."""
    yy, xx = np.mgrid[:H, :W]
    lab = np.zeros((H, W), np.uint8)
    for _ in range(n):
        cy, cx, r = rs.randint(0, H), rs.randint(0, W), rs.randint(2, max(3, min(H, W) // 6))
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rs.randint(1, 4)
        if rs.rand() < 0.5:
            lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= (r // 2) ** 2] = 0
    return lab
