"""The cases of tests/test_object_rounds_gpu.py, their inputs and their expected outputs, shared with
tests/test_object_rounds_cpu.py, which checks without a GPU that every case reaches the loop round it claims (by the
library's rounds queries) and that its expected output can tell a lost carry from a correct one.  Everything here is numpy
and ctypes on host-only entry points; inputs are seeded and cached, so a process builds each of them once."""
import ctypes as C
import functools

import numpy as np

import components_ref as cr
import match_ref as mr
import mosaic_ref as mo
import rle_ref as rr

NLAB = 3          # classes of the ground truth of the components cases, as in tests/test_components_gpu.py
B = 2             # every case is a batch of two different images
MIN_AREA = 20     # the filter of the matching cases: removes the single pixels match_ref.perturb flips


# ------------------------------------------------------------------------------------------------ the library's thresholds

def blocks(lib):
    """(pixels of a components scan block, positions of a seg scan block, records of a sort chunk)."""
    th, tw, p, r = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.dfw_seg_components_tile(C.byref(th), C.byref(tw)) == 0 and lib.dfw_seg_rle_block(C.byref(p), C.byref(r)) == 0
    return th.value * tw.value, p.value, r.value


def _fields(s):
    return {f[0]: getattr(s, f[0]) for f in s._fields_}


def components_rounds(lib, H, W, ws_offset=0, batch=B):
    """dfw_seg_components_rounds for a workspace `ws_offset` bytes off a 16-byte boundary."""
    from diffews_amd import _lib
    out = _lib.SegComponentsRounds()
    assert lib.dfw_seg_components_rounds(batch, H, W, 4096 + ws_offset, C.byref(out)) == 0
    return _fields(out)


def rle_rounds(lib, H, W, cap, max_runs, order, batch=B):
    from diffews_amd import _lib
    out = _lib.SegSortRounds()
    assert lib.dfw_seg_rle_rounds(batch, H, W, cap, max_runs, rr.ORDERS.index(order), C.byref(out)) == 0
    return _fields(out)


def match_rounds(lib, H, W, cap_p, cap_g, max_records, max_pairs, batch=B):
    from diffews_amd import _lib
    out = _lib.SegSortRounds()
    assert lib.dfw_seg_match_rounds(batch, H, W, cap_p, cap_g, max_records, max_pairs, C.byref(out)) == 0
    return _fields(out)


# ------------------------------------------------------------------------------------------------ the case table
# loop: the field of the rounds query the case is about; least: the rounds the query must report for it.

SCAN_SHAPES = {"513x1024": (513, 1024), "1027x511": (1027, 511)}       # W % 4 == 0: the vector paths; odd W: the scalar ones
SCAN_CASES = [dict(id=f"{s}-conn{c}", shape=SCAN_SHAPES[s], conn=c, loop="scan", least=2) for s in SCAN_SHAPES for c in (4, 8)]
# (min_area, cap (None: above every component), bytes the workspace and words the ids lie off their alignment)
SCAN_RUNS = [(0, None, 0, 0), (5, 16, 0, 0), (0, None, 60, 61)]

# 2049 x 2048: the smallest such map of that width, one image row behind the first trip.  2120 x 2048: the mosaic's last
# cell row, 61 rows across two tile borders, lies wholly behind it, so the second trip flattens whole tile rows.
FLATTEN_CASES = [dict(id=f"2049x2048-conn{c}", shape=(2049, 2048), conn=c, loop="flatten", least=2) for c in (4, 8)]
FLATTEN_CASES.append(dict(id="2120x2048-conn8", shape=(2120, 2048), conn=8, loop="flatten", least=2))
# (min_area, cap (None: above every component), words the ids lie off their alignment); the workspace stays aligned, as the
# vector flatten needs it, so the last run moves the ids alone: cc_apply_kernel's scalar path behind the vector flatten
FLATTEN_RUNS = [(0, None, 0), (5, 16, 0), (5, 16, 61)]
FLATTEN_BEHIND = 4096 * 256 * 4                                         # the first pixel of the second grid-stride trip

BLOCK_SHAPES = {"1024x2048": (1024, 2048), "1025x2051": (1025, 2051)}
RLE_BLOCK_CASES = [dict(id=f"{s}-{o}", shape=BLOCK_SHAPES[s], order=o, loop="block_scan", least=2) for s in BLOCK_SHAPES
                   for o in rr.ORDERS]
MATCH_BLOCK_CASES = [dict(id=s, shape=BLOCK_SHAPES[s], loop="block_scan", least=2, caps=(2047, 2047), max_records=1 << 18,
                          max_pairs=1 << 13, ious=((1, 2), (2, 3))) for s in BLOCK_SHAPES]
MATCH_BLOCK_SEED = 1    # a seed for which the images' last pixel is counted: neither ignored in the ground truth nor removed

TABLE_SHAPE = (150, 140)
RLE_TABLE_CASES = [dict(id=f"cap{c}", cap=c, passes=p, loop="table_scan") for c, p in ((255, 1), (300, 2), (65537, 3))]
MATCH_TABLE_CASES = [dict(id=f"caps{c}", caps=(c, c), passes=p, loop="table_scan", max_pairs=300)
                     for c, p in ((15, 1), (255, 2), (4095, 3))]

# the prediction unfiltered (tens of thousands of objects, many of one pixel), the ground truth filtered at MIN_AREA
CHAIN = dict(id="513x1024", shape=(513, 1024), conn=8, caps=(65535, 4095), order="column", max_runs=1 << 17,
             max_records=1 << 17, max_pairs=1 << 14, loop="scan", least=2, names=("discs", "rings", "noise 0.3", "percolation 8"))

HEADS = dict(id="heads", shape=(40, 50), caps=(7, 7), max_pairs=100, loop="heads_scan", least=2)   # max_records: 1024 R


def table_cuts(R):
    """max_runs / max_records at the borders of the digit table's rounds -> the rounds of its scan, 1024 words a round and
    256 words a chunk of R records."""
    return {4 * R: 1, 4 * R + 1: 2, 8 * R - 1: 2, 8 * R + 1: 3}


# ------------------------------------------------------------------------------------------------ inputs

def _noise(H, W, density, rs):
    return ((rs.rand(H, W) < density) * rs.randint(1, NLAB + 1, (H, W))).astype(np.uint8)


def gt_map(shape, rs):
    """0..NLAB, some 255 (ignore) and some ids above NLAB that have no bin."""
    g = rs.randint(0, NLAB + 1, shape).astype(np.uint8)
    g[rs.rand(*shape) < 0.05] = 255
    g[rs.rand(*shape) < 0.05] = NLAB + 2
    return g


@functools.lru_cache(maxsize=None)
def scan_inputs(H, W):
    """labels, gt [2, H, W]: noise at 0.3; image 1 carries the snake across three tile rows.  Six pixels of a class of
    their own at three places of the last row are components that start behind block 256 and pass min_area = 5."""
    rs = np.random.RandomState(1000 * H + W)
    labels = np.stack([_noise(H, W, 0.3, rs), _noise(H, W, 0.3, rs)])
    labels[1, 96:161] = mo._snake(65, W)
    for b in range(B):
        for x in (10 + 7 * b, 100, 300 + b):
            labels[b, H - 1, x:x + 6] = 9
    gt = gt_map((B, H, W), rs)
    labels.setflags(write=False)
    gt.setflags(write=False)
    return labels, gt


@functools.lru_cache(maxsize=None)
def scan_tables(H, W, conn):
    """The flood fill of both images, as mosaic_ref tables."""
    return tuple(mo.table_of_flood(l, cr.flood(l, conn)) for l in scan_inputs(H, W)[0])


@functools.lru_cache(maxsize=None)
def mosaic_inputs(H, W, conn, names=mo.TEMPLATES, perturbed=False, seed=0):
    """labels [2, H, W] and the tables of two different mosaics; with `perturbed`, also a ground truth of the same layout
    whose templates went through match_ref.perturb (a mosaic too: the separators stay background) and its tables.  The
    last cell is the rings, which have no background: the image's last pixel is foreground."""
    rs = np.random.RandomState(7 * H + W + seed)
    labels, tables, gts, gtables = [], [], [], []
    for b in range(B):
        temps = mo.templates(rs, NLAB)
        cells = mo.layout(H, W, rs, names)
        cells[-1] = cells[-1][:4] + ("rings",)
        lab, tab = mo.mosaic(H, W, cells, temps, conn)
        labels.append(lab)
        tables.append(tab)
        if perturbed:
            gt, gtab = mo.mosaic(H, W, cells, {k: mr.perturb(v, rs) for k, v in temps.items()}, conn)
            gts.append(gt)
            gtables.append(gtab)
    labels = np.stack(labels)
    labels.setflags(write=False)
    if not perturbed:
        return labels, tuple(tables)
    gts = np.stack(gts)
    gts.setflags(write=False)
    return labels, tuple(tables), gts, tuple(gtables)


@functools.lru_cache(maxsize=None)
def flatten_gt(H, W):
    gt = gt_map((B, H, W), np.random.RandomState(5))
    gt.setflags(write=False)
    return gt


@functools.lru_cache(maxsize=None)
def table_ids(top, for_match=False):
    """int32 [2, 150, 140]: every pixel a random id in [0, top + 2], so nearly every pixel is a run of its own and an image
    holds more than 8 R + 1 of them; image 1 is background from its 6000th pixel on and keeps fewer records than image 0
    at every cut."""
    H, W = TABLE_SHAPE
    rs = np.random.RandomState(top + (11 if for_match else 0))
    ids = rs.randint(0, top + 3, (B, H, W)).astype(np.int32)
    ids[0][rs.rand(H, W) < 0.05] = top                                   # the highest digit pattern, often
    ids[1].reshape(-1)[6000:] = 0
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def heads_ids():
    rs = np.random.RandomState(3)
    ids = rs.randint(0, 8, (2, B) + HEADS["shape"]).astype(np.int32)
    ids.setflags(write=False)
    return ids[0], ids[1]


# ------------------------------------------------------------------------------------------------ expected outputs

def starts_of(k):
    """The positions where a record of the key stream k starts: k(q) != k(q - 1) and k(q) != 0."""
    k = np.asarray(k)
    return np.flatnonzero((k != np.concatenate([[0], k[:-1]])) & (k != 0))


@functools.lru_cache(maxsize=None)
def rle_block_expected(H, W, conn=8):
    """The expected components of the mosaic (cap above every component) and the object count of each image."""
    labels, tables = mosaic_inputs(H, W, conn)
    n = max(len(t["area"]) for t in tables)
    want = mo.components(labels, tables, 0, n + 3)
    want["ids"].setflags(write=False)
    return want, [len(t["area"]) for t in tables]


def rle_block_runs(H, W, order, P):
    """[(cap, max_runs)]: cap below, at and above the object count of image 0; max_runs = H * W, the runs found, one less,
    and a cut between the runs that start before position 1024 * P (P: the positions of a scan block) and all of them -- taken from the reference, so the
    records the cut leaves are emitted by the blocks of the scan's second round."""
    want, counts = rle_block_expected(H, W)
    ids = want["ids"]
    n0 = counts[0]
    out = []
    for cap, how in ((n0 + 5, "all"), (n0, "found"), (n0 // 2, "found - 1"), (n0 + 5, "cut")):
        found = int(rr.rle_image(ids[0], cap, H * W, order)[2][1])
        if how == "cut":
            v = rr.flatten(ids[0], order)
            before = int((starts_of(np.where(v <= cap, v, 0)) < 1024 * P).sum())
            out.append((cap, (before + found + 1) // 2 if before < found else found - 2))
        else:
            out.append((cap, {"all": H * W, "found": found, "found - 1": found - 1}[how]))
    return out


def match_block_inputs(H, W, conn=8):
    """labels, tables, ground truth and its tables: three discs a cell, the ground truth's cells perturbed."""
    return mosaic_inputs(H, W, conn, mo.FEW_OBJECTS, True, MATCH_BLOCK_SEED)


@functools.lru_cache(maxsize=None)
def match_block_expected(H, W, conn=8):
    """Expected components of the prediction and of the perturbed ground truth, both filtered at MIN_AREA."""
    cap_p, cap_g = MATCH_BLOCK_CASES[0]["caps"]
    labels, tables, gts, gtables = match_block_inputs(H, W, conn)
    p = mo.components(labels, tables, MIN_AREA, cap_p)
    g = mo.components(gts, gtables, MIN_AREA, cap_g)
    return p, g


@functools.lru_cache(maxsize=None)
def chain_expected(which):
    """The chain's expected outputs for input `which` (0, 1): components of both sides, runs, matching."""
    H, W = CHAIN["shape"]
    c = CHAIN
    cp, cg = c["caps"]
    labels, tables, gts, gtables = mosaic_inputs(H, W, c["conn"], c["names"], True, seed=which)
    p = mo.components(labels, tables, 0, cp)
    g = mo.components(gts, gtables, MIN_AREA, cg)
    runs = rr.rle(p["ids"], cp, c["max_runs"], c["order"])
    m = mr.match(p["ids"], g["ids"], cp, cg, NLAB, c["max_records"], c["max_pairs"], pstats=p["stats"], gstats=g["stats"],
                 skip=gts)
    return labels, gts, p, g, runs, m
