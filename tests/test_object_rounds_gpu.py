"""GPU tests of the object stages (ops.seg_components, ops.seg_rle, ops.seg_match) at the smallest sizes at which a loop of
their kernels that carries a value from one round to the next runs a second (and a third) time.  The sibling files are
thorough on content at maps of up to 65 scan blocks, where each of these loops runs once; here the content is plain and
the SIZE is what is tested, always with B = 2 different images, image 1 alone giving slice 1, and one variant per case
with the ids (and, where the case does not need it aligned, the workspace) off the 16-byte alignment of the vector loads.
The captured chain is the exception to both: it runs on the library's own buffer classes, which allocate aligned, and a
graph is captured for one batch size.  All integers: every comparison is exact.
Every buffer sits inside sentinel guards and outputs are pre-filled.

The loops, with the thresholds as the library reports them (dfw_seg_components_rounds, dfw_seg_rle_rounds,
dfw_seg_match_rounds; P = 2048 positions a scan block, R = 2048 records a sort chunk, tile 32 x 64):

| loop | carried value | second round starts at | case here |
|---|---|---|---|
| cc_scan_kernel, 256 block sums a round | ck, ct; wsum reused by two block_scan calls a round | blocks >= 257, H W >= 524 289 | components scan: 513 x 1024 (257 blocks, 2 rounds), 1027 x 511 (257 blocks, 2 rounds); flatten case: 2049 blocks, 9 rounds |
| seg_scan_kernel on the block sums, 1024 words a round (rle, match) | carry, nout = (min(sum, limit), sum) | blocks >= 1025, H W >= 2 097 152 | rle / match blocks: 1024 x 2048 (1025 blocks: position H W alone in round 2), 1025 x 2051 (1027 blocks) |
| seg_scan_kernel on the sort table, 256 words a chunk | carry | max_runs / max_records > 4 R | table cases: 4 R (1 round), 4 R + 1 and 8 R - 1 (2), 8 R + 1 (3), one to three digit passes, rle and match; block cases: up to 257 rounds |
| seg_scan_kernel, offset (plane * images + image) * n together with a carry | -- | B >= 2 at any of the above | every case (B = 2); planes = 2 in the heads case |
| seg_scan_kernel on run_off / pair_off | carry | cap + 1 > 1024, capP + 2 > 1024 | rle blocks (cap about 10^5), match blocks (capP 2047), chain (cap 65535: 64 and 65 rounds) |
| seg_scan_kernel on the heads and lengths (match) | carry, n[0..1] | max_records >= 1024 R | heads case: a 40 x 50 map with max_records = 1024 R -- the validators allow it (42 MB of workspace an image) |
| cc_flatten_kernel, four pixels a thread, grid capped at 4096 workgroups | grid-stride e | H W > 4 194 304, H W % 4 == 0, aligned workspace | flatten cases: 2049 x 2048 (2 trips; row 2048, the only one behind, starts a tile row, so its runs are tile-local roots) and 2120 x 2048 (2 trips; the last cell row wholly behind) |
| cc_flatten_kernel, one pixel a thread over the same grid | grid-stride p | every size | scan cases at 1027 x 511 and with the workspace 60 bytes off (4 trips) |
| cc_merge_kernel, grid capped at 4096 | grid-stride t | (ntx - 1) H + (nty - 1) W > 1 048 576, about 22 M pixels | LEFT OUT: does not fit a test of a few seconds |
| cc_count, cc_number, seg_count, seg_emit: blk[...] at block indices above 256 / 1024, p0 = block * 2048 | -- | as rows 1 and 2 | the same cases: components, runs and records start behind those blocks |

tests/test_object_rounds_cpu.py asserts, without a GPU, that every case reaches these rounds by the queries and that
the expected outputs have objects on both sides of the borders.  References: the flood fill of tests/components_ref.py
for the scan cases, tests/mosaic_ref.py (equal to the flood fill, checked in the CPU file) above 0.6 M pixels,
tests/rle_ref.py and tests/match_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import match_ref as mr
import mosaic_ref as mo
import object_rounds_cases as oc
import rle_ref as rr

pytestmark = pytest.mark.gpu

SENT = 0xA5
FILL = 0x7B
TABLES = ("n", "pair_off", "area", "match", "gmatch", "pq")
i32, u8 = torch.int32, torch.uint8


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def sizes(hip_lib):
    return oc.blocks(hip_lib)


class _Guarded:
    """A tensor inside a flat allocation with `pad` sentinel elements (0xA5 bytes / -7 words) on either side; the tensor
    itself starts as sentinels too, or as `fill` bytes."""

    def __init__(self, shape, dtype, pad, fill=None):
        n = int(np.prod(shape))
        self.sent = SENT if dtype == torch.uint8 else -7
        self.flat = torch.full((n + 2 * pad,), self.sent, dtype=dtype, device="cuda")
        self.t = self.flat[pad:pad + n].view(shape)
        self.pad, self.n = pad, n
        if fill is not None:
            self.t.view(torch.uint8).fill_(fill)

    def check(self, name):
        assert (self.flat[:self.pad] == self.sent).all() and (self.flat[self.pad + self.n:] == self.sent).all(), f"wrote outside {name}"


def _word(fill):
    return int(np.array([fill] * 4, np.uint8).view(np.int32)[0])


def _checked(bufs):
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)


def _put(g, a):
    g.t.copy_(torch.from_numpy(np.array(a)))                              # a copy: the cached inputs are read-only
    return g


# ------------------------------------------------------------------------------------------------ launches

def _components(ops, labels, conn, min_area, cap, gt=None, ws_off=0, ids_off=0):
    """ops.seg_components into guarded, pre-filled buffers -> (numpy results, the buffers).  ws_off: bytes the workspace
    lies off a 16-byte boundary; ids_off: words the ids do."""
    Bn, H, W = labels.shape
    bufs = dict(labels=_put(_Guarded((Bn, H, W), u8, 64), labels), ids=_Guarded((Bn, H, W), i32, 4 + ids_off, FILL),
                n=_Guarded((Bn, 2), i32, 4, FILL), ws=_Guarded((ops.seg_components_workspace(Bn, H, W),), u8, 64 + ws_off, FILL),
                filtered=_Guarded((Bn, H, W), u8, 64, FILL), stats=_Guarded((Bn, cap, 8), i32, 4, FILL))
    if gt is not None:
        bufs["gt"] = _put(_Guarded((Bn, H, W), u8, 64), gt)
        bufs["counts"] = _Guarded((Bn, 2, oc.NLAB + 1), torch.int64, 2, FILL)
    assert bufs["ws"].t.data_ptr() % 16 == ws_off % 16 and bufs["ids"].t.data_ptr() % 16 == 4 * ids_off % 16
    ops.seg_components(bufs["labels"].t, bufs["ids"].t, bufs["n"].t, bufs["ws"].t, filtered=bufs["filtered"].t,
                       stats=bufs["stats"].t, gt=bufs["gt"].t if gt is not None else None,
                       counts=bufs["counts"].t if gt is not None else None, connectivity=conn, min_area=min_area,
                       nlabels=oc.NLAB if gt is not None else None)
    _checked(bufs)
    assert np.array_equal(bufs["labels"].t.cpu().numpy(), labels), "the input was modified"
    return {k: bufs[k].t.cpu().numpy() for k in ("ids", "n", "filtered", "stats", "counts") if k in bufs}, bufs


def _same_components(got, want, what):
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (what, k, int((v != want[k]).sum()))


def _rle(ops, ids, cap, max_runs, order, ws_off=0):
    """ops.seg_rle on a DEVICE tensor ids [B, H, W] into guarded, pre-filled buffers -> numpy results."""
    Bn, H, W = ids.shape
    bufs = dict(runs=_Guarded((Bn, max_runs, 2), i32, 4, FILL), run_off=_Guarded((Bn, cap + 1), i32, 4, FILL),
                nruns=_Guarded((Bn, 2), i32, 4, FILL),
                ws=_Guarded((ops.seg_rle_workspace(Bn, H, W, cap, max_runs, order),), u8, 64 + ws_off, FILL))
    ops.seg_rle(ids, bufs["runs"].t, bufs["run_off"].t, bufs["nruns"].t, bufs["ws"].t, cap, order)
    _checked(bufs)
    return {k: bufs[k].t.cpu().numpy() for k in ("runs", "run_off", "nruns")}


def _same_runs(got, want, what, b0=0):
    """nruns and run_off whole, runs up to kept; the rows behind kept keep the fill.  b0: `got` is image b0 alone."""
    n = len(got["nruns"])
    assert np.array_equal(got["nruns"], want["nruns"][b0:b0 + n]), (what, got["nruns"].tolist(), want["nruns"].tolist())
    assert np.array_equal(got["run_off"], want["run_off"][b0:b0 + n]), (what, "run_off")
    for b in range(n):
        w = want["runs"][b0 + b]
        assert np.array_equal(got["runs"][b, :len(w)], w), (what, "runs", b0 + b, int((got["runs"][b, :len(w)] != w).sum()))
        assert (got["runs"][b, len(w):] == _word(FILL)).all(), (what, "rows behind kept were written", b0 + b)


def _match(ops, pids, gids, cap_p, cap_g, nlabels, max_records, max_pairs, pstats=None, gstats=None, skip=None, iou=(1, 2),
           ws_off=0):
    """ops.seg_match on DEVICE tensors into guarded, pre-filled buffers -> numpy results."""
    Bn, H, W = pids.shape
    nbytes = ops.seg_match_workspace(Bn, H, W, cap_p, cap_g, max_records, max_pairs)
    assert nbytes > 0
    bufs = dict(pairs=_Guarded((Bn, max_pairs, 3), i32, 4, FILL), pair_off=_Guarded((Bn, cap_p + 2), i32, 4, FILL),
                area=_Guarded((Bn, cap_p + cap_g + 2), i32, 4, FILL), match=_Guarded((Bn, cap_p, 3), i32, 4, FILL),
                gmatch=_Guarded((Bn, cap_g), i32, 4, FILL), pq=_Guarded((Bn, nlabels + 1, 4), torch.int64, 2, FILL),
                n=_Guarded((Bn, 4), i32, 4, FILL), ws=_Guarded((nbytes,), u8, 64 + ws_off, FILL))
    g = {k: v.t for k, v in bufs.items()}
    ops.seg_match(pids, gids, g["pairs"], g["pair_off"], g["area"], g["match"], g["gmatch"], g["pq"], g["n"], g["ws"],
                  max_records, pstats=pstats, gstats=gstats, skip=skip, iou=iou)
    _checked(bufs)
    return {k: g[k].cpu().numpy() for k in TABLES + ("pairs",)}


def _same_match(got, want, what, b0=0):
    n = len(got["n"])
    for k in TABLES:
        w = want[k][b0:b0 + n]
        assert got[k].dtype == w.dtype and np.array_equal(got[k], w), (what, k, int((got[k] != w).sum()))
    for b in range(n):
        w = want["pairs"][b0 + b]
        assert np.array_equal(got["pairs"][b, :len(w)], w), (what, "pairs", b0 + b)
        assert (got["pairs"][b, len(w):] == _word(FILL)).all(), (what, "rows behind kept were written", b0 + b)


def _off(off, a):
    """The numpy int32 array `a` on the device, `off` words behind a 16-byte boundary, inside guards."""
    g = _put(_Guarded(a.shape, i32, 4 + off), a)
    assert g.t.data_ptr() % 16 == 4 * off % 16
    return g


# ------------------------------------------------------------------------------------------------ components

@pytest.mark.parametrize("case", oc.SCAN_CASES, ids=[c["id"] for c in oc.SCAN_CASES])
def test_components_scan_second_round(ops, hip_lib, sizes, case):
    """257 scan blocks: cc_scan_kernel goes round twice, and components start in block 256.  Noise at 0.3 and the snake
    against the flood fill; min_area 0 with a cap above every component and min_area 5 with cap 16; a ground truth with 255
    and ids above nlabels; then the workspace and the ids off their alignment (the scalar flatten, which wraps)."""
    H, W = case["shape"]
    assert oc.components_rounds(hip_lib, H, W)[case["loop"]] >= case["least"]
    labels, gt = oc.scan_inputs(H, W)
    tables = oc.scan_tables(H, W, case["conn"])
    top = max(len(t["area"]) for t in tables) + 3
    for min_area, cap, ws_off, ids_off in oc.SCAN_RUNS:
        cap = top if cap is None else cap
        want = mo.components(labels, tables, min_area, cap, gt, oc.NLAB)
        got, _ = _components(ops, labels, case["conn"], min_area, cap, gt, ws_off, ids_off)
        _same_components(got, want, (case["id"], min_area, cap, ws_off))
        if ws_off == 0:
            one, _ = _components(ops, labels[1:], case["conn"], min_area, cap, gt[1:])
            _same_components(one, {k: v[1:] for k, v in want.items()}, (case["id"], min_area, "image 1 alone"))


@pytest.mark.parametrize("case", oc.FLATTEN_CASES, ids=[c["id"] for c in oc.FLATTEN_CASES])
def test_components_vector_flatten_second_trip(ops, hip_lib, case):
    """2049 x 2048 with an aligned workspace: the four-pixels-a-thread flatten wraps, and the runs of row 2048, which
    starts a tile row, are tile-local roots of components whose first pixel lies far before; at 2120 x 2048 the mosaic's
    last cell row lies wholly behind the first trip.  A mosaic against the mosaic reference; the scan goes round nine
    times on the way.  The last run has the ids 61 words off their alignment (the workspace must stay aligned here)."""
    H, W = case["shape"]
    q = oc.components_rounds(hip_lib, H, W)
    assert q["flatten_vector"] == 1 and q[case["loop"]] >= case["least"]
    labels, tables = oc.mosaic_inputs(H, W, case["conn"])
    gt = oc.flatten_gt(H, W)
    top = max(len(t["area"]) for t in tables) + 3
    for min_area, cap, ids_off in oc.FLATTEN_RUNS:
        cap = top if cap is None else cap
        want = mo.components(labels, tables, min_area, cap, gt, oc.NLAB)
        got, _ = _components(ops, labels, case["conn"], min_area, cap, gt, ids_off=ids_off)
        _same_components(got, want, (case["id"], min_area, cap, ids_off))
    one, _ = _components(ops, labels[1:], case["conn"], min_area, cap, gt[1:])
    _same_components(one, {k: v[1:] for k, v in want.items()}, (case["id"], "image 1 alone"))


# ------------------------------------------------------------------------------------------------ run-length encoding

@pytest.mark.parametrize("case", oc.RLE_BLOCK_CASES, ids=[c["id"] for c in oc.RLE_BLOCK_CASES])
def test_rle_block_scan_second_round(ops, hip_lib, sizes, case):
    """1025 and 1027 scan blocks: seg_scan_kernel goes round twice on the block sums, seg_emit reads them behind block
    1024.  The ids are seg_components' own on a mosaic and stay on the device; cap below, at and above the object count,
    max_runs = H W, the runs found, one less, and a cut that leaves records of the second round; the column order also
    transposes ragged tiles on both axes at 1025 x 2051."""
    H, W = case["shape"]
    order = case["order"]
    _, P, R = sizes
    labels, tables = oc.mosaic_inputs(H, W, 8)
    want_c, counts = oc.rle_block_expected(H, W)
    got_c, bufs = _components(ops, labels, 8, 0, want_c["stats"].shape[1])
    _same_components(got_c, want_c, (case["id"], "components"))
    ids = bufs["ids"].t                                                    # the chain goes on on the device
    assert ids.data_ptr() % 16 == 0
    for cap, max_runs in oc.rle_block_runs(H, W, order, P):
        assert oc.rle_rounds(hip_lib, H, W, cap, max_runs, order)[case["loop"]] >= case["least"]
        want = rr.rle(want_c["ids"], cap, max_runs, order)
        _same_runs(_rle(ops, ids, cap, max_runs, order), want, (case["id"], cap, max_runs))
    # image 1 alone gives slice 1; then both images 61 words off the alignment, the workspace 60 bytes
    _same_runs(_rle(ops, ids[1:], cap, max_runs, order), want, (case["id"], "image 1 alone"), b0=1)
    odd = _off(61, want_c["ids"])
    _same_runs(_rle(ops, odd.t, cap, max_runs, order, ws_off=60), want, (case["id"], "off alignment"))
    odd.check("ids")


@pytest.mark.parametrize("case", oc.RLE_TABLE_CASES, ids=[c["id"] for c in oc.RLE_TABLE_CASES])
def test_rle_sort_table_two_and_three_rounds(ops, hip_lib, sizes, case):
    """max_runs at 4 R, 4 R + 1, 8 R - 1 and 8 R + 1 on a map with more runs than that in image 0 and fewer in image 1: the
    digit table of 256 words a chunk is scanned in one, two and three rounds, per image, with one to three digit passes."""
    _, P, R = sizes
    H, W = oc.TABLE_SHAPE
    cap = case["cap"]
    ids = oc.table_ids(cap)
    for off in (0, 61):
        dev = _off(off, ids)
        for M, rounds in oc.table_cuts(R).items():
            for order in rr.ORDERS:
                q = oc.rle_rounds(hip_lib, H, W, cap, M, order)
                assert q["table_scan"] == rounds and q["passes"] == case["passes"]
                want = rr.rle(ids, cap, M, order)
                assert want["nruns"][0, 0] == M > want["nruns"][1, 0] == want["nruns"][1, 1]
                _same_runs(_rle(ops, dev.t, cap, M, order, ws_off=60 if off else 0), want, (cap, M, order, off))
                if off == 0 and rounds == 3:
                    _same_runs(_rle(ops, dev.t[1:], cap, M, order), want, (cap, M, order, "image 1 alone"), b0=1)
        dev.check("ids")


# ------------------------------------------------------------------------------------------------ matching

@pytest.mark.parametrize("case", oc.MATCH_TABLE_CASES, ids=[c["id"] for c in oc.MATCH_TABLE_CASES])
def test_match_sort_table_two_and_three_rounds(ops, hip_lib, sizes, case):
    """The same cuts for max_records, keys of one to three bytes."""
    _, P, R = sizes
    H, W = oc.TABLE_SHAPE
    cp, cg = case["caps"]
    MP = case["max_pairs"]
    pids, gids = oc.table_ids(cp), oc.table_ids(cg, True)
    for off in (0, 61):
        dp, dg = _off(off, pids), _off(off, gids)
        for M, rounds in oc.table_cuts(R).items():
            q = oc.match_rounds(hip_lib, H, W, cp, cg, M, MP)
            assert q["table_scan"] == rounds and q["passes"] == case["passes"]
            want = mr.match(pids, gids, cp, cg, 1, M, MP)
            assert want["n"][0, 2] == M > want["n"][1, 2] == want["n"][1, 3]
            _same_match(_match(ops, dp.t, dg.t, cp, cg, 1, M, MP, ws_off=60 if off else 0), want, (cp, M, off))
            if off == 0 and rounds == 3:
                _same_match(_match(ops, dp.t[1:], dg.t[1:], cp, cg, 1, M, MP), want, (cp, M, "image 1 alone"), b0=1)
        dp.check("pids")
        dg.check("gids")


@pytest.mark.parametrize("case", oc.MATCH_BLOCK_CASES, ids=[c["id"] for c in oc.MATCH_BLOCK_CASES])
def test_match_block_scan_second_round(ops, hip_lib, sizes, case):
    """1025 and 1027 scan blocks with a few hundred objects a side: pids are seg_components' ids of a mosaic, gids those of
    the same mosaic with perturbed cells, both filtered by area and both left on the device; the ground-truth labels are
    the skip map, both sides bring their class tables, and the threshold is 1/2 and 2/3."""
    H, W = case["shape"]
    cp, cg = case["caps"]
    M, MP = case["max_records"], case["max_pairs"]
    assert oc.match_rounds(hip_lib, H, W, cp, cg, M, MP)[case["loop"]] >= case["least"]
    labels, _, gts, _ = oc.match_block_inputs(H, W)
    want_p, want_g = oc.match_block_expected(H, W)
    got_p, pb = _components(ops, labels, 8, oc.MIN_AREA, cp)
    got_g, gb = _components(ops, gts, 8, oc.MIN_AREA, cg)
    _same_components(got_p, want_p, (case["id"], "prediction"))
    _same_components(got_g, want_g, (case["id"], "ground truth"))
    dev = dict(pids=pb["ids"].t, gids=gb["ids"].t, pstats=pb["stats"].t, gstats=gb["stats"].t, skip=gb["labels"].t)
    for iou in case["ious"]:
        want = mr.match(want_p["ids"], want_g["ids"], cp, cg, oc.NLAB, M, MP, pstats=want_p["stats"], gstats=want_g["stats"],
                        skip=gts, iou=iou)
        assert (want["n"][:, 0] == want["n"][:, 1]).all() and (want["n"][:, 2] == want["n"][:, 3]).all()
        assert want["pq"][:, 1:, 0].sum() > 50 and want["pq"][:, 1:, 1:3].sum() > 0
        got = _match(ops, dev["pids"], dev["gids"], cp, cg, oc.NLAB, M, MP, pstats=dev["pstats"], gstats=dev["gstats"],
                     skip=dev["skip"], iou=iou)
        _same_match(got, want, (case["id"], iou))
    one = _match(ops, dev["pids"][1:], dev["gids"][1:], cp, cg, oc.NLAB, M, MP, pstats=dev["pstats"][1:],
                 gstats=dev["gstats"][1:], skip=dev["skip"][1:], iou=iou)
    _same_match(one, want, (case["id"], "image 1 alone"), b0=1)
    # both id maps 61 words and skip 3 bytes off the alignment of the vector loads, the workspace 60 bytes
    op, og = _off(61, want_p["ids"]), _off(61, want_g["ids"])
    sk = _put(_Guarded(gts.shape, u8, 3), gts)
    got = _match(ops, op.t, og.t, cp, cg, oc.NLAB, M, MP, pstats=dev["pstats"], gstats=dev["gstats"], skip=sk.t, iou=iou,
                 ws_off=60)
    _same_match(got, want, (case["id"], "off alignment"))
    for k, v in (("pids", op), ("gids", og), ("skip", sk)):
        v.check(k)


def test_match_heads_scan_second_round(ops, hip_lib, sizes):
    """max_records = 1024 R on a 40 x 50 map: dfw_seg_match accepts it (the validators bound B * max_records by 2^31 - 1,
    not by the map), the heads and lengths are scanned in two rounds over two planes and two images, and n[0..1] is the
    carry behind the second.  All records of so small a map lie in chunk 0: the second round scans zeros, and no record
    reads the words it writes, so a wrong offset written in round 2 (not the carried sum) would go unseen here."""
    _, P, R = sizes
    h = oc.HEADS
    H, W = h["shape"]
    cp, cg = h["caps"]
    M, MP = 1024 * R, h["max_pairs"]
    q = oc.match_rounds(hip_lib, H, W, cp, cg, M, MP)
    assert q[h["loop"]] >= h["least"]
    pids, gids = oc.heads_ids()
    want = mr.match(pids, gids, cp, cg, 1, M, MP)
    assert (want["n"][:, 0] == 63).all() and (want["n"][:, 2] > 1000).all()
    dp, dg = _off(0, pids), _off(0, gids)
    _same_match(_match(ops, dp.t, dg.t, cp, cg, 1, M, MP), want, "heads")
    _same_match(_match(ops, dp.t[1:], dg.t[1:], cp, cg, 1, M, MP), want, "heads, image 1 alone", b0=1)
    op, og = _off(61, pids), _off(61, gids)
    _same_match(_match(ops, op.t, og.t, cp, cg, 1, M, MP, ws_off=60), want, "heads, off alignment")
    for k, v in (("pids", dp), ("gids", dg), ("pids off", op), ("gids off", og)):
        v.check(k)


# ------------------------------------------------------------------------------------------------ the chain, captured

def test_captured_chain_at_the_scan_s_second_round(ops, hip_lib, sizes):
    """seg_components of the prediction and of the ground truth, seg_rle and seg_match in one torch.cuda.graph at 513 x
    1024, B = 2: no memset node, the node count of the headers' formulas, and a replay on a second input is exact on every
    output of the three stages."""
    from diffews_amd.objects import ComponentBuffers, MatchBuffers, RunBuffers
    c = oc.CHAIN
    H, W = c["shape"]
    (cp, cg), order = c["caps"], c["order"]
    pb, gb = ComponentBuffers(oc.B, H, W, cp), ComponentBuffers(oc.B, H, W, cg)
    rb = RunBuffers(oc.B, H, W, cp, max_runs=c["max_runs"], order=order)
    mb = MatchBuffers(oc.B, H, W, cp, cg, oc.NLAB, max_records=c["max_records"], max_pairs=c["max_pairs"])
    lab = torch.zeros(oc.B, H, W, dtype=u8, device="cuda")
    gt = torch.zeros(oc.B, H, W, dtype=u8, device="cuda")

    def call():
        ops.seg_components(lab, pb.ids, pb.n, pb.ws, filtered=pb.labels, stats=pb.stats, connectivity=c["conn"])
        ops.seg_components(gt, gb.ids, gb.n, gb.ws, filtered=gb.labels, stats=gb.stats, connectivity=c["conn"],
                           min_area=oc.MIN_AREA)
        ops.seg_rle(pb.ids, rb.runs, rb.run_off, rb.nruns, rb.ws, cp, order)
        ops.seg_match(pb.ids, gb.ids, mb.pairs, mb.pair_off, mb.area, mb.match, mb.gmatch, mb.pq, mb.n, mb.ws, mb.max_records,
                      pstats=pb.stats, gstats=gb.stats, skip=gt)
    call()                                                                 # modules loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    nodes = C.c_int32()
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0
    rq = oc.rle_rounds(hip_lib, H, W, cp, c["max_runs"], order)
    mq = oc.match_rounds(hip_lib, H, W, cp, cg, c["max_records"], c["max_pairs"])
    assert rq["passes"] == 2 and mq["passes"] == 4 and rq["offsets_scan"] == 64 and mq["offsets_scan"] == 65
    assert nodes.value == 8 + 8 + (5 + (order == "column") + 3 * 2) + (14 + 3 * 4)
    graph.instantiate()
    for which in (0, 1, 0):
        labels, gts, p, g, runs, m = oc.chain_expected(which)
        for t in (pb.ids, gb.ids, rb.runs, mb.pairs):
            t.view(torch.uint8).fill_(FILL)
        lab.copy_(torch.from_numpy(np.array(labels)))
        gt.copy_(torch.from_numpy(np.array(gts)))
        graph.replay()
        torch.cuda.synchronize()
        for buf, want, side in ((pb, p, "prediction"), (gb, g, "ground truth")):
            got = dict(ids=buf.ids.cpu().numpy(), n=buf.n.cpu().numpy(), filtered=buf.labels.cpu().numpy(),
                       stats=buf.stats.cpu().numpy())
            _same_components(got, want, ("replay", which, side))
        _same_runs({k: getattr(rb, k).cpu().numpy() for k in ("runs", "run_off", "nruns")}, runs, ("replay", which))
        _same_match({k: getattr(mb, k).cpu().numpy() for k in TABLES + ("pairs",)}, m, ("replay", which))
