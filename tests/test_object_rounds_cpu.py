"""CPU checks behind tests/test_object_rounds_gpu.py (no GPU): the mosaic reference equals the flood fill, and every GPU
case reaches what it claims -- the library's rounds queries report the loop round the case is about, and the expected
output alone shows that the case can tell a lost carry from a correct one: components, runs or records start on both sides
of the block at which a scan's second round begins, tile-crossing components have pixels behind the flatten kernel's first
trip, records fall into the words of the digit table's second and third round.  These are conditions on the seeded
inputs of tests/object_rounds_cases.py, asserted here; the case table is the one the GPU file runs."""
import numpy as np
import pytest

import components_ref as cr
import match_ref as mr
import mosaic_ref as mo
import object_rounds_cases as oc
import rle_ref as rr


@pytest.fixture(scope="module")
def sizes(hip_lib):
    return oc.blocks(hip_lib)


# ------------------------------------------------------------------------------------------------ the mosaic reference

def _small_mosaic(rs, conn):
    H, W = rs.randint(40, 70), rs.randint(50, 90)
    cell, least = (9 + rs.randint(0, 6), 13 + rs.randint(0, 9)), (3, 4)
    temps = mo.templates(rs, oc.NLAB, cell)
    cells = mo.layout(H, W, rs, mo.TEMPLATES + ("discs",), cell, least)
    lab, tab = mo.mosaic(H, W, cells, temps, conn)
    return lab, tab, cells


@pytest.mark.parametrize("conn", [4, 8])
def test_mosaic_reference_equals_the_flood_fill(conn):
    """Mosaics of a few thousand pixels with ragged last cells: ids, filtered, n, stats and counts of the mosaic reference
    are those of components_ref.components, with min_area 0 and 5 and with a cap below and above the number of
    components; so is the numpy assemble on the table of a plain flood fill."""
    rs = np.random.RandomState(100 + conn)
    removed = 0
    for _ in range(12):
        lab, tab, cells = _small_mosaic(rs, conn)
        H, W = lab.shape
        assert 2000 <= H * W < 7000 and len(cells) >= 9 and len({c[4] for c in cells}) >= 3
        # one background row and column between two cells, and the cells reach the last pixel
        for y, x, h, w, _ in cells:
            assert (y == 0 or not lab[y - 1].any()) and (x == 0 or not lab[:, x - 1].any())
        assert max(c[0] + c[2] for c in cells) == H and max(c[1] + c[3] for c in cells) == W
        gt = oc.gt_map((1, H, W), rs)
        comps = [cr.flood(lab, conn)]
        assert len(comps[0]) == len(tab["area"]) > 16
        for min_area in (0, 5):
            for cap in (16, len(comps[0]) + 2):
                want = cr.components(lab[None], conn, min_area, cap, gt, oc.NLAB, comps=comps)
                for tables in ([tab], [mo.table_of_flood(lab, comps[0])]):
                    got = mo.components(lab[None], tables, min_area, cap, gt, oc.NLAB)
                    for k in want:
                        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, min_area, cap)
        removed += want["n"][0, 0] < want["n"][0, 1]
    assert removed >= 6                                                    # min_area = 5 removes something in most of them


@pytest.mark.parametrize("conn", [4, 8])
def test_mosaic_reference_is_scipy_s_partition(conn):
    """An independent labelling: scipy.ndimage.label per class, renumbered by first pixel and filtered by area."""
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)
    rs = np.random.RandomState(200 + conn)
    for _ in range(6):
        lab, tab, _ = _small_mosaic(rs, conn)
        part, found = np.zeros(lab.shape, np.int64), 0
        for c in np.unique(lab[lab > 0]):
            l, n = ndimage.label(lab == c, structure=structure)
            part[l > 0] = l[l > 0] + found
            found += n
        for min_area in (0, 5):
            flat = part.ravel()
            keep = np.bincount(flat, minlength=found + 1) >= min_area
            keep[0] = False
            flat = np.where(keep[flat], flat, 0)
            u, first = np.unique(flat, return_index=True)
            u, first = u[u > 0], first[u > 0]
            remap = np.zeros(found + 1, np.int64)
            remap[u[np.argsort(first)]] = np.arange(1, len(u) + 1)
            ids, _, n, _ = mo.assemble(lab, tab, min_area, 8)
            assert n == (len(u), found) and np.array_equal(ids, remap[flat].reshape(lab.shape))


def test_truncated_runs_are_the_runs_of_the_stream_cut_at_run_m():
    """rle_ref truncated to m runs equals rle_ref untruncated on the stream zeroed from the start of run m on: the oracle
    of the cuts inside the second scan round."""
    rs = np.random.RandomState(9)
    for _ in range(40):
        H, W = rs.randint(3, 30), rs.randint(3, 40)
        ids = (rs.randint(0, 6, (H, W)) * (rs.rand(H, W) < 0.7)).astype(np.int32)
        for order in rr.ORDERS:
            v = rr.flatten(ids, order)
            st = oc.starts_of(v)
            for m in (1, len(st) // 2, len(st) - 1):
                if 1 <= m < len(st):
                    cut = v.copy()
                    cut[st[m]:] = 0
                    cut = cut.reshape(H, W) if order == "row" else cut.reshape(W, H).T
                    a, b = rr.rle_image(ids, 5, m, order), rr.rle_image(cut, 5, H * W, order)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2][0] == b[2][0] == m


# ------------------------------------------------------------------------------------------------ components cases

def _both_sides(first, border, what):
    assert (first < border).any() and (first >= border).any(), what


@pytest.mark.parametrize("case", oc.SCAN_CASES, ids=[c["id"] for c in oc.SCAN_CASES])
def test_scan_cases_reach_the_second_round(hip_lib, sizes, case):
    H, W = case["shape"]
    PC = sizes[0]
    for _, _, ws_off, _ in oc.SCAN_RUNS:
        q = oc.components_rounds(hip_lib, H, W, ws_off)
        assert q[case["loop"]] >= case["least"] and q["blocks"] == -(-H * W // PC) > 256
        vector = H * W % 4 == 0 and ws_off % 16 == 0
        assert q["flatten_vector"] == vector and (vector or q["flatten"] >= 2)
    assert oc.components_rounds(hip_lib, 256, PC, 0)["scan"] == 1           # 256 blocks: one round; one pixel more: two
    labels, gt = oc.scan_inputs(H, W)
    assert not np.array_equal(labels[0], labels[1]) and (gt == 255).any() and (gt == oc.NLAB + 2).any()
    for b, t in enumerate(oc.scan_tables(H, W, case["conn"])):
        for min_area, cap, _, _ in oc.SCAN_RUNS:
            kept = t["first"][t["area"] >= min_area]
            _both_sides(kept, 256 * PC, (case["id"], b, min_area, "kept components on both sides of block 256"))
            if cap is None:                                                # stats holds a row for every kept component
                assert len(kept) > 16
    assert t["area"].max() > 65 * W // 2                                   # image 1: the snake is one component across tiles


@pytest.mark.parametrize("case", oc.FLATTEN_CASES, ids=[c["id"] for c in oc.FLATTEN_CASES])
def test_flatten_cases_reach_the_vector_path_s_second_trip(hip_lib, sizes, case):
    H, W = case["shape"]
    q = oc.components_rounds(hip_lib, H, W, 0)
    assert q["flatten_vector"] == 1 and q["flatten"] >= case["least"] and q["scan"] >= 2
    assert H * W % 4 == 0 and H * W > oc.FLATTEN_BEHIND
    one = oc.components_rounds(hip_lib, oc.FLATTEN_BEHIND // W, W, 0)       # the largest map of one trip
    assert one["flatten_vector"] == 1 and one["flatten"] == 1
    labels, tables = oc.mosaic_inputs(H, W, case["conn"])
    assert not np.array_equal(labels[0], labels[1])
    row = oc.FLATTEN_BEHIND // W
    assert row % 32 == 0                               # a tile row starts there: every run of that row is a tile-local root
    last = mo.spans(H, mo.CELL_H, 32)[-1]
    for b, t in enumerate(tables):
        if H == row + 1:                               # one image row behind: components with pixels on both sides of it,
            crossing = (t["y0"] < row) & (t["y1"] > row)                   # whose roots lie before it
        else:                                          # the last cell row wholly behind, across at least one tile border:
            border = -(-last[0] // 32) * 32            # components of it with pixels on both sides of that border
            assert row < last[0] < border < H and last[1] > 32
            crossing = (t["y0"] >= last[0]) & (t["y0"] < border) & (t["y1"] > border)
        assert crossing.sum() >= 3, (case["id"], b)
        assert t["area"][crossing].max() > 1000        # a snake or a percolation cluster among them
        _both_sides(t["first"], 256 * sizes[0], (case["id"], b))


# ------------------------------------------------------------------------------------------------ run-length cases

@pytest.mark.parametrize("case", oc.RLE_BLOCK_CASES, ids=[c["id"] for c in oc.RLE_BLOCK_CASES])
def test_rle_block_cases_reach_the_second_round(hip_lib, sizes, case):
    H, W = case["shape"]
    _, P, R = sizes
    want, counts = oc.rle_block_expected(H, W)
    ids = want["ids"]
    assert counts[0] != counts[1] and min(counts) > 1024
    runs = oc.rle_block_runs(H, W, case["order"], P)
    assert [c - counts[0] for c, _ in runs[:3]] == [5, 0, -(counts[0] - counts[0] // 2)]       # above, at, below
    for cap, max_runs in runs:
        q = oc.rle_rounds(hip_lib, H, W, cap, max_runs, case["order"])
        assert q[case["loop"]] >= case["least"] and q["blocks"] == (H * W + 1 + P - 1) // P > 1024
        assert q["offsets_scan"] >= 2 and q["table_scan"] >= 2              # cap + 1 > 1024 words; more than 4 chunks
    assert oc.rle_rounds(hip_lib, H, W, 5, 5, case["order"])["blocks"] == (1025 if H * W == 1024 * P else 1027)
    cap, cut = runs[3]
    for b in range(oc.B):
        v = rr.flatten(ids[b], case["order"])
        assert v[-1] != 0                                                  # the last run is closed at position H * W
        st = oc.starts_of(np.where(v <= cap, v, 0))
        if H * W > 1024 * P:
            _both_sides(st, 1024 * P, (case["id"], b, "runs start on both sides of block 1024"))
            if b == 0:
                before = int((st < 1024 * P).sum())
                assert before < cut < len(st)                              # the cut leaves records of the second round
        else:
            assert H * W == 1024 * P and len(st) > 1024                     # block 1024 holds position H * W alone
    full = rr.rle(ids, cap, H * W, case["order"])
    assert (full["nruns"][:, 0] == full["nruns"][:, 1]).all() and full["nruns"][0, 1] != full["nruns"][1, 1]


@pytest.mark.parametrize("case", oc.RLE_TABLE_CASES, ids=[c["id"] for c in oc.RLE_TABLE_CASES])
def test_rle_table_cases_reach_two_and_three_rounds(hip_lib, sizes, case):
    _, P, R = sizes
    H, W = oc.TABLE_SHAPE
    ids = oc.table_ids(case["cap"])
    for M, rounds in oc.table_cuts(R).items():
        q = oc.rle_rounds(hip_lib, H, W, case["cap"], M, "row")
        assert q["table_scan"] == rounds and q["passes"] == case["passes"]
        for order in rr.ORDERS:
            _records_fill_the_rounds([rr.flatten(i, order) for i in ids], case["cap"], M, R, rounds)


def _records_fill_the_rounds(streams, top, M, R, rounds):
    """The kept records of both images, by the low byte of their key and their chunk, lie in every round of the first
    pass's table scan; image 1 keeps fewer records than image 0, which is cut at M."""
    nchunk = -(-M // R)
    kept = []
    for v in streams:
        v = np.where((v >= 1) & (v <= top), v, 0)
        st = oc.starts_of(v)[:M]
        word = (v[st] & 255) * nchunk + np.arange(len(st)) // R
        assert set((word // 1024).tolist()) == set(range(rounds)), (M, rounds)
        kept.append(len(st))
    assert kept[0] == M > kept[1] > 4 * R // 2


@pytest.mark.parametrize("case", oc.MATCH_TABLE_CASES, ids=[c["id"] for c in oc.MATCH_TABLE_CASES])
def test_match_table_cases_reach_two_and_three_rounds(hip_lib, sizes, case):
    _, P, R = sizes
    H, W = oc.TABLE_SHAPE
    cp, cg = case["caps"]
    pids, gids = oc.table_ids(cp), oc.table_ids(cg, True)
    for M, rounds in oc.table_cuts(R).items():
        q = oc.match_rounds(hip_lib, H, W, cp, cg, M, case["max_pairs"])
        assert q["table_scan"] == rounds and q["passes"] == case["passes"]
        _records_fill_the_rounds([mr.keys(pids[b], gids[b], cp, cg) for b in range(oc.B)], (cp + 1) * (cg + 1), M, R, rounds)


# ------------------------------------------------------------------------------------------------ matching cases

@pytest.mark.parametrize("case", oc.MATCH_BLOCK_CASES, ids=[c["id"] for c in oc.MATCH_BLOCK_CASES])
def test_match_block_cases_reach_the_second_round(hip_lib, sizes, case):
    H, W = case["shape"]
    _, P, R = sizes
    cp, cg = case["caps"]
    q = oc.match_rounds(hip_lib, H, W, cp, cg, case["max_records"], case["max_pairs"])
    assert q[case["loop"]] >= case["least"] and q["blocks"] > 1024 and q["table_scan"] >= 2 and q["passes"] == 3
    p, g = oc.match_block_expected(H, W)
    gts = oc.match_block_inputs(H, W)[2]
    assert (gts == 255).any()
    for b in range(oc.B):
        assert 100 < p["n"][b, 0] <= cp and 100 < g["n"][b, 0] <= cg                          # a few hundred objects a side
        assert g["n"][b, 0] < g["n"][b, 1]                                 # the filter removed the flipped single pixels
        k = mr.keys(p["ids"][b], g["ids"][b], cp, cg, gts[b])
        st = oc.starts_of(k)
        assert 8 * R < len(st) <= case["max_records"]                       # nothing truncates, the sort table has rounds
        assert len(np.unique(k[st])) <= case["max_pairs"]
        if H * W > 1024 * P:
            _both_sides(st, 1024 * P, (case["id"], b, "records start on both sides of block 1024"))
        else:
            assert k[-1] != 0                                              # the last record is closed at position H * W
    assert not np.array_equal(p["ids"][0], p["ids"][1])


def test_chain_and_heads_cases(hip_lib, sizes):
    PC, P, R = sizes
    c = oc.CHAIN
    H, W = c["shape"]
    assert oc.components_rounds(hip_lib, H, W, 0)[c["loop"]] >= c["least"]
    for which in (0, 1):
        labels, gts, p, g, runs, m = oc.chain_expected(which)
        for side, cap in zip((p, g), c["caps"]):
            assert (100 < side["n"][:, 0]).all() and (side["n"][:, 0] <= cap).all()               # every object has a row
        for b in range(oc.B):                                              # the prediction numbers objects behind block 256
            _both_sides(p["stats"][b, :p["n"][b, 0], 6], 256 * PC, ("chain", which, b))
        assert (runs["nruns"][:, 0] > 4 * R).all() and (m["n"][:, 2] > 4 * R).all() and m["pq"][:, 1:, 0].sum() > 10
    assert not np.array_equal(oc.chain_expected(0)[0], oc.chain_expected(1)[0])
    h = oc.HEADS
    q = oc.match_rounds(hip_lib, *h["shape"], *h["caps"], 1024 * R, h["max_pairs"])
    assert q[h["loop"]] >= h["least"]
    assert oc.match_rounds(hip_lib, *h["shape"], *h["caps"], 1024 * R - 1, h["max_pairs"])[h["loop"]] == 1
    from diffews_amd import ops
    assert 0 < ops.seg_match_workspace(oc.B, *h["shape"], *h["caps"], 1024 * R, h["max_pairs"]) < 100 << 20
