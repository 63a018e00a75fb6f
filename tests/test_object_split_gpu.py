"""GPU tests of the instance split, byte for byte against tests/split_ref.py (which tests/test_object_split_cpu.py holds
against the per-pixel definition): ops_split.seg_nearest at the shapes where its kernels change path -- four pixels a thread
and one, buffers one element off alignment, a row, a run and a reach across the border of a workgroup of the row pass, one
row, one column, one pixel, one row more than one and two tiles of the column pass, reach 1 and 254, ties, gaps, other
objects, passes 1, 2, 3 and 8, two images, extreme seed values; ops_split.seg_components_keyed around the tile of the LDS
pass; then objects.split_objects and what every later stage makes of its result, captured graphs, LDS poison and repeated
launches, and pipe.split_objects on the tiny engine.  The sizes come from dfw_seg_boundary_block and
dfw_seg_components_tile.  All integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_ref as cr
import edt_ref as er
import split_ref as sr
import test_object_boundaries_gpu as tb
from test_object_boundaries_gpu import pipe  # noqa: F401  (the tiny engine, a module fixture)

pytestmark = pytest.mark.gpu

NLAB = 3


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def sp(hip_lib):
    from diffews_amd import ops_split
    return ops_split


@pytest.fixture(scope="module")
def block(ops):
    return ops.seg_boundary_block()                                        # rows, cols of the column tile; row positions


@pytest.fixture(scope="module")
def tile(hip_lib):
    th, tw = C.c_int32(), C.c_int32()
    assert hip_lib.dfw_seg_components_tile(C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


# ------------------------------------------------------------------------------------------------ the nearest seed

def _nearest(sp, m, s, R, passes=1, off=False, fill=None, repeat=1):
    """ops_split.seg_nearest on numpy maps [B, H, W] in guarded buffers; `off` puts every buffer one element into its
    allocation (one pixel a thread).  Returns (nearest, dist) after checking every guard and both inputs."""
    B, H, W = m.shape
    pad = 61 if off else 4
    bufs = dict(map=tb._Guarded(m.shape, torch.int32, pad), seeds=tb._Guarded(m.shape, torch.int32, pad),
                nearest=tb._Guarded(m.shape, torch.int32, pad, fill), dist=tb._Guarded(m.shape, torch.uint16, 1 if off else 32, fill),
                ws=tb._Guarded((sp.seg_nearest_workspace(B, H, W),), torch.uint8, 68 if off else 64, fill))
    bufs["map"].t.copy_(torch.from_numpy(m))
    bufs["seeds"].t.copy_(torch.from_numpy(s))
    for _ in range(repeat):
        sp.seg_nearest(bufs["map"].t, bufs["seeds"].t, bufs["nearest"].t, bufs["dist"].t, bufs["ws"].t, R, passes)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert np.array_equal(bufs["map"].t.cpu().numpy(), m) and np.array_equal(bufs["seeds"].t.cpu().numpy(), s), "an input was modified"
    return bufs["nearest"].t.cpu().numpy(), bufs["dist"].t.cpu().numpy()


def _check(sp, m, s, R, passes, off, what, want=None, **kw):
    m, s = np.ascontiguousarray(m, np.int32), np.ascontiguousarray(s, np.int32)
    if m.ndim == 2:
        m, s = m[None], s[None]
    wn, wd = sr.nearest_ref(m, s, R, passes) if want is None else want
    near, dist = _nearest(sp, m, s, R, passes, off, **kw)
    tag = (what, m.shape, R, passes, off)
    assert near.dtype == np.int32 and np.array_equal(near, wn), tag + ("nearest", int((near != wn).sum()), np.argwhere(near != wn)[:4].tolist())
    assert dist.dtype == np.uint16 and np.array_equal(dist, wd), tag + ("dist", int((dist != wd).sum()), np.argwhere(dist != wd)[:4].tolist())
    return near, dist


def _ids_and_cores(lab, radius=2):
    """ids and core ids (the seeds split_objects would use) of uint8 label maps [B, H, W], from the references."""
    ids = cr.components(lab, 8, 0, lab[0].size + 1)["ids"]
    core = np.where(er.dist2_ref(ids, max(radius, 1)).astype(np.int64) > radius * radius, lab, 0).astype(np.uint8)
    return ids, cr.components(core, 8, 0, lab[0].size + 1)["ids"]


def _family_maps(H, W, n=2):
    return np.stack([sr.family(seed, H, W) for seed in sr.FAMILY_SEEDS[:n]])


@pytest.mark.parametrize("vec", [True, False], ids=["W%4==0", "W%4!=0"])
def test_nearest_on_the_family_both_paths_and_two_images(sp, block, vec):
    """Two different images of the random family over more than two tiles of the column pass a side: aligned buffers take
    four pixels a thread when W % 4 == 0, one otherwise; buffers one element off always take one.  Passes 1, 2, 3."""
    R_, Cc, P = block
    H, W = 2 * R_ + 9, (2 * Cc + 16 if vec else 2 * Cc + 15)
    assert H >= 40 and W >= 52 and (W % 4 == 0) == vec and H * W > P
    ids, seeds = _ids_and_cores(_family_maps(H, W))
    assert not np.array_equal(ids[0], ids[1])
    for passes in (1, 2, 3):
        for off in (False, True):
            near, _ = _check(sp, ids, seeds, sr.FAMILY["reach"], passes, off, "family")
    assert ((near == 0) & (ids != 0)).any() and (near != 0).any()


@pytest.mark.parametrize("shape", ["1x1", "1xW", "Hx1", "rows+1", "2rows+1"])
def test_nearest_small_shapes_and_one_row_more_than_the_tile(sp, block, shape):
    R_, Cc, P = block
    H, W = {"1x1": (1, 1), "1xW": (1, 37), "Hx1": (37, 1), "rows+1": (R_ + 1, Cc + 1), "2rows+1": (2 * R_ + 1, 12)}[shape]
    assert (R_, 2 * R_) == (16, 32) or shape not in ("rows+1", "2rows+1") or (H - 1) % R_ == 0
    rs = np.random.RandomState(H * 100 + W)
    for t in range(4):
        m = ((rs.rand(2, H, W) < 0.85) * rs.randint(1, 3, (2, H, W))).astype(np.int32)
        s = ((rs.rand(2, H, W) < (0.5 if H * W < 40 else 0.03)) * rs.randint(-2, 9, (2, H, W))).astype(np.int32)
        if t == 0:
            m[:], s[:] = 4, 0
            s[0, 0, 0], s[1, -1, -1] = 3, 7                                # one object, one seed: the far end is H - 1 away
        for R, passes in ((1, 1), (3, 2), (max(H, W), 1), (40, 3)):
            _check(sp, m, s, min(R, 254), passes, t % 2 == 1, shape)


def test_nearest_across_the_border_of_a_row_block(sp, block):
    """A row longer than a workgroup of the row pass, a run that crosses the border, and a seed exactly `reach` away on the
    other side of it: the pixel that sees it at distance reach, and its neighbour that sees nothing."""
    R_, Cc, P = block
    W = P + 300
    m = np.full((1, 3, W), 6, np.int32)
    m[0, 1] = 7                                                            # rows 0 and 2 do not see each other
    m[0, 2, P - 40:P - 30] = 9                                             # row 2: a run that ends before the border, one across it
    s = np.zeros_like(m)
    s[0, 0, P + 150] = 5                                                   # row 0: one seed beyond the border
    s[0, 2, P + 3], s[0, 2, P - 45] = 8, 2                                 # 2 lies behind the gap of 9
    for R in (254, 100):
        near, dist = _check(sp, m, s, R, 1, R == 100, "border")
        assert near[0, 0, P + 150 - R] == 5 and dist[0, 0, P + 150 - R] == R * R and near[0, 0, P + 150 - R - 1] == 0
        assert near[0, 0, P - 1] == (5 if R == 254 else 0) and near[0, 2, P - 10] == 8 and near[0, 2, P - 35] == 0
    # three rows of exactly one block each, and a block that ends inside a row: the window's halo lies in other rows
    for H, W in ((3, P), (5, P // 2 + 3)):
        rs = np.random.RandomState(W)
        m = np.kron(rs.randint(0, 3, (1, H, W // 64 + 1)), np.ones((1, 1, 64), np.int64))[:, :, :W].astype(np.int32)
        s = ((rs.rand(1, H, W) < 0.004) * rs.randint(1, 99, (1, H, W))).astype(np.int32)
        s[0, :, 0], s[0, :, -1] = 11, 12                                   # seeds at both ends of every row: never seen from
        _check(sp, m, s, 254, 2, False, "rows of a block")                 # the row before or behind
        _check(sp, m, s, 200, 1, True, "rows of a block")


def test_nearest_reach_1_and_reach_254_on_300_rows(sp, block):
    R_, Cc, P = block
    H, W = 300, 24
    assert H > 254 + R_
    m = np.full((1, H, W), 3, np.int32)
    m[0, :, 4:8], m[0, :, 20:] = 8, 0                                      # three strips: 3, 8, 3, then background
    m[0, 140, 5] = 0                                                       # column 5 is cut: nothing passes through
    s = np.zeros_like(m)
    s[0, 0, 2], s[0, H - 1, 17], s[0, 150, 5] = 21, 22, -4
    near, dist = _check(sp, m, s, 254, 1, False, "reach 254")
    assert near[0, 254, 2] == 21 and dist[0, 254, 2] == 254 * 254 and near[0, 255, 2] == 0 and dist[0, 255, 2] == 255 * 255
    assert near[0, 139, 5] == 0 and near[0, 139, 4] == -4 and near[0, 141, 5] == -4   # above the cut only round it
    _check(sp, m, s, 254, 2, True, "reach 254, offset")
    near, dist = _check(sp, m, s, 1, 1, False, "reach 1")
    assert (near != 0).sum() == 4 + 4 + 5 and int(dist.max()) == 4         # the seeds and their 4-neighbours
    _check(sp, m, s, 1, 8, True, "reach 1, eight passes")


def test_nearest_named_cases_passes_1_2_3_and_8(sp):
    """Ties left / right and up / down, equal distances with different values, a gap, another object, extreme seed values,
    a seed on background, a comb and a U -- one to eight passes, aligned and one element off."""
    for name, (m, s, R) in sr.named_cases().items():
        for passes in (1, 2, 3, 8):
            for off in (False, True):
                near, dist = _check(sp, m, s, R, passes, off, name)
        if name.startswith(("a comb", "a U")):
            assert np.array_equal(near != 0, m[None] != 0)                 # eight passes reach everything, two did already
            one, _ = _check(sp, m, s, R, 1, False, name)
            assert ((one == 0) & (m[None] != 0)).any()
        if name.startswith("seed values"):
            assert near[0, 0, 0] == (1 << 31) - 1 and near[0, 4, 4] == -(1 << 31) and near[0, 2, 2] == -(1 << 31)
    # W % 4 == 0, so the ties are also seen four pixels a thread
    m = np.full((9, 8), 5, np.int32)
    s = np.zeros_like(m)
    s[4, 1], s[4, 7], s[0, 4], s[8, 4], s[2, 2] = 9, 3, 6, 2, 1
    for R in (2, 3, 4, 9):
        _check(sp, m, s, R, 1, False, "ties, four pixels a thread")


def test_nearest_poisoned_and_repeated_launches_give_the_same_bits(sp, block):
    """Outputs and workspace pre-filled with different bytes, two launches back to back into the same buffers (the second
    one's later passes meet a `nearest` that is already full), aligned and offset: the same bytes every time."""
    R_, Cc, P = block
    ids, seeds = _ids_and_cores(_family_maps(2 * R_ + 9, 2 * Cc + 16))
    want = sr.nearest_ref(ids, seeds, 8, 3)
    for fill in (0x00, 0xFF, 0x5A):
        for off in (False, True):
            _check(sp, ids, seeds, 8, 3, off, "poisoned", want, fill=fill, repeat=2)


@pytest.mark.parametrize("off", [False, True], ids=["four pixels a thread", "one pixel a thread"])
def test_nearest_lds_poison(sp, block, off):
    """Plain, then with every CU's LDS filled with 0xFF, 0x7B and 0x00 in front of the call: byte-equal, and equal to the
    reference.  The row pass reads its two windows, its bytes of h and the waves' scan ends from LDS."""
    from test_lds_poison_gpu import four_runs
    R_, Cc, P = block
    ids, seeds = _ids_and_cores(_family_maps(2 * R_ + 9, 2 * Cc + 16))
    want = sr.nearest_ref(ids, seeds, 8, 2)

    def check(got):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    four_runs("dfw_seg_components", lambda: _nearest(sp, ids, seeds, 8, 2, off), check, ("seg_nearest", off))


@pytest.mark.parametrize("passes", [1, 3])
def test_nearest_captured_graph_has_two_kernel_nodes_a_pass(sp, hip_lib, block, passes):
    R_, Cc, P = block
    H, W = 2 * R_ + 9, 2 * Cc + 16
    maps = [_ids_and_cores(_family_maps(H, W)), _ids_and_cores(_family_maps(H, W)[::-1].copy())]
    ids, seeds = (torch.zeros(2, H, W, dtype=torch.int32, device="cuda") for _ in range(2))
    near, dist = torch.empty_like(ids), torch.empty(2, H, W, dtype=torch.uint16, device="cuda")
    ws = torch.empty(sp.seg_nearest_workspace(2, H, W), dtype=torch.uint8, device="cuda")

    def call():
        sp.seg_nearest(ids, seeds, near, dist, ws, 8, passes)
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    nodes = C.c_int32()
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0     # no memset node
    assert nodes.value == 2 * passes
    graph.instantiate()
    for m, s in maps + [maps[0]]:
        ids.copy_(torch.from_numpy(m))
        seeds.copy_(torch.from_numpy(s))
        graph.replay()
        torch.cuda.synchronize()
        wn, wd = sr.nearest_ref(m, s, 8, passes)
        assert np.array_equal(near.cpu().numpy(), wn) and np.array_equal(dist.cpu().numpy(), wd)


# ------------------------------------------------------------------------------------------------ keyed components

def _keyed(sp, ops, labels, keys, conn, min_area, cap, gt=None, off=False, fill=None, repeat=1):
    """ops_split.seg_components_keyed (ops.seg_components when keys is None) into guarded buffers; numpy results."""
    B, H, W = labels.shape
    pad = 61 if off else 64
    bufs = dict(labels=tb._Guarded((B, H, W), torch.uint8, pad), ids=tb._Guarded((B, H, W), torch.int32, 1 if off else 4, fill),
                n=tb._Guarded((B, 2), torch.int32, 4, fill), ws=tb._Guarded((ops.seg_components_workspace(B, H, W),), torch.uint8, 64, fill),
                filtered=tb._Guarded((B, H, W), torch.uint8, pad, fill), stats=tb._Guarded((B, cap, 8), torch.int32, 4, fill))
    if keys is not None:
        bufs["keys"] = tb._Guarded((B, H, W), torch.int32, 1 if off else 4)
        bufs["keys"].t.copy_(torch.from_numpy(np.ascontiguousarray(keys, np.int32)))
    if gt is not None:
        bufs["gt"], bufs["counts"] = tb._Guarded((B, H, W), torch.uint8, pad), tb._Guarded((B, 2, NLAB + 1), torch.int64, 2, fill)
        bufs["gt"].t.copy_(torch.from_numpy(gt))
    bufs["labels"].t.copy_(torch.from_numpy(labels))
    g = {k: v.t for k, v in bufs.items()}
    kw = dict(filtered=g["filtered"], stats=g["stats"], gt=g.get("gt"), counts=g.get("counts"), connectivity=conn, min_area=min_area,
              nlabels=NLAB if gt is not None else None)
    for _ in range(repeat):
        if keys is None:
            ops.seg_components(g["labels"], g["ids"], g["n"], g["ws"], **kw)
        else:
            sp.seg_components_keyed(g["labels"], g["keys"], g["ids"], g["n"], g["ws"], **kw)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert np.array_equal(g["labels"].cpu().numpy(), labels), "the labels were modified"
    return {k: g[k].cpu().numpy() for k in ("ids", "n", "filtered", "stats", "counts") if k in g}


def _same(got, want, what):
    for k in ("ids", "n", "filtered", "stats", "counts"):
        if k in got:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


def _gt(shape, rs):
    g = rs.randint(0, NLAB + 1, shape).astype(np.uint8)
    g[rs.rand(*shape) < 0.05] = 255
    return g


def _keyed_contents(H, W, th, tw, rs):
    """{name: (labels uint8 [H, W], keys [H, W])}: one per way the pair comparison can go wrong."""
    yy, xx = np.mgrid[:H, :W]
    out = {}
    out["random bytes and keys"] = (((rs.rand(H, W) < 0.7) * rs.randint(1, NLAB + 1, (H, W))), rs.randint(-1, 2, (H, W)))
    out["one byte, random keys"] = (np.full((H, W), 2), rs.randint(0, 2, (H, W)))
    out["only the key differs at the tile borders"] = (np.full((H, W), 1), (yy // th) * 1000 - (xx // tw))
    out["only the key differs one pixel off the borders"] = (np.full((H, W), 1), ((yy + 1) // th) * 7 + ((xx + 1) // tw))
    above = np.where((yy + xx) % 2 == 0, 5, -5)                            # equal byte, another key above and beside: only the
    out["checkerboard of keys"] = (np.full((H, W), 3), above)              # diagonals join, across every border
    stripes = np.where(yy % 2 == 0, xx // 3, -1 - (xx + 1) // 3)           # the pixel above differs in the key alone
    out["the diagonal shortcut"] = (np.where(rs.rand(H, W) < 0.9, 1, 0), stripes)
    big = np.array([0, -(1 << 31), (1 << 31) - 1, -1])[(yy // 5 + xx // 7) % 4]
    out["keys 0, negative and 2^31 - 1"] = (1 + (xx // 11) % 2, big)
    out["background with keys"] = (np.zeros((H, W)), rs.randint(0, 3, (H, W)))
    return {k: (a.astype(np.uint8), b.astype(np.int32)) for k, (a, b) in out.items()}


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", ["tile+1", "two tiles and more"])
def test_keyed_components_equal_the_reference(sp, ops, tile, shape, conn):
    """33 x 65 and 70 x 131 at the tile of 32 x 64: the scalar path of every kernel (odd widths), then 72 x 132 on the word
    path; min_area, a stats table that is cut short, and counts."""
    th, tw = tile
    shapes = [(th + 1, tw + 1)] if shape == "tile+1" else [(2 * th + 6, 2 * tw + 3), (2 * th + 8, 2 * tw + 4)]
    for H, W in shapes:
        rs = np.random.RandomState(H * W + conn)
        gt = _gt((1, H, W), rs)
        for i, (name, (lab, keys)) in enumerate(_keyed_contents(H, W, th, tw, rs).items()):
            for min_area, cap in ((0, H * W), (3, 5)):
                want = sr.components_keyed(lab[None], keys[None], conn, min_area, cap, gt, NLAB)
                want["counts"] = want["counts"].astype(np.int64)
                got = _keyed(sp, ops, lab[None], keys[None], conn, min_area, cap, gt, off=(i % 2 == 1))
                _same(got, want, (name, H, W, conn, min_area, cap))
                if name == "checkerboard of keys":
                    assert got["n"][0, 1] == (2 if conn == 8 else H * W)
                if name == "only the key differs at the tile borders" and min_area == 0:
                    assert got["n"][0, 0] == -(-H // th) * -(-W // tw)
                if cap == 5 and name.startswith("random"):
                    assert got["n"][0, 0] > cap                            # only stats is cut short


def test_keyed_components_with_equal_keys_and_without_keys(sp, ops, tile):
    """keys all equal: byte for byte the keyless call.  B = 2, word and scalar path."""
    th, tw = tile
    for H, W in ((th + 1, tw + 1), (2 * th + 8, 2 * tw + 4)):
        rs = np.random.RandomState(H)
        lab = ((rs.rand(2, H, W) < 0.6) * rs.randint(1, NLAB + 1, (2, H, W))).astype(np.uint8)
        gt = _gt(lab.shape, rs)
        for conn in (4, 8):
            plain = _keyed(sp, ops, lab, None, conn, 2, 40, gt)
            ref = cr.components(lab, conn, 2, 40, gt, NLAB)
            _same(plain, ref, "keyless")
            for value in (0, -3, 1 << 30):
                _same(_keyed(sp, ops, lab, np.full(lab.shape, value), conn, 2, 40, gt, fill=0xFF), plain, ("equal keys", value))


def test_keyed_poisoned_repeated_and_lds_poison(sp, ops, tile):
    from test_lds_poison_gpu import four_runs
    th, tw = tile
    H, W = 2 * th + 6, 2 * tw + 4
    rs = np.random.RandomState(77)
    lab = ((rs.rand(2, H, W) < 0.75) * rs.randint(1, NLAB + 1, (2, H, W))).astype(np.uint8)
    keys = rs.randint(0, 3, lab.shape).astype(np.int32)
    gt = _gt(lab.shape, rs)
    want = sr.components_keyed(lab, keys, 8, 2, 64, gt, NLAB)
    for fill in (0x00, 0xFF, 0x5A):
        for off in (False, True):
            _same(_keyed(sp, ops, lab, keys, 8, 2, 64, gt, off, fill, repeat=2), want, ("poisoned", fill, off))
    for off in (False, True):
        four_runs("dfw_seg_components", lambda: _keyed(sp, ops, lab, keys, 8, 2, 64, gt, off), lambda got: _same(got, want, "lds"), ("keyed", off))


@pytest.mark.parametrize("one_tile", [False, True], ids=["8 launches", "7 launches"])
def test_keyed_and_keyless_calls_have_the_same_kernel_nodes(sp, ops, hip_lib, tile, one_tile):
    """With keys null the launches are the parent's, 8 (7 for an image of one tile), and the keyed call has as many."""
    th, tw = tile
    H, W = (th, tw) if one_tile else (th + 1, tw + 1)
    rs = np.random.RandomState(9)
    lab = torch.from_numpy(((rs.rand(1, H, W) < 0.6) * rs.randint(1, 4, (1, H, W))).astype(np.uint8)).cuda()
    keys = torch.from_numpy(rs.randint(0, 2, (1, H, W)).astype(np.int32)).cuda()
    ids, n = torch.empty(1, H, W, dtype=torch.int32, device="cuda"), torch.empty(1, 2, dtype=torch.int32, device="cuda")
    stats = torch.empty(1, 16, 8, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.seg_components_workspace(1, H, W), dtype=torch.uint8, device="cuda")
    for keyed in (False, True):
        def call():
            if keyed:
                sp.seg_components_keyed(lab, keys, ids, n, ws, stats=stats)
            else:
                ops.seg_components(lab, ids, n, ws, stats=stats)
        call()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            call()
        nodes = C.c_int32()
        assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0
        assert nodes.value == (7 if one_tile else 8), keyed
        graph.instantiate()
        graph.replay()
        torch.cuda.synchronize()
        want = (sr.components_keyed(lab.cpu().numpy(), keys.cpu().numpy(), 8, 0, 16) if keyed
                else cr.components(lab.cpu().numpy(), 8, 0, 16))
        assert np.array_equal(ids.cpu().numpy(), want["ids"]) and np.array_equal(stats.cpu().numpy(), want["stats"])


# ------------------------------------------------------------------------------------------------ the composition

def _two_discs():
    yy, xx = np.mgrid[:64, :64]
    return (((yy - 32) ** 2 + (xx - 20) ** 2 <= 196) | ((yy - 32) ** 2 + (xx - 42) ** 2 <= 196)).astype(np.uint8)


def _squares_and_bridge():
    lab = np.zeros((14, 26), np.uint8)
    lab[2:12, 1:11] = lab[2:12, 15:25] = 1
    lab[6:8, 11:15] = 1
    return lab


def _np(r, *keys):
    return [r[k].cpu().numpy() for k in keys]


def _split_equals_reference(r, o, radius, reach, passes, min_area, cap, conn=8):
    ids, labels = _np(o, "ids", "labels")
    squeeze = ids.ndim == 2
    if squeeze:
        ids, labels = ids[None], labels[None]
    want = sr.split_ref(ids, labels, radius, reach, passes, min_area, conn, cap)
    for k in ("ids", "n", "stats", "parent", "nearest", "cores"):
        got = r[k].cpu().numpy()
        assert np.array_equal(got.reshape(want[k].shape), want[k]), (k, radius, reach, passes)
    assert np.array_equal(r["labels"].cpu().numpy().reshape(want["filtered"].shape), want["filtered"]) and r["counts"] is None
    return want


def test_split_worked_examples(hip_lib):
    from diffews_amd.objects import label_objects, objects_to_host, split_objects
    lab = torch.from_numpy(_two_discs()).cuda()
    o = label_objects(lab, connectivity=8, max_components=16)
    r = split_objects(o, 10, reach=22, passes=1)
    _split_equals_reference(r, o, 10, 22, 1, 0, 16)
    objs, cut = objects_to_host(r)
    assert [(c, a) for c, a, _, _ in objs] == [(1, 586), (1, 569)] and not cut
    assert r["cores"].tolist() == [2, 2] and r["parent"].tolist()[:3] == [1, 1, 0] and r["ids"].dim() == 2
    assert not ((r["nearest"] == 0) & (lab != 0)).any()                    # no pixel unassigned
    o = label_objects(torch.from_numpy(_squares_and_bridge()).cuda(), max_components=16)
    r = split_objects(o, 3, reach=8, passes=1)
    _split_equals_reference(r, o, 3, 8, 1, 0, 16)
    assert [a for _, a, _, _ in objects_to_host(r)[0]] == [104, 104]
    assert r["ids"][6:8, 11:15].tolist() == [[1, 1, 2, 2], [1, 1, 2, 2]]  # the bridge is cut down its middle
    # the defaults: reach = min(254, 2 * radius + 2), three passes
    _split_equals_reference(split_objects(o, 3), o, 3, 8, 3, 0, 16)


def test_split_on_the_family_what_it_promises(hip_lib, block):
    from diffews_amd.objects import SplitBuffers, label_objects, split_objects
    R_, Cc, P = block
    F = sr.FAMILY
    lab = np.stack([sr.family(seed) for seed in sr.FAMILY_SEEDS])
    B, H, W = lab.shape
    cap = 128
    o = label_objects(torch.from_numpy(lab).cuda(), connectivity=F["connectivity"], max_components=cap)
    buffers = SplitBuffers(B, H, W, cap)
    for _ in range(2):                                                     # the buffers again: the same result
        r = split_objects(o, F["radius"], reach=F["reach"], passes=F["passes"], buffers=buffers, connectivity=F["connectivity"])
        assert r["ids"].data_ptr() == buffers.out.ids.data_ptr() and r["parent"].data_ptr() == buffers.parent.data_ptr()
        assert r["nearest"].data_ptr() == buffers.nearest.data_ptr()
        want = _split_equals_reference(r, o, F["radius"], F["reach"], F["passes"], 0, cap)
    ids, stats, n, parent, oi, ol = _np(r, "ids", "stats", "n", "parent") + _np(o, "ids", "labels")
    assert np.array_equal(ids != 0, ol != 0)                               # no pixel lost with min_area = 0
    assert (n[:, 0] > _np(o, "n")[0][:, 0]).all() and (n[:, 0] <= cap).all()
    for b in range(B):
        for k in range(1, int(n[b, 0]) + 1):
            inside = np.unique(oi[b][ids[b] == k])
            assert inside.tolist() == [parent[b, k - 1]], (b, k)           # every instance lies inside one parent
        assert not parent[b, int(n[b, 0]):].any()
        # every instance is connected: each id is ONE component of its own mask
        for k in range(1, int(n[b, 0]) + 1):
            assert cr.components((ids[b] == k).astype(np.uint8)[None], F["connectivity"], 0, 4)["n"][0, 0] == 1, (b, k)
    # a speck filter removes the unreached fragments like any other
    r5 = split_objects(o, F["radius"], reach=F["reach"], passes=F["passes"], min_area=5)
    _split_equals_reference(r5, o, F["radius"], F["reach"], F["passes"], 5, cap)
    assert (r5["n"][:, 0] < r5["n"][:, 1]).all()
    # a radius above every object's thickness: no cores, keys all 0, o's own ids, stats and n
    thick = split_objects(o, 40)
    assert not thick["cores"].any() and not thick["nearest"].any()
    for k in ("ids", "stats", "n", "labels"):
        assert torch.equal(thick[k], o[k]), k
    rows = np.arange(cap)[None]
    assert np.array_equal(thick["parent"].cpu().numpy(), np.where(rows < _np(o, "n")[0][:, :1], rows + 1, 0))
    del want


def test_split_result_passes_through_the_later_stages(hip_lib):
    """object_runs, object_contours, match_objects and object_scores take the result as it stands and find the areas of its
    stats; so do fill_holes, object_boundaries and object_thickness."""
    from diffews_amd.objects import (contours_to_host, fill_holes, label_objects, match_objects, matches_to_host,
                                     object_boundaries, object_contours, object_runs, object_scores, object_thickness,
                                     objects_to_host, planes_for_binary, rings_to_mask, runs_to_host, scores_to_host,
                                     split_objects)
    F = sr.FAMILY
    lab = np.stack([(sr.family(seed) != 0).astype(np.uint8) for seed in sr.FAMILY_SEEDS[:2]])
    B, H, W = lab.shape
    o = label_objects(torch.from_numpy(lab).cuda(), max_components=128)
    r = split_objects(o, F["radius"], reach=F["reach"], passes=F["passes"])
    objs, cut = objects_to_host(r)
    areas = [[a for _, a, _, _ in per] for per in objs]
    assert not cut and [len(a) for a in areas] == r["n"][:, 0].tolist() and all(len(a) > 3 for a in areas)
    runs, short = runs_to_host(object_runs(r))
    assert not short and [[int(k[:, 1].sum()) for k in per] for per in runs] == areas
    rings, incomplete = contours_to_host(object_contours(r))
    assert not incomplete and [[int(rings_to_mask(k, H, W).sum()) for k in per] for per in rings] == areas
    m, short = matches_to_host(match_objects(r, r, nlabels=1))
    cap = r["stats"].shape[1]
    for b in range(B):
        k = len(areas[b])
        assert not short and m["area"][b, 1:k + 1].tolist() == areas[b] and m["area"][b, cap + 2:cap + 2 + k].tolist() == areas[b]
        assert m["match"][b, :k, 0].tolist() == list(range(1, k + 1)) and m["pq"][b, 1, 0] == k
    seg = torch.from_numpy(np.broadcast_to(np.where(lab != 0, 200, 30).astype(np.uint8)[:, None], (B, 3, H, W)).copy()).cuda()
    sc = scores_to_host(object_scores(r, seg, planes_for_binary(B)))
    for b in range(B):
        assert sc["n"][b, :len(areas[b])].tolist() == areas[b] and (sc["min"][b, :len(areas[b])] == 600).all()
    filled = fill_holes(r)
    assert (filled["n"][:, 0] == r["n"][:, 0]).all()
    assert object_boundaries(r, d=2)["ids"]["band"].shape == (B, H, W) and object_thickness(r, dmax=9)["peaks"].shape == (B, cap)
    torch.cuda.synchronize()


def test_split_lists_and_single_maps(hip_lib):
    from diffews_amd.objects import label_objects, nearest_seeds, split_objects
    F = sr.FAMILY
    items = [torch.from_numpy(sr.family(1, 44, 60)).cuda(), torch.from_numpy(sr.family(2, 41, 53)).cuda()]
    ol = label_objects(items, max_components=96)
    rl = split_objects(ol, F["radius"], reach=F["reach"], passes=2)
    assert isinstance(rl["ids"], list) and set(rl) == {"ids", "labels", "n", "stats", "counts", "parent", "cores", "nearest"}
    for i in range(2):
        _split_equals_reference({k: v[i] for k, v in rl.items()}, {k: v[i] for k, v in ol.items()}, F["radius"], F["reach"], 2, 0, 96)
    near = nearest_seeds([o for o in ol["ids"]], [n for n in rl["nearest"]], 4, passes=1)
    assert near["reach"] == [4, 4] and near["shape"] == [(44, 60), (41, 53)]
    one = nearest_seeds(ol["ids"][0], rl["nearest"][0], 4)
    wn, wd = sr.nearest_ref(ol["ids"][0].cpu().numpy(), rl["nearest"][0].cpu().numpy(), 4, 1)
    assert np.array_equal(one["nearest"].cpu().numpy(), wn) and np.array_equal(one["dist"].cpu().numpy(), wd)
    assert torch.equal(one["nearest"], near["nearest"][0])
    # label_objects with keys: an int32 map labelled through (map != 0, map)
    ids = ol["ids"][0]
    again = label_objects((ids != 0).to(torch.uint8), keys=ids, max_components=96)
    assert torch.equal(again["ids"], ids)
    for bad in (lambda: label_objects(items[0], keys=ids.long()), lambda: label_objects(items[0], keys=ids[:, :-1]),
                lambda: split_objects(ol, 2, reach=0), lambda: split_objects(ol, 2, passes=9), lambda: nearest_seeds(ids, ids, 255)):
        with pytest.raises(ValueError):
            bad()


def test_split_captured_graph_replayed_on_two_maps(hip_lib):
    from diffews_amd.objects import ComponentBuffers, SplitBuffers, label_objects, split_objects
    F = sr.FAMILY
    maps = [np.stack([sr.family(s) for s in (1, 2)]), np.stack([sr.family(s) for s in (3, 1)])]
    B, H, W = maps[0].shape
    lab = torch.zeros(B, H, W, dtype=torch.uint8, device="cuda")
    cb, sb = ComponentBuffers(B, H, W, 96), SplitBuffers(B, H, W, 96)

    def call():
        o = label_objects(lab, max_components=96, buffers=cb)
        return o, split_objects(o, F["radius"], reach=F["reach"], passes=F["passes"], buffers=sb)
    lab.copy_(torch.from_numpy(maps[0]))
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        o, r = call()
    for m in maps + [maps[0]]:
        lab.copy_(torch.from_numpy(m))
        graph.replay()
        torch.cuda.synchronize()
        _split_equals_reference(r, o, F["radius"], F["reach"], F["passes"], 0, 96)


# ------------------------------------------------------------------------------------------------ the routes, tiny engine

def test_pipe_split_objects_on_the_binary_native_route(pipe):  # noqa: F811
    from diffews_amd.input_pipeline import NativeTargets
    from test_support_bank_gpu import _queries, _support_set
    sup, msk = _support_set(2, 64, seed=930)
    bank = pipe.prepare_support(sup.cuda(), msk.cuda())
    sizes = [(50, 70), (33, 41)]
    r = pipe.segment_queries(bank, _queries(2, 64, 79).cuda(), native=NativeTargets((64, 64), sizes), captured=False)
    o = pipe.objects(r, key="pred", connectivity=8, max_components=256)
    for res in (o, pipe.fill_holes(o)):
        s = pipe.split_objects(res, 1, passes=2)
        assert [tuple(i.shape) for i in s["ids"]] == sizes
        for i in range(2):
            _split_equals_reference({k: v[i] for k, v in s.items()}, {k: v[i] for k, v in res.items()}, 1, 4, 2, 0, 256)
