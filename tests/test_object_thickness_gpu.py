"""GPU tests of the Euclidean side of the boundary stage: ops.seg_boundary(metric="euclidean") with band and peaks, and
ops.seg_boundary_counts on squared maps, byte for byte against tests/edt_ref.py (the two-pass form in numpy, which
tests/test_object_thickness_cpu.py holds against the per-pixel definition) -- at one pixel, one row, one column, 2 x 2, 3 x
3, a tile of the column pass plus a row and a column, a width that takes four pixels a thread and one that takes one, a row
longer than a workgroup of the row pass with both halos, two and three images, uint8 and int32, the radii 1, 5 and 254 --
then the peaks table content by content, guarded, poisoned and repeated launches, LDS poison, a captured graph, the objects
layer and the pipeline's entry points.  The sizes come from ops.seg_boundary_block().  All integers."""
import ctypes as C

import numpy as np
import pytest
import torch

import boundary_ref as br
import edt_ref as er
import match_ref as mr
import rle_ref as rr
import test_object_boundaries_gpu as tb
from test_object_boundaries_gpu import pipe  # noqa: F401  (the tiny engine, a module fixture)

pytestmark = pytest.mark.gpu

DMAX_LIMIT = 254


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def tile(ops):
    return ops.seg_boundary_block()


def _launch(ops, m, dmax, d=None, off=False, fill=None, repeat=1, cap=None):
    """ops.seg_boundary(metric="euclidean") on a numpy map [B, H, W] in guarded buffers; `off` puts every buffer one element
    (the maps 3 bytes / 61 words) into its allocation, which takes the one-pixel-a-thread path.  Returns dict(dist2, band,
    peaks) as numpy after checking every guard and that the map did not change."""
    B, H, W = m.shape
    dt = torch.uint8 if m.dtype == np.uint8 else torch.int32
    mpad = (3 if off else 64) if dt == torch.uint8 else (61 if off else 4)
    bufs = dict(map=tb._Guarded(m.shape, dt, mpad), dist=tb._Guarded(m.shape, torch.uint16, 1 if off else 32, fill),
                ws=tb._Guarded((ops.seg_boundary_workspace(B, H, W, m.dtype.itemsize),), torch.uint8, 64, fill))
    if d is not None:
        bufs["band"] = tb._Guarded(m.shape, dt, mpad, fill)
    if cap is not None:
        bufs["peaks"] = tb._Guarded((B, cap), torch.int64, 4, fill)
    bufs["map"].t.copy_(torch.from_numpy(m))
    for _ in range(repeat):
        ops.seg_boundary(bufs["map"].t, bufs["dist"].t, bufs["ws"].t, dmax, band=bufs["band"].t if d is not None else None, d=d,
                         metric="euclidean", peaks=bufs["peaks"].t if cap is not None else None)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert np.array_equal(bufs["map"].t.cpu().numpy(), m), "the map was modified"
    return {k: bufs[k].t.cpu().numpy() for k in ("dist", "band", "peaks") if k in bufs}


def _check(ops, m, dmax, d, off, what, want=None, cap=None, **kw):
    want = er.dist2_ref(m, dmax) if want is None else want
    got = _launch(ops, m, dmax, d, off, cap=cap, **kw)
    dist = got["dist"]
    tag = (what, m.shape, str(m.dtype), dmax, d, off)
    assert dist.dtype == np.uint16 and np.array_equal(dist, want), tag + (int((dist != want).sum()),)
    assert np.array_equal(dist == 0, m == 0) and int(dist.max()) <= (dmax + 1) ** 2
    if d is not None:
        assert got["band"].dtype == m.dtype and np.array_equal(got["band"], er.band_ref(m, want, d)), tag
    if cap is not None:
        peaks = er.peaks_ref(m, want, cap)
        assert got["peaks"].dtype == np.int64 and np.array_equal(got["peaks"], peaks), tag + (np.flatnonzero(got["peaks"] != peaks)[:8],)
    return got


def _shapes(tile):
    R, Cc, P = tile
    halo = DMAX_LIMIT + 1                                                  # the least the row pass keeps on either side
    assert Cc % 16 == 0 and (2 * R + 3) * (2 * Cc + 16) > 2 * P
    return [(1, 1), (1, 37), (37, 1), (2, 2), (3, 3), (R + 1, Cc + 1), (2 * R + 3, 2 * Cc + 16), (2 * R + 3, Cc + 3),
            (3, P + 2 * halo + 7)]


@pytest.mark.parametrize("which", range(9), ids=["1x1", "1xW", "Hx1", "2x2", "3x3", "tile+row+column", "W%4==0", "W=cols+3",
                                                 "row longer than a block and its halos"])
def test_equals_the_reference(ops, tile, which):
    """Every content of the chessboard tests (one per way to go wrong; batches of two and three images among them), uint8
    and int32, dmax 1 and 5 with a band of d = 1, 2 and dmax from the same launch; aligned buffers (four pixels a thread
    where W % 4 == 0) and buffers one element off (one pixel a thread) alternate."""
    R, Cc, P = tile
    H, W = _shapes(tile)[which]
    if which == 6:
        assert W % 4 == 0 and H > 2 * R and W > 2 * Cc
    if which == 7:
        assert W % 4 != 0 and W > Cc
    rs = np.random.RandomState(1000 * H + W)
    case = 0
    for name, m64 in tb._contents(H, W, R, Cc, rs).items():
        for dtype in (np.uint8, np.int32):
            if dtype == np.uint8 and name.startswith("int32"):
                continue
            m = m64.astype(dtype)
            assert np.array_equal(m.astype(np.int64), m64)
            wants = {dmax: er.dist2_ref(m, dmax) for dmax in (1, 5)}
            for dmax, d in ((1, 1), (5, 2), (5, 5), (5, 1)):
                dist = _check(ops, m, dmax, d, case % 2 == 1, name, wants[dmax])["dist"]
                case += 1
                if name == "empty":
                    assert not dist.any()
                if name == "one value":                                    # the image border alone
                    yy, xx = np.mgrid[:H, :W]
                    edge = np.minimum(np.minimum(yy + 1, H - yy), np.minimum(xx + 1, W - xx))
                    assert np.array_equal(dist[0], np.minimum(edge, dmax + 1) ** 2)
                if name == "batch of one value":                           # nothing bleeds from image 0 into image 1
                    assert (dist[0, -1] == 1).all() and (dist[1, 0] == 1).all()


def test_radius_254(ops, tile):
    """dmax = 254 on one component of 520 x 520: a full square (uint8, four pixels a thread), whose centre is deeper than 254
    so that the cap is reached, and a disc of radius 258 (int32, one pixel a thread, with peaks); the walk of 254 rows
    crosses more than 30 tiles of the column pass."""
    R, Cc, P = tile
    H = W = 520
    assert 2 * DMAX_LIMIT > 30 * R and W % 4 == 0
    yy, xx = np.mgrid[:H, :W]
    edge = np.minimum(np.minimum(yy + 1, H - yy), np.minimum(xx + 1, W - xx))
    full = np.full((1, H, W), 77, np.uint8)
    want = er.dist2_ref(full, 254)
    assert np.array_equal(want[0], np.minimum(edge, 255) ** 2) and (want == 255 * 255).sum() > 0
    _check(ops, full, 254, 254, False, "square", want)
    disc = (((yy - 260) ** 2 + (xx - 260) ** 2 <= 258 ** 2) * 9).astype(np.int32)[None]
    want = er.dist2_ref(disc, 254)
    assert 0 < (want == 255 * 255).sum() < 100
    got = _check(ops, disc, 254, 116, True, "disc", want, cap=9)
    r2, pos, capped = er.decode_peak(got["peaks"][0, 8], W, 254)
    assert (r2, capped) == (255 * 255, True) and (pos[0] - 260) ** 2 + (pos[1] - 260) ** 2 <= 9
    _check(ops, np.full((1, 5, 7), 200, np.uint8), 254, 254, True, "tiny")


@pytest.mark.parametrize("conn", [4, 8])
def test_ids_of_seg_components(ops, tile, conn):
    """int32 id maps as ops.seg_components writes them, hundreds of distinct values, with their peaks."""
    R, Cc, P = tile
    H, W = 2 * R + 3, 2 * Cc + (5 if conn == 4 else 16)
    rs = np.random.RandomState(conn)
    c = rr.contents(H, W, rs)
    lab = torch.from_numpy(np.stack([c["noise 0.5"], c["checkerboard"], mr.blobs(H, W, rs)])).cuda()
    B = lab.shape[0]
    ids = torch.empty(B, H, W, dtype=torch.int32, device="cuda")
    n = torch.empty(B, 2, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.seg_components_workspace(B, H, W), dtype=torch.uint8, device="cuda")
    ops.seg_components(lab, ids, n, ws, connectivity=conn)
    m = ids.cpu().numpy()
    assert int(m.max()) > 255
    _check(ops, m, 7, 2, False, "ids", cap=int(m.max()))
    _check(ops, m, 7, 7, True, "ids, a short table", cap=100)


# ------------------------------------------------------------------------------------------------ peaks

def _peak_maps(H, W, R, Cc, rs):
    """int32 id maps [1, H, W] by name with the cap of their table: one per way the reduction can go wrong."""
    yy, xx = np.mgrid[:H, :W]
    out = {}
    out["one object over several tiles"] = (np.full((H, W), 3), 4)
    big = np.zeros((H, W), np.int64)
    big[2:H - 1, 3:W - 2] = 2
    out["an object over several tiles inside background"] = (big, 2)
    small = np.zeros((H, W), np.int64)
    small[R + 2:R + 5, Cc + 7:Cc + 10] = 1                                 # 3 x 3 inside one wave's lanes
    small[1, 1:4] = 2
    out["an object inside one wave"] = (small, 3)
    out["many one-pixel objects"] = (np.where((yy + xx) % 2 == 0, yy * W + xx + 1, 0), H * W)
    out["one-pixel objects side by side"] = (yy * W + xx + 1, H * W)
    out["columns of ids"] = (1 + xx, W)                                    # every lane another id, the rows fold
    out["pairs of columns"] = (1 + xx // 2, W)                             # runs that end inside a thread of four
    out["triples of columns"] = (1 + (xx + 1) // 3, W)                     # ... and that go on into the next one
    ign = np.array([0, 5, -1, 9, 2, -(1 << 31), 6, 1 << 30])[(yy // 3 + xx // 5) % 8]
    out["ids above the cap, zero and negative"] = (ign, 5)                 # 6, 9 and 2^30 are above it; row 3 and 4 stay 0
    tie = np.zeros((H, W), np.int64)
    tie[1:6, W - 6:W - 1] = 4                                              # two equal squares of one id in two workgroups:
    tie[R + 2:R + 7, 2:7] = 4                                              # the first in row-major order wins
    tie[2 * R - 1:2 * R + 2, 0:3] = 4
    out["a tie across two workgroups"] = (tie, 4)
    out["blobs as ids"] = (mr.blobs(H, W, rs, nlabels=7).astype(np.int64), 7)
    return {k: (v[None].astype(np.int32), cap) for k, (v, cap) in out.items()}


@pytest.mark.parametrize("vec", [True, False], ids=["four pixels a thread", "one pixel a thread"])
def test_peaks(ops, tile, vec):
    R, Cc, P = tile
    H, W = 2 * R + 3, (2 * Cc + 16 if vec else Cc + 3)
    rs = np.random.RandomState(W)
    for name, (m, cap) in _peak_maps(H, W, R, Cc, rs).items():
        for dmax in (5, 1):
            got = _check(ops, m, dmax, None, not vec, name, cap=cap, fill=0xFF)
        peaks = got["peaks"][0]
        if name.startswith("ids above"):
            assert peaks[0] == 0 and peaks[1] != 0 and peaks[2] == 0 and peaks[3] == 0 and peaks[4] != 0
        if name.startswith("a tie"):
            assert er.decode_peak(peaks[3], W, 1) == (4, (2, W - 5), True) and not peaks[:3].any()
        if name == "many one-pixel objects":
            assert ((peaks != 0) == ((np.arange(H * W) // W + np.arange(H * W) % W) % 2 == 0)).all()
    # two images: the second one's rows are its own
    both = np.concatenate([_peak_maps(H, W, R, Cc, rs)["blobs as ids"][0], _peak_maps(H, W, R, Cc, rs)["a tie across two workgroups"][0]])
    _check(ops, both, 5, 3, not vec, "two images", cap=7)


# ------------------------------------------------------------------------------------------------ counts

@pytest.mark.parametrize("shape", [(5, 7), (70, 61), (72, 60)], ids=["5x7", "two blocks, scalar", "two blocks, words"])
def test_counts_with_squared_maps(ops, shape):
    """uint16 squared maps against the reference's rule 1 <= dist2 <= d^2, and uint8 maps as before; poisoned, offset and
    repeated launches."""
    H, W = shape
    rs = np.random.RandomState(H * W)
    pred = np.stack([mr.blobs(H, W, rs, nlabels=5), mr.blobs(H, W, rs, nlabels=5)])
    gt = mr.perturb(pred, rs)
    gt[0, :2, :3], pred[1, -2:, -3:] = 200, 254
    dmax = 5
    p2, g2 = er.dist2_ref(pred, dmax), er.dist2_ref(gt, dmax)
    p1, g1 = br.dist_ref(pred, dmax), br.dist_ref(gt, dmax)
    differ = 0
    for nlabels in (1, 3, 254):
        for d in (1, 2, 4):
            want2 = br.counts_ref(pred, p2, gt, g2, d * d, nlabels)
            want1 = br.counts_ref(pred, p1, gt, g1, d, nlabels)
            differ += int(not np.array_equal(want1, want2))
            for off, fill, repeat in ((False, None, 1), (True, 0xFF, 2)):
                got = _counts(ops, pred, p2, gt, g2, d, nlabels, off, fill, repeat)
                assert np.array_equal(got, want2), (shape, nlabels, d, off)
            assert np.array_equal(tb._counts(ops, pred, p1, gt, g1, d, nlabels, True, 0xFF, 2), want1), (shape, nlabels, d)
    assert differ > 0 or shape == (5, 7)                                   # the two metrics are told apart
    with pytest.raises(ValueError):
        ops.seg_boundary_counts(*(torch.from_numpy(a).cuda() for a in (pred, p2, gt, g1)),
                                torch.empty(2, 2, 4, dtype=torch.int64, device="cuda"), 2)


def _counts(ops, pred, pdist, gt, gdist, d, nlabels, off=False, fill=None, repeat=1):
    pad = 3 if off else 64
    B = pred.shape[0]
    bufs = {k: tb._Guarded(pred.shape, torch.uint8, pad) for k in ("pred", "gt")}
    bufs.update({k: tb._Guarded(pred.shape, torch.uint16, 1 if off else 32) for k in ("pdist", "gdist")})
    bufs["counts"] = tb._Guarded((B, 2, nlabels + 1), torch.int64, 4, fill)
    src = dict(pred=pred, pdist=pdist, gt=gt, gdist=gdist)
    for k, v in src.items():
        bufs[k].t.copy_(torch.from_numpy(v))
    for _ in range(repeat):
        ops.seg_boundary_counts(*(bufs[k].t for k in ("pred", "pdist", "gt", "gdist", "counts")), d)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    for k, v in src.items():
        assert np.array_equal(bufs[k].t.cpu().numpy(), v), "an input was modified"
    return bufs["counts"].t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ launch behaviour

def _ids_case(tile, vec=True):
    R, Cc, P = tile
    H, W = 2 * R + 3, 2 * Cc + 16
    rs = np.random.RandomState(5)
    m = np.stack([mr.blobs(H, W, rs, nlabels=9), rr.contents(H, W, rs)["rings"]]).astype(np.int32)
    want = er.dist2_ref(m, 7)
    return m, want, er.band_ref(m, want, 4), er.peaks_ref(m, want, 9)


def test_poisoned_and_repeated_launches_give_the_same_bits(ops, tile):
    """Outputs and workspace pre-filled with two different bytes, two launches back to back into the same buffers, aligned
    and offset: the same bytes every time."""
    m, want, band, peaks = _ids_case(tile)
    for fill in (0x00, 0xFF, 0x5A):
        for off in (False, True):
            got = _launch(ops, m, 7, 4, off, fill, repeat=2, cap=9)
            assert np.array_equal(got["dist"], want) and np.array_equal(got["band"], band) and np.array_equal(got["peaks"], peaks)
    got = _launch(ops, m.astype(np.uint8), 7, 4, False, 0xFF, repeat=2)
    assert np.array_equal(got["dist"], want) and np.array_equal(got["band"], band.astype(np.uint8))


@pytest.mark.parametrize("off", [False, True], ids=["four pixels a thread", "one pixel a thread"])
def test_lds_poison(ops, tile, off):
    """Plain, then with every CU's LDS filled with 0xFF, 0x7B and 0x00 in front of the call: byte-equal, and equal to the
    reference.  The row pass reads its window, its bytes of h and the waves' scan ends from LDS."""
    from test_lds_poison_gpu import four_runs
    m, want, band, peaks = _ids_case(tile)

    def check(got):
        assert np.array_equal(got["dist"], want) and np.array_equal(got["band"], band) and np.array_equal(got["peaks"], peaks)
    four_runs("dfw_seg_boundary", lambda: _launch(ops, m, 7, 4, off, cap=9), check, ("seg_boundary euclidean", off))
    pred, gt = (m % 4).astype(np.uint8), mr.perturb((m % 4).astype(np.uint8), np.random.RandomState(6))
    p2, g2 = er.dist2_ref(pred, 5), er.dist2_ref(gt, 5)
    four_runs("dfw_seg_boundary_counts", lambda: _counts(ops, pred, p2, gt, g2, 3, 3, off),
              lambda got: np.testing.assert_array_equal(got, br.counts_ref(pred, p2, gt, g2, 9, 3)), ("seg_boundary_counts squared", off))


@pytest.mark.parametrize("with_peaks", [False, True], ids=["2 kernel nodes", "3 kernel nodes with peaks"])
def test_captured_graph_replayed_on_two_maps(ops, hip_lib, tile, with_peaks):
    from diffews_amd.objects import BoundaryBuffers
    R, Cc, P = tile
    B, H, W, dmax, d, cap = 2, 2 * R + 3, 2 * Cc + 16, 6, 3, 9
    rs = np.random.RandomState(31)
    maps = [np.stack([mr.blobs(H, W, rs, nlabels=9), mr.blobs(H, W, rs, nlabels=12)]).astype(np.int32),
            np.stack([rr.contents(H, W, rs)[k] for k in ("rings", "snake")]).astype(np.int32)]
    bb = BoundaryBuffers(B, H, W, dmax, torch.int32, metric="euclidean", max_components=cap if with_peaks else None)
    ids = torch.zeros(B, H, W, dtype=torch.int32, device="cuda")

    def call():
        ops.seg_boundary(ids, bb.dist, bb.ws, dmax, band=bb.band, d=d, metric="euclidean", peaks=bb.peaks)
    call()                                                                 # modules loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    nodes = C.c_int32()
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0     # no memset node
    assert nodes.value == (3 if with_peaks else 2)
    graph.instantiate()
    for m in maps + [maps[0]]:
        ids.copy_(torch.from_numpy(m))
        graph.replay()
        torch.cuda.synchronize()
        want = er.dist2_ref(m, dmax)
        assert np.array_equal(bb.dist.cpu().numpy(), want) and np.array_equal(bb.band.cpu().numpy(), er.band_ref(m, want, d))
        if with_peaks:
            assert np.array_equal(bb.peaks.cpu().numpy(), er.peaks_ref(m, want, cap))


# ------------------------------------------------------------------------------------------------ objects.py

def _thickness_checks(t, ids, cap, dmax):
    from diffews_amd.objects import thickness_to_host
    ids = ids.cpu().numpy()
    squeeze = ids.ndim == 2
    ids3 = ids[None] if squeeze else ids
    want = er.dist2_ref(ids3, dmax)
    peaks = er.peaks_ref(ids3, want, cap)
    assert t["dist2"].dtype == torch.uint16 and np.array_equal(t["dist2"].cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(t["peaks"].cpu().numpy().reshape(peaks.shape), peaks)
    assert t["dmax"] == dmax and t["shape"] == ids3.shape[1:]
    host = thickness_to_host(t)
    host = [host] if squeeze else host
    for b in range(ids3.shape[0]):
        k = min(int(ids3[b].max()), cap)
        assert host[b] == [er.decode_peak(key, ids3.shape[2], dmax) for key in peaks[b, :k]]
        for r2, pos, capped in host[b]:
            assert r2 >= 1 and ids3[b][pos] != 0 and want[b][pos] == r2    # the label point lies inside its object
    return host[0] if squeeze else host


def _bridge():
    """Two 9 x 9 squares of class 2 joined by a bridge two pixels thick, and a sliver of class 1."""
    lab = np.zeros((16, 40), np.uint8)
    lab[3:12, 2:11] = 2
    lab[3:12, 20:29] = 2
    lab[6:8, 11:20] = 2
    lab[14, 1:30] = 1
    return lab


def test_objects_layer(hip_lib):
    from diffews_amd.objects import (BoundaryBuffers, boundary_bands, boundary_counts, fill_holes, label_objects, object_boundaries,
                                     object_cores, object_thickness, objects_to_host, thickness_to_host)
    lab = torch.from_numpy(_bridge()).cuda()
    o = label_objects(lab, connectivity=8, max_components=8)
    objs, _ = objects_to_host(o)
    assert [(c, a) for c, a, _, _ in objs] == [(2, 81 + 81 + 18), (1, 29)]  # ONE object of class 2 ...
    t = object_thickness(o)
    host = _thickness_checks(t, o["ids"], 8, 254)
    assert host == [(25, (7, 6), False), (1, (14, 1), False)]              # the first square's centre; the sliver is 1 thick
    cores = object_cores(o, 1)
    cobjs, _ = objects_to_host(cores)
    assert [(c, a) for c, a, _, _ in cobjs] == [(2, 51), (2, 51)]          # ... and TWO cores (7 x 7 and the two pixels in front
    #                                                                      of the bridge); the bridge and the sliver are gone
    assert [(c, a) for c, a, _, _ in objects_to_host(object_cores(o, 0))[0]] == [(c, a) for c, a, _, _ in objs]
    assert objects_to_host(object_cores(o, 5, min_area=1))[0] == []
    # a batch and a list with buffers, dmax from the buffers; a fill_holes result
    rs = np.random.RandomState(41)
    maps = np.stack([mr.blobs(33, 47, rs), rr.contents(33, 47, rs)["rings"]])
    ob = label_objects(torch.from_numpy(maps).cuda(), max_components=64)
    bb = BoundaryBuffers(2, 33, 47, 9, torch.int32, metric="euclidean", max_components=64)
    for _ in range(2):
        tb_ = object_thickness(ob, buffers=bb)
        assert tb_["dist2"].data_ptr() == bb.dist.data_ptr() and tb_["peaks"].data_ptr() == bb.peaks.data_ptr()
        _thickness_checks(tb_, ob["ids"], 64, 9)
    filled = fill_holes(ob)
    _thickness_checks(object_thickness(filled, dmax=12), filled["ids"], 64, 12)
    items = [torch.from_numpy(mr.blobs(h, w, rs)).cuda() for h, w in ((40, 64), (21, 30))]
    ol = label_objects(items, max_components=32)
    tl = object_thickness(ol, dmax=6)
    assert isinstance(tl["peaks"], list) and tl["shape"] == [(40, 64), (21, 30)]
    hl = thickness_to_host(tl)
    for i in range(2):
        assert hl[i] == _thickness_checks({k: v[i] for k, v in tl.items()}, ol["ids"][i], 32, 6)
    cl = object_cores(ol, 2, max_components=32)
    for i in range(2):
        ids = ol["ids"][i].cpu().numpy()
        core = np.where(er.dist2_ref(ids, 2) > 4, items[i].cpu().numpy(), 0)
        assert np.array_equal(cl["labels"][i].cpu().numpy(), core)
    # the Euclidean bands of both maps, and their counts
    e = object_boundaries(ob, d=3, dmax=5, metric="euclidean")
    assert e["ids"]["metric"] == "euclidean" and set(e["labels"]) == {"dist2", "band", "d", "dmax", "metric"}
    for key, m in (("labels", ob["labels"].cpu().numpy()), ("ids", ob["ids"].cpu().numpy())):
        want = er.dist2_ref(m, 5)
        assert np.array_equal(e[key]["dist2"].cpu().numpy(), want) and np.array_equal(e[key]["band"].cpu().numpy(), er.band_ref(m, want, 3))
    c = object_boundaries(ob, d=3, dmax=5)
    assert set(c["labels"]) == {"dist", "band", "d", "dmax"} and c["labels"]["dist"].dtype == torch.uint8   # the default, as before
    gt = torch.from_numpy(mr.perturb(maps, rs)).cuda()
    eg = boundary_bands(gt, d=3, dmax=5, metric="euclidean")
    counts = boundary_counts(e["labels"], eg, ob["labels"], gt, 3, d=2)
    lm, gm = ob["labels"].cpu().numpy(), gt.cpu().numpy()
    assert np.array_equal(counts.cpu().numpy(), br.counts_ref(lm, er.dist2_ref(lm, 5), gm, er.dist2_ref(gm, 5), 4, 3))
    for bad in (lambda: boundary_counts(e["labels"], boundary_bands(gt, d=3, dmax=5), ob["labels"], gt, 3),
                lambda: boundary_bands(gt, d=3, buffers=BoundaryBuffers(2, 33, 47, 5)
                                       , metric="euclidean"),
                lambda: object_thickness(ob, buffers=BoundaryBuffers(2, 33, 47, 9, torch.int32, metric="euclidean", max_components=63)),
                lambda: object_thickness(ob, dmax=255), lambda: object_thickness(ob["ids"])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ the routes, tiny engine

def test_pipe_thickness_on_the_binary_native_route(pipe):  # noqa: F811
    from diffews_amd.input_pipeline import NativeTargets
    from test_support_bank_gpu import _queries, _support_set
    sup, msk = _support_set(2, 64, seed=930)
    bank = pipe.prepare_support(sup.cuda(), msk.cuda())
    sizes = [(50, 70), (33, 41)]
    r = pipe.segment_queries(bank, _queries(2, 64, 79).cuda(), native=NativeTargets((64, 64), sizes), captured=False)
    o = pipe.objects(r, key="pred", connectivity=8, max_components=256)
    for res in (o, pipe.fill_holes(o)):
        t = pipe.object_thickness(res, dmax=20)
        assert [tuple(d.shape) for d in t["dist2"]] == sizes
        for i in range(2):
            _thickness_checks({k: v[i] for k, v in t.items()}, res["ids"][i], 256, 20)
    cores = pipe.object_cores(o, 1, max_components=256)
    for i in range(2):
        ids = o["ids"][i].cpu().numpy()
        assert np.array_equal(cores["labels"][i].cpu().numpy(), np.where(er.dist2_ref(ids, 1) > 1, o["labels"][i].cpu().numpy(), 0))
    e = pipe.object_boundaries(o, metric="euclidean")
    for i in range(2):
        ids, d = o["ids"][i].cpu().numpy(), e["d"][i]
        assert np.array_equal(e["ids"]["band"][i].cpu().numpy(), er.band_ref(ids, er.dist2_ref(ids, d), d))
