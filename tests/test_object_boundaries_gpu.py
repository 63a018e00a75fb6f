"""GPU tests of the boundary stage: ops.seg_boundary and ops.seg_boundary_counts against tests/boundary_ref.py (the
published erosion procedure by array shifts, per value) at the smallest shapes that reach every path of the two kernels --
one pixel, one row, one column, 5 x 7, exactly a tile of the column pass, a tile plus a row, a tile plus a column, three
tiles each way with an odd width (one pixel a thread, more than two blocks of the row pass), a width that is a multiple of
16 (four pixels a thread) -- with the radii 1, 2, 7 and 254, uint8 and int32 maps, and one content per way the kernels can
go wrong; then the counts, batches, poisoned and repeated launches, a captured chain behind seg_components, the objects
layer, per-object Boundary IoU through match_objects, and the pipeline's two entry points.  All integers: every comparison
is exact.

Every buffer sits inside sentinel guards.  Half of the cases put an int32 map and band 61 WORDS into their allocation and
the byte maps (map, dist, band) 3 BYTES into theirs, which takes the one-pixel-a-thread path and the byte stores."""
import ctypes as C

import numpy as np
import pytest
import torch

import boundary_ref as br
import match_ref as mr
import rle_ref as rr

pytestmark = pytest.mark.gpu

SENT = 0xA5


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def tile(ops):
    return ops.seg_boundary_block()


class _Guarded:
    """A tensor inside a flat allocation with `pad` sentinel elements (0xA5 bytes) on either side; the tensor itself
    starts as sentinels too, or as `fill` bytes."""

    def __init__(self, shape, dtype, pad, fill=None):
        n = int(np.prod(shape))
        self.flat = torch.empty(n + 2 * pad, dtype=dtype, device="cuda")
        self.flat.view(torch.uint8).fill_(SENT)
        self.t = self.flat[pad:pad + n].view(shape)
        self.pad, self.n = pad, n
        if fill is not None:
            self.t.view(torch.uint8).fill_(fill)

    def check(self, name):
        f = self.flat.view(torch.uint8)
        e = self.flat.element_size()
        assert (f[:self.pad * e] == SENT).all() and (f[(self.pad + self.n) * e:] == SENT).all(), f"wrote outside {name}"


def _launch(ops, m, dmax, d=None, off=False, fill=None, repeat=1):
    """ops.seg_boundary on a numpy map [B, H, W] in guarded buffers; returns (dist, band or None) as numpy after checking
    every guard and that the map did not change."""
    B, H, W = m.shape
    dt = torch.uint8 if m.dtype == np.uint8 else torch.int32
    mpad = (3 if off else 64) if dt == torch.uint8 else (61 if off else 4)
    bufs = dict(map=_Guarded(m.shape, dt, mpad), dist=_Guarded(m.shape, torch.uint8, 3 if off else 64, fill),
                ws=_Guarded((ops.seg_boundary_workspace(B, H, W, m.dtype.itemsize),), torch.uint8, 64, fill))
    if d is not None:
        bufs["band"] = _Guarded(m.shape, dt, mpad, fill)
    bufs["map"].t.copy_(torch.from_numpy(m))
    for _ in range(repeat):
        ops.seg_boundary(bufs["map"].t, bufs["dist"].t, bufs["ws"].t, dmax, band=bufs["band"].t if d is not None else None, d=d)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert np.array_equal(bufs["map"].t.cpu().numpy(), m), "the map was modified"
    return bufs["dist"].t.cpu().numpy(), (bufs["band"].t.cpu().numpy() if d is not None else None)


def _check(ops, m, dmax, d, off, what, want=None):
    want = br.dist_ref(m, dmax) if want is None else want
    dist, band = _launch(ops, m, dmax, d, off)
    assert dist.dtype == np.uint8 and np.array_equal(dist, want), (what, m.shape, str(m.dtype), dmax, off, int((dist != want).sum()))
    assert np.array_equal(dist == 0, m == 0) and int(dist.max()) <= dmax + 1
    assert band.dtype == m.dtype and np.array_equal(band, br.band_ref(m, want, d)), (what, m.shape, str(m.dtype), dmax, d, off)
    return dist


def _contents(H, W, R, Cc, rs):
    """int64 maps [B, H, W] by name, values that fit a byte unless the name says otherwise: one per way to go wrong."""
    yy, xx = np.mgrid[:H, :W]
    sx, sy = (Cc if W > Cc else W // 2), (R if H > R else H // 2)
    ends = np.zeros((H, W), np.int64)
    ends[0::2, W - 1] = 5                                                  # a row that ends in 5 ...
    ends[1::2, 0] = 5                                                      # ... and the next one starts with it
    ring = np.full((H, W), 3, np.int64)
    ring[H // 4:H - H // 4, W // 4:W - W // 4] = 9
    ring[H // 4 + 1:H - H // 4 - 1, W // 4 + 1:W - W // 4 - 1] = 3
    three = np.array([1, 257, 513])[(xx // 2 + yy // 3) % 3]
    out = {"empty": np.zeros((H, W), np.int64), "one value": np.full((H, W), 7, np.int64),
           "checkerboard": 1 + (yy + xx) % 2, "checkerboard on background": ((yy + xx) % 2) * 4,
           "vertical stripes": 1 + xx % 2, "horizontal stripes": 1 + yy % 2,
           "seam on the tile border, x": 1 + (xx >= sx), "seam one off, x": 1 + (xx >= sx + 1),
           "seam on the tile border, y": 1 + (yy >= sy), "seam one off, y": 1 + (yy >= sy - 1),
           "line ends": ends, "ring": ring, "254 and 255": np.where((yy // 3 + xx // 5) % 2 == 0, 254, 255),
           "255 and background": np.where((yy // 4 + xx // 3) % 3 == 0, 0, 255),
           "int32: 1, 257, 513": three, "int32: negative": np.where((yy // 3 + xx // 4) % 2 == 0, -5, -700),
           "int32: negative and background": np.where((yy // 2 + xx // 5) % 3 == 0, 0, -(1 << 31))}
    for k, v in rr.contents(H, W, rs).items():
        out["rle " + k] = v.astype(np.int64)
    out["blobs"] = mr.blobs(H, W, rs).astype(np.int64)
    both = np.stack([out["one value"], out["one value"]])                 # the last row of image 0 = the first of image 1
    both[1, H // 2:, :] = 2
    stack = {k: v[None] for k, v in out.items()}
    stack["batch of one value"] = both
    stack["batch of blobs"] = np.stack([mr.blobs(H, W, rs), mr.blobs(H, W, rs), out["rle rings"]]).astype(np.int64)
    return stack


def _shapes(tile):
    R, Cc, P = tile
    assert Cc % 16 == 0 and (2 * R + 3) * (2 * Cc + 5) > 2 * P
    return [(1, 1), (1, 37), (37, 1), (5, 7), (R, Cc), (R + 1, Cc), (R, Cc + 1), (2 * R + 3, 2 * Cc + 5), (2 * R + 3, 2 * Cc + 16)]


@pytest.mark.parametrize("which", range(9), ids=["1x1", "1x37", "37x1", "5x7", "tile", "tile+row", "tile+column",
                                                 "3-tiles-odd-W", "W%16==0"])
def test_equals_the_reference(ops, tile, which):
    """Every content, uint8 and int32, dmax 1 / 2 / 7 with a band of d <= dmax from the same launch."""
    R, Cc, P = tile
    H, W = _shapes(tile)[which]
    if which == 7:
        assert W % 2 == 1 and 2 * R < H <= 3 * R and 2 * Cc < W <= 3 * Cc
    if which == 8:
        assert W % 16 == 0 and H * W > 2 * P
    rs = np.random.RandomState(1000 * H + W)
    case = 0
    for name, m64 in _contents(H, W, R, Cc, rs).items():
        for dtype in (np.uint8, np.int32):
            if dtype == np.uint8 and name.startswith("int32"):
                continue
            m = m64.astype(dtype)
            assert np.array_equal(m.astype(np.int64), m64)
            for dmax, d in ((1, 1), (2, 1), (7, 7), (7, 3)):
                dist = _check(ops, m, dmax, d, case % 2 == 1, name)
                case += 1
                if name == "empty":
                    assert not dist.any()
                if name.startswith("checkerboard") or "stripes" in name and name[0] != "r":
                    assert int(dist.max()) == int(m.any())
                if name == "one value":                                    # the image border alone
                    yy, xx = np.mgrid[:H, :W]
                    edge = np.minimum(np.minimum(yy + 1, H - yy), np.minimum(xx + 1, W - xx))
                    assert np.array_equal(dist[0], np.minimum(edge, dmax + 1))
                if name == "batch of one value":                           # nothing bleeds from image 0 into image 1
                    assert (dist[0, -1] == 1).all() and (dist[1, 0] == 1).all()


def test_radius_254(ops, tile):
    """dmax = 254: on a map smaller than the radius both ways (600 x 130, the walk of 254 rows crosses many tiles), on a
    tiny map, and on one value over 520 x 516, where the centre is deeper than 254 and the cap is reached."""
    R, Cc, P = tile
    rs = np.random.RandomState(254)
    H, W = 600, 130
    yy, xx = np.mgrid[:H, :W]
    halves = (1 + (yy >= 19 * R)).astype(np.int64)
    blobs = mr.blobs(H, W, rs, count=12, radius=40).astype(np.int64)
    for i, m64 in enumerate((np.full((H, W), 3, np.int64), halves, blobs)):
        for dtype in (np.uint8, np.int32):
            dist = _check(ops, m64.astype(dtype)[None], 254, 100, i % 2 == 1, i)
    assert int(dist.max()) > 20
    _check(ops, np.full((1, 5, 7), 200, np.uint8), 254, 254, True, "tiny")
    H, W = 520, 516
    yy, xx = np.mgrid[:H, :W]
    edge = np.minimum(np.minimum(yy + 1, H - yy), np.minimum(xx + 1, W - xx))
    want = np.minimum(edge, 255).astype(np.uint8)[None]
    assert (want == 255).sum() > 0 and (edge > 255).any()
    for dtype, off in ((np.uint8, False), (np.int32, True)):
        _check(ops, np.full((1, H, W), 77, dtype), 254, 116, off, "deep", want)


@pytest.mark.parametrize("conn", [4, 8])
def test_ids_of_seg_components(ops, tile, conn):
    """int32 id maps as ops.seg_components writes them, hundreds of distinct values."""
    R, Cc, P = tile
    H, W = 2 * R + 3, 2 * Cc + 5
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
    _check(ops, m, 7, 2, conn == 8, "ids")


# ------------------------------------------------------------------------------------------------ counts

def _counts(ops, pred, pdist, gt, gdist, d, nlabels, off=False, fill=None, repeat=1):
    pad = 3 if off else 64
    B = pred.shape[0]
    bufs = {k: _Guarded(pred.shape, torch.uint8, pad) for k in ("pred", "pdist", "gt", "gdist")}
    bufs["counts"] = _Guarded((B, 2, nlabels + 1), torch.int64, 4, fill)
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


@pytest.mark.parametrize("shape", [(5, 7), (70, 61), (72, 60)], ids=["5x7", "two blocks, scalar", "two blocks, words"])
def test_counts_equal_the_reference(ops, shape):
    """gt bytes 255 and nlabels < gt < 255, predicted bytes above nlabels, nlabels 1 / 3 / 254, B = 2, two widths from one
    pair of dist maps, poisoned and repeated launches."""
    H, W = shape
    rs = np.random.RandomState(H * W)
    pred = np.stack([mr.blobs(H, W, rs, nlabels=5), mr.blobs(H, W, rs, nlabels=5)])
    gt = mr.perturb(pred, rs)
    gt[0, :2, :3], pred[1, -2:, -3:] = 200, 254
    assert (gt == 255).any() and ((gt > 3) & (gt < 255)).any() and (pred > 3).any()
    dmax = 5
    pdist, gdist = br.dist_ref(pred, dmax), br.dist_ref(gt, dmax)
    for nlabels in (1, 3, 254):
        for d in (1, 4):
            want = br.counts_ref(pred, pdist, gt, gdist, d, nlabels)
            assert want[:, 0, 1:].sum() > 0 or nlabels == 1
            for off, fill, repeat in ((False, None, 1), (True, 0xFF, 3)):
                got = _counts(ops, pred, pdist, gt, gdist, d, nlabels, off, fill, repeat)
                assert np.array_equal(got, want), (shape, nlabels, d, off)
    from diffews_amd import metrics
    iou, miou = metrics.boundary_iou(torch.from_numpy(want))
    tot = want.sum(0)
    assert iou[1].item() == 100.0 * tot[0, 1] / tot[1, 1] and 0.0 < miou <= 100.0


# ------------------------------------------------------------------------------------------------ launch behaviour

def test_poisoned_and_repeated_launches_give_the_same_bits(ops, tile):
    R, Cc, P = tile
    H, W = 2 * R + 3, 2 * Cc + 16
    rs = np.random.RandomState(5)
    m = np.stack([mr.blobs(H, W, rs), rr.contents(H, W, rs)["rings"]])
    want = br.dist_ref(m, 7)
    for dtype in (np.uint8, np.int32):
        for fill in (0x00, 0xFF, 0x5A):
            for off in (False, True):
                dist, band = _launch(ops, m.astype(dtype), 7, 4, off, fill, repeat=3)
                assert np.array_equal(dist, want) and np.array_equal(band, br.band_ref(m.astype(dtype), want, 4))


def test_captured_chain_follows_the_labels(ops, hip_lib):
    """seg_components -> seg_boundary (ids and labels) -> seg_boundary_counts in one torch.cuda.graph: no memset node, 8 + 2
    + 2 + 2 kernel nodes, and each replay describes whatever the label tensor holds."""
    from diffews_amd.objects import BoundaryBuffers, ComponentBuffers
    rs = np.random.RandomState(31)
    B, H, W, cap, dmax, d, N = 2, 41, 72, 600, 6, 3, 3
    maps = [np.stack([mr.blobs(H, W, rs), mr.blobs(H, W, rs)]), np.stack([rr.contents(H, W, rs)[k] for k in ("rings", "snake")]),
            np.zeros((B, H, W), np.uint8)]
    gt = mr.perturb(maps[0], rs)
    gdist = br.dist_ref(gt, dmax)
    buf = ComponentBuffers(B, H, W, cap)
    bi, bl = BoundaryBuffers(B, H, W, dmax, torch.int32), BoundaryBuffers(B, H, W, dmax, torch.uint8)
    lab = torch.zeros(B, H, W, dtype=torch.uint8, device="cuda")
    tgt, tgd = torch.from_numpy(gt).cuda(), torch.from_numpy(gdist).cuda()
    counts = torch.empty(B, 2, N + 1, dtype=torch.int64, device="cuda")

    def call():
        ops.seg_components(lab, buf.ids, buf.n, buf.ws, stats=buf.stats, connectivity=8)
        ops.seg_boundary(buf.ids, bi.dist, bi.ws, dmax, band=bi.band, d=d)
        ops.seg_boundary(lab, bl.dist, bl.ws, dmax, band=bl.band, d=d)
        ops.seg_boundary_counts(lab, bl.dist, tgt, tgd, counts, d)
    call()                                                                 # modules loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    nodes = C.c_int32()
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0
    assert nodes.value == 8 + 2 + 2 + 2
    graph.instantiate()
    for m in maps + [maps[0]]:
        lab.copy_(torch.from_numpy(m))
        graph.replay()
        torch.cuda.synchronize()
        ids = buf.ids.cpu().numpy()
        want_i, want_l = br.dist_ref(ids, dmax), br.dist_ref(m, dmax)
        assert np.array_equal(bi.dist.cpu().numpy(), want_i) and np.array_equal(bi.band.cpu().numpy(), br.band_ref(ids, want_i, d))
        assert np.array_equal(bl.dist.cpu().numpy(), want_l) and np.array_equal(bl.band.cpu().numpy(), br.band_ref(m, want_l, d))
        assert np.array_equal(counts.cpu().numpy(), br.counts_ref(m, want_l, gt, gdist, d, N))


# ------------------------------------------------------------------------------------------------ objects.py

def test_objects_layer(hip_lib):
    """boundary_bands, object_boundaries and boundary_counts on [H, W], [B, H, W] and a ragged list whose items get their
    own d; BoundaryBuffers reused and aliased; the ValueErrors."""
    from diffews_amd import metrics
    from diffews_amd.objects import BoundaryBuffers, boundary_bands, boundary_counts, label_objects, object_boundaries
    rs = np.random.RandomState(41)
    sizes = [(120, 90), (40, 64)]
    assert [metrics.boundary_width(h, w) for h, w in sizes] == [3, 2] == [br.width(h, w) for h, w in sizes]
    maps = [mr.blobs(h, w, rs) for h, w in sizes]
    gts = [mr.perturb(m, rs) for m in maps]
    dev, gdev = [torch.from_numpy(m).cuda() for m in maps], [torch.from_numpy(g).cuda() for g in gts]
    bp, bg = boundary_bands(dev), boundary_bands(gdev)
    assert bp["d"] == [3, 2] and bp["dmax"] == [3, 2] and all(isinstance(bp[k], list) for k in ("dist", "band"))
    cs = boundary_counts(bp, bg, dev, gdev, 3)
    for i, (m, g) in enumerate(zip(maps, gts)):
        d = bp["d"][i]
        wp, wg = br.dist_ref(m, d), br.dist_ref(g, d)
        assert np.array_equal(bp["dist"][i].cpu().numpy(), wp) and np.array_equal(bp["band"][i].cpu().numpy(), br.band_ref(m, wp, d))
        assert np.array_equal(bg["dist"][i].cpu().numpy(), wg)
        assert cs[i].shape == (2, 4) and np.array_equal(cs[i].cpu().numpy(), br.counts_ref(m[None], wp[None], g[None], wg[None], d, 3)[0])
    iou, miou = metrics.boundary_iou(cs)
    assert iou.shape == (4,) and 0.0 < miou < 100.0
    # a list result of label_objects: labels and ids, one d per item
    o = label_objects(dev, connectivity=8, max_components=512)
    ob = object_boundaries(o)
    assert ob["d"] == [3, 2]
    for i in range(2):
        ids = o["ids"][i].cpu().numpy()
        wi = br.dist_ref(ids, ob["d"][i])
        assert ob["ids"]["band"][i].dtype == torch.int32 and np.array_equal(ob["ids"]["band"][i].cpu().numpy(), br.band_ref(ids, wi, ob["d"][i]))
        assert np.array_equal(ob["labels"]["dist"][i].cpu().numpy(), br.dist_ref(maps[i], ob["d"][i]))
    # a batch with buffers, reused and aliased; a wider search radius than the band; another width from the same dist
    lab = torch.from_numpy(np.stack([mr.blobs(33, 47, rs), mr.blobs(33, 47, rs)])).cuda()
    gt = torch.from_numpy(mr.perturb(lab.cpu().numpy(), rs)).cuda()
    bb = BoundaryBuffers(2, 33, 47, 6)
    want = br.dist_ref(lab.cpu().numpy(), 6)
    for _ in range(2):
        r = boundary_bands(lab, d=2, buffers=bb)
        assert r["dist"].data_ptr() == bb.dist.data_ptr() and r["band"].data_ptr() == bb.band.data_ptr() and (r["d"], r["dmax"]) == (2, 6)
        assert np.array_equal(r["dist"].cpu().numpy(), want)
    g = boundary_bands(gt, d=2, dmax=6)
    wg = br.dist_ref(gt.cpu().numpy(), 6)
    counts = torch.empty(2, 2, 4, dtype=torch.int64, device="cuda")
    for d in (2, 5, None):
        c = boundary_counts(r, g, lab, gt, 3, d=d, counts=counts)
        assert c.data_ptr() == counts.data_ptr()
        assert np.array_equal(c.cpu().numpy(), br.counts_ref(lab.cpu().numpy(), want, gt.cpu().numpy(), wg, d or 2, 3))
    one = boundary_bands(lab[1])
    assert one["dist"].shape == (33, 47) and one["d"] == metrics.boundary_width(33, 47) == 1
    assert np.array_equal(one["dist"].cpu().numpy(), br.dist_ref(lab[1].cpu().numpy(), 1))
    for bad in (lambda: boundary_bands(lab, d=255), lambda: boundary_bands(lab, d=3, dmax=2), lambda: boundary_bands(lab, d=0),
                lambda: boundary_bands(lab.float()), lambda: boundary_bands(lab.cpu()), lambda: boundary_bands(lab, buffers=BoundaryBuffers(2, 33, 48, 6)),
                lambda: boundary_bands(lab.int(), d=2, buffers=bb), lambda: boundary_bands([lab[0], lab[1]], d=[1]),
                lambda: boundary_counts(r, g, lab, gt, 3, d=7), lambda: boundary_counts(r, g, lab, gt.int(), 3),
                lambda: boundary_counts(r, g, lab, gt, 255), lambda: boundary_counts(r, g, lab, gt[:, :, :40], 3),
                lambda: BoundaryBuffers(2, 33, 47, 255), lambda: BoundaryBuffers(2, 33, 47, 6, torch.int64)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="254"):
        boundary_bands(torch.zeros(1, 1, dtype=torch.uint8, device="cuda"), d=255)


def test_per_object_boundary_iou_through_match_objects(hip_lib):
    """match_objects on the bands of the ids: pairs, areas and pq are those of the reference's band id maps, and the pq
    table is the one computed from the shared band pixels in Python integers."""
    from diffews_amd.objects import label_objects, match_objects, object_boundaries
    rs = np.random.RandomState(43)
    B, H, W, N, cap, d = 2, 64, 80, 3, 256, 2
    pred = np.stack([mr.blobs(H, W, rs, count=10, radius=9) for _ in range(B)])
    gt = mr.perturb(pred, rs)
    tp, tg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    skip = tg.clone()
    glab = torch.where(tg == 255, torch.zeros_like(tg), tg)
    op, og = label_objects(tp, max_components=cap), label_objects(glab, max_components=cap)
    pb, gb = object_boundaries(op, d=d), object_boundaries(og, d=d)
    m = match_objects((pb["ids"]["band"], op["stats"]), (gb["ids"]["band"], og["stats"]), skip=skip, nlabels=N)
    pid, gid = op["ids"].cpu().numpy(), og["ids"].cpu().numpy()
    pband, gband = br.band_ref(pid, br.dist_ref(pid, d), d), br.band_ref(gid, br.dist_ref(gid, d), d)
    assert np.array_equal(pb["ids"]["band"].cpu().numpy(), pband) and np.array_equal(gb["ids"]["band"].cpu().numpy(), gband)
    pst, gst = op["stats"].cpu().numpy(), og["stats"].cpu().numpy()
    n = m["n"].cpu().numpy()
    assert (n[:, 0] == n[:, 1]).all() and (n[:, 2] == n[:, 3]).all()
    pairs, area, pq = m["pairs"].cpu().numpy(), m["area"].cpu().numpy(), m["pq"].cpu().numpy()
    for b in range(B):
        shared = mr.pixel_pairs(pband[b].tolist(), gband[b].tolist(), cap, cap, gt[b].tolist())
        got = {(p, g): i for p, g, i in pairs[b, :n[b, 0]].tolist()}
        assert got == shared and len(shared) > 4
        keep = gt[b] != 255
        for k in range(1, cap + 1):
            assert area[b, k] == int(((pband[b] == k) & keep).sum()) and area[b, cap + 1 + k] == int(((gband[b] == k) & keep).sum())
        table = [[0, 0, 0, 0] for _ in range(N + 1)]
        hit_p, hit_g = set(), set()
        for (p, g), i in shared.items():
            if p and g and pst[b, p - 1, 0] == gst[b, g - 1, 0] and 1 <= pst[b, p - 1, 0] <= N:
                union = int(area[b, p]) + int(area[b, cap + 1 + g]) - i
                if 2 * i > union:
                    table[pst[b, p - 1, 0]][0] += 1
                    table[pst[b, p - 1, 0]][3] += (i << 32) // union
                    hit_p.add(p), hit_g.add(g)
        for k in range(1, cap + 1):
            if area[b, k] and k not in hit_p and 1 <= pst[b, k - 1, 0] <= N:
                table[pst[b, k - 1, 0]][1] += 1
            if area[b, cap + 1 + k] and k not in hit_g and 1 <= gst[b, k - 1, 0] <= N:
                table[gst[b, k - 1, 0]][2] += 1
        assert pq[b].tolist() == table and sum(r[0] + r[1] for r in table) > 0


# ------------------------------------------------------------------------------------------------ the routes, tiny engine

@pytest.fixture(scope="module")
def pipe(hip_lib):
    """The tiny-config engine of tests/test_support_bank_gpu.py (bf16), without its oracle."""
    from diffews_amd import config, weights
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise
    from diffews_amd.scheduler import DDIMSchedulerCustomized
    from diffews_amd.unet import MyUNet2DConditionModel
    from diffews_amd.vae import AutoencoderKL
    dt = torch.bfloat16
    kw = lambda cfg: {k: v for k, v in cfg.items() if not k.startswith("_")}  # noqa: E731
    ucfg, vcfg = config.get("tiny_unet"), config.get("tiny_vae")
    unet = MyUNet2DConditionModel(ucfg, weights.synthetic_unet_state_dict(ucfg, round_to=dt), torch_dtype=dt)
    vae = AutoencoderKL(vcfg, weights.synthetic_vae_state_dict(vcfg, round_to=dt), torch_dtype=dt)
    te = weights.synthetic_text_embed(ucfg).to(dt).float()
    return MarigoldPipelineRGBLatentNoise(unet, vae, DDIMSchedulerCustomized(**kw(config.get("scheduler"))), text_embeds=te)


def _pipe_checks(pipe, r, key, maps, N, seed):
    """pipe.boundary_counts and pipe.object_boundaries on the route's own map(s) against the reference, the ground truth a
    perturbed copy of the map."""
    rs = np.random.RandomState(seed)
    many = isinstance(maps, list)
    host = [m.cpu().numpy() for m in maps] if many else maps.cpu().numpy()
    gts = [mr.perturb(h, rs) for h in host] if many else mr.perturb(host, rs)
    gdev = [torch.from_numpy(g).cuda() for g in gts] if many else torch.from_numpy(gts).cuda()
    counts = pipe.boundary_counts(r, gdev, N, key=key)
    o = pipe.objects(r, key=key, connectivity=8, max_components=1024)
    ob = pipe.object_boundaries(o)
    items = list(zip(host, gts, counts, ob["d"], ob["ids"]["band"], o["ids"])) if many else \
        [(host, gts, counts, ob["d"], ob["ids"]["band"], o["ids"])]
    for h, g, c, d, band, ids in items:
        assert d == br.width(*h.shape[-2:])
        h3, g3 = h.reshape(-1, *h.shape[-2:]), g.reshape(-1, *g.shape[-2:])
        want = br.counts_ref(h3, br.dist_ref(h3, d), g3, br.dist_ref(g3, d), d, N)
        assert np.array_equal(c.cpu().numpy().reshape(want.shape), want)
        ids = ids.cpu().numpy()
        assert np.array_equal(band.cpu().numpy(), br.band_ref(ids, br.dist_ref(ids, d), d))
    with pytest.raises(KeyError):
        pipe.boundary_counts(r, gdev, N, key="nothing")


def test_pipe_boundaries_on_the_n_way_route(pipe):
    from test_support_bank_gpu import _queries, _support_set
    sets = [_support_set(s, 64, seed=910 + 10 * c) for c, s in enumerate((1, 3, 2))]
    library = pipe.prepare_support_classes([a.cuda() for a, _ in sets], [m.cuda() for _, m in sets])
    r = pipe.segment_classes(library, _queries(2, 64, 77).cuda(), captured=False)
    assert r["labels"].shape == (2, 64, 64)
    _pipe_checks(pipe, r, "labels", r["labels"], 3, 61)


def test_pipe_boundaries_on_the_binary_native_route(pipe):
    from diffews_amd.input_pipeline import NativeTargets
    from test_support_bank_gpu import _queries, _support_set
    sup, msk = _support_set(2, 64, seed=930)
    bank = pipe.prepare_support(sup.cuda(), msk.cuda())
    sizes = [(50, 70), (33, 41)]
    r = pipe.segment_queries(bank, _queries(2, 64, 79).cuda(), native=NativeTargets((64, 64), sizes), captured=False)
    maps = r["native"]["pred"]
    assert [tuple(m.shape) for m in maps] == sizes
    _pipe_checks(pipe, r, "pred", maps, 1, 62)
