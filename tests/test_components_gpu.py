"""GPU tests of the connected-components stage: ops.seg_components against the flood fill of tests/components_ref.py on ids,
filtered labels, n, stats and counts, at the smallest shapes that reach every path of the kernels -- one pixel, one row,
one column, exactly a tile, a tile plus one, three tiles per axis with an odd width (the scalar path), a width that is a
multiple of four (the word path) -- on contents that stress the union-find (one object everywhere, a checkerboard, a snake
through every tile, rings, noise); then batches, the stats cap, a no-op filter behind ops.seg_labels, guards, poisoned and
repeated launches, a captured launch, and objects.label_objects / pipe.objects / objects_to_host on top.  All integers:
every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_ref as cr

pytestmark = pytest.mark.gpu

SENT = 0xA5
NLAB = 3          # classes of the ground truth; the contents use 1..3 and one byte (7) above it, which has no bin


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def tile(hip_lib):
    th, tw = C.c_int32(), C.c_int32()
    assert hip_lib.dfw_seg_components_tile(C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


# ------------------------------------------------------------------------------------------------ contents

def _checker(H, W):
    yy, xx = np.mgrid[:H, :W]
    return (((yy + xx) % 2) * 2).astype(np.uint8)


def _snake(H, W):
    """One pixel wide, boustrophedon: every even row, joined to the next at alternating ends."""
    lab = np.zeros((H, W), np.uint8)
    lab[::2] = 1
    for y in range(1, H, 2):
        lab[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return lab


def _rings(H, W):
    yy, xx = np.mgrid[:H, :W]
    d = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
    return (1 + d % 2).astype(np.uint8)


def _noise(H, W, density, rs):
    return ((rs.rand(H, W) < density) * rs.randint(1, NLAB + 1, (H, W))).astype(np.uint8)


def _contents(H, W, rs):
    return {"background": np.zeros((H, W), np.uint8), "one class": np.full((H, W), 7, np.uint8), "checkerboard": _checker(H, W),
            "snake": _snake(H, W), "rings": _rings(H, W), "noise 0.3": _noise(H, W, 0.3, rs),
            "noise 0.5": _noise(H, W, 0.5, rs), "noise 0.65": _noise(H, W, 0.65, rs)}


def _gt(shape, rs):
    """0..NLAB, some 255 (ignore) and some ids above NLAB that have no bin."""
    g = rs.randint(0, NLAB + 1, shape).astype(np.uint8)
    g[rs.rand(*shape) < 0.05] = 255
    g[rs.rand(*shape) < 0.05] = NLAB + 2
    return g


# ------------------------------------------------------------------------------------------------ guarded launches

class _Guarded:
    """A tensor inside a flat allocation with `pad` sentinel elements (0xA5 bytes / -7 words) on either side."""

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


def _launch(ops, labels, conn, min_area, cap, gt=None, pad=64, fill=None, want=("filtered", "stats"), bufs=None, repeat=1):
    """ops.seg_components on `labels` (numpy uint8 [B, H, W]) into guarded buffers, optionally pre-filled with a byte;
    returns numpy results after checking every guard.  pad = 61 puts the byte buffers off word alignment."""
    B, H, W = labels.shape
    if bufs is None:
        lab = _Guarded((B, H, W), torch.uint8, pad)
        bufs = dict(labels=lab, ids=_Guarded((B, H, W), torch.int32, 4, fill), n=_Guarded((B, 2), torch.int32, 4, fill),
                    ws=_Guarded((ops.seg_components_workspace(B, H, W),), torch.uint8, 64, fill),
                    filtered=_Guarded((B, H, W), torch.uint8, pad, fill) if "filtered" in want else None,
                    stats=_Guarded((B, cap, 8), torch.int32, 4, fill) if "stats" in want else None,
                    gt=_Guarded((B, H, W), torch.uint8, pad) if gt is not None else None,
                    counts=_Guarded((B, 2, NLAB + 1), torch.int64, 2, fill) if gt is not None else None)
    bufs["labels"].t.copy_(torch.from_numpy(labels))
    if gt is not None:
        bufs["gt"].t.copy_(torch.from_numpy(gt))
    g = {k: (None if v is None else v.t) for k, v in bufs.items()}
    for _ in range(repeat):
        ops.seg_components(g["labels"], g["ids"], g["n"], g["ws"], filtered=g["filtered"], stats=g["stats"], gt=g["gt"],
                           counts=g["counts"], connectivity=conn, min_area=min_area, nlabels=NLAB if gt is not None else None)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        if v is not None:
            v.check(k)
    assert np.array_equal(g["labels"].cpu().numpy(), labels), "the input was modified"
    return {k: (None if g[k] is None else g[k].cpu().numpy()) for k in ("ids", "n", "filtered", "stats", "counts")}, bufs


def _same(got, want, what):
    for k in ("ids", "n", "filtered", "stats", "counts"):
        if got[k] is None:
            continue
        w = want["filtered" if k == "filtered" else k]
        assert np.array_equal(got[k], w), (what, k, int((got[k] != w).sum()))


def _shapes(tile):
    th, tw = tile
    w4 = 2 * tw + 4
    assert w4 % 4 == 0 and (3 * tw + 5) % 2 == 1
    return [(1, 1), (1, 37), (37, 1), (5, 7), (th, tw), (th + 1, tw + 1), (2 * th + 3, 3 * tw + 5), (th + 5, w4)]


@pytest.mark.parametrize("which", range(8), ids=["1x1", "1x37", "37x1", "5x7", "tile", "tile+1", "3-tiles-odd-W", "W%4==0"])
def test_equals_the_flood_fill(ops, tile, which):
    """Every content, both connectivities, min_area 0 / 1 / 2 / 5 / above every area, with a ground truth that holds 255
    and ids above nlabels; cap = 16 so that the checkerboard (HW / 2 objects with 4 neighbours) runs into the truncation."""
    H, W = _shapes(tile)[which]
    rs = np.random.RandomState(1000 * H + W)
    cap = 16
    gt = _gt((1, H, W), rs)
    for name, lab in _contents(H, W, rs).items():
        for conn in (4, 8):
            comps = [cr.flood(lab, conn)]
            for min_area in (0, 1, 2, 5, H * W + 1):
                want = cr.components(lab[None], conn, min_area, cap, gt, NLAB, comps=comps)
                pad = 61 if min_area == 2 else 64
                got, _ = _launch(ops, lab[None], conn, min_area, cap, gt, pad=pad)
                _same(got, want, (name, H, W, conn, min_area))
            if name == "checkerboard" and H * W > 1:
                n4 = cr.assemble(lab, comps[0], 0, cap)[2]
                assert n4 == ((H * W // 2,) * 2 if conn == 4 else (1, 1) if min(H, W) > 1 else (H * W // 2,) * 2)
            if name == "snake":
                assert len(comps[0]) == 1                          # the long chain is one object whatever the neighbours
    if which == 6:
        th, tw = tile
        assert H > 2 * th and W > 2 * tw                           # the snake crosses at least three tiles per axis


def test_clusters_that_wind_through_many_tiles(ops, tile):
    """One class at the site-percolation density of each neighbourhood (0.593 with 4 neighbours, 0.407 with 8) on 10 x 8
    tiles, and the snake at that size: components that cross many tile borders many times, so the border unions of many
    workgroups meet on the same roots."""
    th, tw = tile
    H, W = 9 * th + 5, 7 * tw + 3
    rs = np.random.RandomState(43)
    gt = _gt((1, H, W), rs)
    for conn, density in ((4, 0.6), (8, 0.41)):
        for lab in ((rs.rand(H, W) < density).astype(np.uint8), _snake(H, W)):
            comps = [cr.flood(lab, conn)]
            assert max(len(c[1]) for c in comps[0]) > 8 * th * tw          # something spans many tiles
            for min_area in (0, 50):
                got, _ = _launch(ops, lab[None], conn, min_area, 64, gt)
                _same(got, cr.components(lab[None], conn, min_area, 64, gt, NLAB, comps=comps), (conn, density, min_area))


def test_optional_outputs_left_out(ops, tile):
    """Without filtered / stats / gt the remaining outputs are the same."""
    th, tw = tile
    H, W = th + 3, tw + 9
    rs = np.random.RandomState(3)
    lab = _noise(H, W, 0.5, rs)
    want = cr.components(lab[None], 8, 3, 8)
    got, _ = _launch(ops, lab[None], 8, 3, 8, None, want=())
    assert got["filtered"] is None and got["stats"] is None and got["counts"] is None
    _same(got, want, "ids and n only")


def test_three_images_are_independent_and_numbered_apart(ops, tile):
    th, tw = tile
    H, W = th + 7, 2 * tw + 3
    rs = np.random.RandomState(11)
    labs = np.stack([_noise(H, W, 0.5, rs), _rings(H, W), _checker(H, W)])
    gt = _gt((3, H, W), rs)
    for conn in (4, 8):
        for min_area in (0, 3):
            want = cr.components(labs, conn, min_area, 32, gt, NLAB)
            got, _ = _launch(ops, labs, conn, min_area, 32, gt)
            _same(got, want, ("B = 3", conn, min_area))
            for b in range(3):                                     # each image alone gives its slice: numbering restarts
                one, _ = _launch(ops, labs[b:b + 1], conn, min_area, 32, gt[b:b + 1])
                for k in ("ids", "n", "filtered", "stats", "counts"):
                    assert np.array_equal(one[k][0], got[k][b]), (k, b)
            assert got["ids"][0].max() == got["n"][0, 0] and got["ids"][1].min() >= 0 and got["ids"][1].max() == got["n"][1, 0]


def test_only_stats_truncates(ops, tile):
    """cap = 1, n, n + 1 on the same map: ids, filtered, n and counts never change, stats holds the first min(n, cap) rows."""
    th, tw = tile
    H, W = th + 2, tw + 5
    rs = np.random.RandomState(17)
    lab = _noise(H, W, 0.3, rs)
    gt = _gt((1, H, W), rs)
    comps = [cr.flood(lab, 8)]
    n = len(comps[0])
    assert n > 3
    full = cr.components(lab[None], 8, 0, n + 1, gt, NLAB, comps=comps)
    for cap in (1, n, n + 1):
        got, _ = _launch(ops, lab[None], 8, 0, cap, gt)
        _same(got, cr.components(lab[None], 8, 0, cap, gt, NLAB, comps=comps), cap)
        assert got["n"].tolist() == [[n, n]] and np.array_equal(got["ids"], full["ids"])
        assert np.array_equal(got["stats"][0, :min(n, cap)], full["stats"][0, :min(n, cap)])
        assert not got["stats"][0, n:].any()


def test_a_noop_filter_reproduces_seg_labels_counts(ops):
    """Labels and counts made by ops.seg_labels; seg_components with min_area 0 and 1 returns those counts bit for bit
    and the labels as the filtered map; a real filter changes both."""
    rs = np.random.RandomState(23)
    N, B, H, W = 3, 2, 37, 52
    seg = torch.from_numpy(rs.randint(0, 256, (N, B, 3, H, W)).astype(np.uint8)).cuda()
    mx = seg.view(N, B, -1).amax(-1).to(torch.int32)
    gt = torch.from_numpy(_gt((B, H, W), rs)).cuda()
    labels, counts = ops.seg_labels(seg, mx, gt, r_threshold=0.0, threshold=0.5)
    dev = labels.device
    ids = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    n = torch.empty(B, 2, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.seg_components_workspace(B, H, W), dtype=torch.uint8, device=dev)
    filt = torch.empty_like(labels)
    for min_area in (0, 1):
        mine = torch.full_like(counts, -1)
        ops.seg_components(labels, ids, n, ws, filtered=filt, gt=gt, counts=mine, connectivity=8, min_area=min_area, nlabels=N)
        assert torch.equal(mine, counts) and torch.equal(filt, labels) and bool((n[:, 0] == n[:, 1]).all())
    mine = torch.full_like(counts, -1)
    ops.seg_components(labels, ids, n, ws, filtered=filt, gt=gt, counts=mine, connectivity=4, min_area=4, nlabels=N)
    want = cr.components(labels.cpu().numpy(), 4, 4, 1, gt.cpu().numpy(), N)
    assert np.array_equal(mine.cpu().numpy(), want["counts"]) and np.array_equal(filt.cpu().numpy(), want["filtered"])
    assert not torch.equal(mine, counts) and bool((n[:, 0] < n[:, 1]).all())


def test_poisoned_and_repeated_launches_give_the_same_bits(ops, tile):
    """Outputs and workspace pre-filled with 0xFF and with 0x7B, and two launches back to back into the same buffers: the
    reference's bits every time -- nothing is read before it is written, nothing accumulates across launches."""
    th, tw = tile
    H, W = 2 * th + 1, 2 * tw + 4
    rs = np.random.RandomState(29)
    labs = np.stack([_noise(H, W, 0.5, rs), _snake(H, W)])
    gt = _gt((2, H, W), rs)
    want = cr.components(labs, 8, 2, 8, gt, NLAB)
    for fill in (0xFF, 0x7B):
        got, bufs = _launch(ops, labs, 8, 2, 8, gt, fill=fill)
        _same(got, want, hex(fill))
    again, _ = _launch(ops, labs, 8, 2, 8, gt, bufs=bufs, repeat=2)
    _same(again, want, "back to back")
    other = np.stack([_checker(H, W), _rings(H, W)])               # the same buffers, another map: nothing is left over
    got, _ = _launch(ops, other, 4, 0, 8, gt, bufs=bufs)
    _same(got, cr.components(other, 4, 0, 8, gt, NLAB), "reused buffers")


def test_captured_launch_follows_the_input_tensor(ops, hip_lib, tile):
    """The whole call in one torch.cuda.graph: no memset node, and each replay labels whatever the input tensor holds."""
    th, tw = tile
    B, H, W, cap = 2, th + 9, 2 * tw + 8, 8
    rs = np.random.RandomState(31)
    maps = [np.stack([_noise(H, W, 0.5, rs), _rings(H, W)]), np.stack([_snake(H, W), _noise(H, W, 0.3, rs)])]
    gt = _gt((B, H, W), rs)
    from diffews_amd.objects import ComponentBuffers
    buf = ComponentBuffers(B, H, W, cap)
    lab = torch.zeros(B, H, W, dtype=torch.uint8, device="cuda")
    gtd = torch.from_numpy(gt).cuda()
    counts = buf.counts(NLAB)

    def call():
        ops.seg_components(lab, buf.ids, buf.n, buf.ws, filtered=buf.labels, stats=buf.stats, gt=gtd, counts=counts,
                           connectivity=8, min_area=3, nlabels=NLAB)
    call()                                                         # modules loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    nodes = C.c_int32()
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0
    assert 2 <= nodes.value <= 10                                  # a fixed, small number of launches
    graph.instantiate()
    for m in maps + maps[:1]:
        lab.copy_(torch.from_numpy(m))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(ids=buf.ids.cpu().numpy(), n=buf.n.cpu().numpy(), filtered=buf.labels.cpu().numpy(),
                   stats=buf.stats.cpu().numpy(), counts=counts.cpu().numpy())
        _same(got, cr.components(m, 8, 3, cap, gt, NLAB), "replay")


# ------------------------------------------------------------------------------------------------ objects.py

def test_label_objects_on_a_list_of_native_size_views(hip_lib):
    """Two maps of different sizes cut out of one packed byte buffer at odd offsets, as the native routes return them: one
    call per item, every value of the result a list; a [H, W] tensor comes back without the batch axis."""
    from diffews_amd.objects import ComponentBuffers, label_objects, objects_to_host
    rs = np.random.RandomState(37)
    sizes = [(37, 53), (20, 64)]
    maps = [_noise(h, w, 0.5, rs) for h, w in sizes]
    gts = [_gt((h, w), rs) for h, w in sizes]
    packed = torch.full((3 + 37 * 53 + 20 * 64 + 5,), SENT, dtype=torch.uint8, device="cuda")
    views, off = [], 3
    for m in maps:
        v = packed[off:off + m.size].view(m.shape)
        v.copy_(torch.from_numpy(m))
        views.append(v)
        off += m.size
    r = label_objects(views, gt=[torch.from_numpy(g).cuda() for g in gts], connectivity=4, min_area=2, max_components=512,
                      nlabels=NLAB)
    assert all(isinstance(r[k], list) and len(r[k]) == 2 for k in ("ids", "labels", "n", "stats", "counts"))
    objs, truncated = objects_to_host(r)
    assert not truncated and len(objs) == 2
    for i, (m, g) in enumerate(zip(maps, gts)):
        want = cr.components(m[None], 4, 2, 512, g[None], NLAB)
        assert r["ids"][i].shape == m.shape and r["stats"][i].shape == (512, 8) and r["n"][i].shape == (2,)
        got = dict(ids=r["ids"][i].cpu().numpy()[None], n=r["n"][i].cpu().numpy()[None], filtered=r["labels"][i].cpu().numpy()[None],
                   stats=r["stats"][i].cpu().numpy()[None], counts=r["counts"][i].cpu().numpy()[None])
        _same(got, want, i)
        k = int(want["n"][0, 0])
        assert objs[i] == [(s[0], s[1], (s[2], s[3], s[4], s[5]), s[6]) for s in want["stats"][0, :k].tolist()]
    assert (packed[:3] == SENT).all() and (packed[off:] == SENT).all() and np.array_equal(views[1].cpu().numpy(), maps[1])
    # caller-owned buffers are reused and aliased by the result; a wrong shape is refused
    buf = ComponentBuffers(1, 37, 53, 64)
    r1 = label_objects(views[0][None], buffers=buf)
    assert r1["ids"].data_ptr() == buf.ids.data_ptr() and r1["counts"] is None and r1["ids"].shape == (1, 37, 53)
    with pytest.raises(ValueError):
        label_objects(views[1], buffers=buf)
    with pytest.raises(ValueError):
        label_objects(views[0], gt=torch.from_numpy(gts[0]).cuda())               # a ground truth without nlabels


def test_objects_to_host_reports_truncation(hip_lib):
    from diffews_amd.objects import label_objects, objects_to_host
    lab = torch.from_numpy(np.stack([_checker(9, 11), _rings(9, 11)])).cuda()
    r = label_objects(lab, connectivity=4, max_components=8)
    objs, truncated = objects_to_host(r)
    assert truncated and r["n"].tolist() == [[49, 49], [5, 5]]
    assert len(objs[0]) == 8 and objs[0][0] == (2, 1, (0, 1, 1, 2), 1) and objs[0][7] == (2, 1, (1, 4, 2, 5), 15)
    assert objs[1][0] == (1, 36, (0, 0, 9, 11), 0) and objs[1][4] == (1, 3, (4, 4, 5, 7), 48) and len(objs[1]) == 5
    objs, truncated = objects_to_host(label_objects(lab, connectivity=8, max_components=8))
    assert not truncated and len(objs[0]) == 1 and objs[0][0] == (2, 49, (0, 0, 9, 11), 1)
    one, truncated = objects_to_host(label_objects(lab[1], connectivity=8))
    assert not truncated and one == objs[1]


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


def test_pipe_objects_on_the_n_way_and_tiled_routes(pipe):
    """pipe.objects on the results of segment_classes (b = 2) and segment_tiled (88 x 150): the reference run on the labels
    the route returned, counts against the ground truth included; a result without the asked map is a KeyError."""
    from test_support_bank_gpu import _queries, _support_set
    sets = [_support_set(s, 64, seed=910 + 10 * c) for c, s in enumerate((1, 3, 2))]
    library = pipe.prepare_support_classes([a.cuda() for a, _ in sets], [m.cuda() for _, m in sets])
    N = 3
    rs = np.random.RandomState(41)
    r = pipe.segment_classes(library, _queries(2, 64, 77).cuda(), captured=False)
    gt = _gt((2, 64, 64), rs)
    for kw in (dict(connectivity=8, min_area=0), dict(connectivity=4, min_area=6, max_components=16)):
        o = pipe.objects(r, torch.from_numpy(gt).cuda(), nlabels=N, **kw)
        lab = r["labels"].cpu().numpy()
        want = cr.components(lab, kw["connectivity"], kw["min_area"], kw.get("max_components", 1024), gt, N)
        got = {k: o[k].cpu().numpy() for k in ("ids", "n", "stats", "counts")}
        got["filtered"] = o["labels"].cpu().numpy()
        _same(got, want, ("segment_classes", kw))
    img = rs.randint(0, 256, (88, 150, 3)).astype(np.uint8)
    gt = _gt((88, 150), rs)
    r = pipe.segment_tiled(library, img, gt, batch=3, captured=False)
    o = pipe.objects(r, torch.from_numpy(gt).cuda(), nlabels=N, min_area=3)
    assert o["ids"].shape == (88, 150) and o["n"].shape == (2,)
    want = cr.components(r["labels"].cpu().numpy()[None], 8, 3, 1024, gt[None], N)
    got = {k: o[k].cpu().numpy()[None] for k in ("ids", "n", "stats", "counts")}
    got["filtered"] = o["labels"].cpu().numpy()[None]
    _same(got, want, "segment_tiled")
    # without a filter the counts are the route's own
    o = pipe.objects(r, torch.from_numpy(gt).cuda(), nlabels=N)
    assert torch.equal(o["counts"], r["counts"]) and torch.equal(o["labels"], r["labels"])
    with pytest.raises(KeyError):
        pipe.objects(r, key="pred")
