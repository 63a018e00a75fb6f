"""GPU tests of the outline stage (ops.seg_contours, csrc/seg_contours.hip) against tests/contours_ref.py on n, rings,
ring_off and verts; every comparison is exact.  Random maps of two different images around every block size, aligned (the
16-byte loads) and not, ids from label_objects and raw int32 maps; objects, holes and islands across the block borders;
one long ring around the powers of two that decide the doubling rounds; overflow; one, two and three sort passes; the
second trip of every scan (tests/contours_cases.py, whose sizes tests/test_object_contours_cpu.py proves); poisoned
workspaces, guards, determinism, a captured call, and the stage next to label_objects, fill_holes and the pipeline."""
import ctypes as C

import numpy as np
import pytest
import torch

import contours_cases as cc
import contours_ref as ct
import rle_ref as rr

pytestmark = pytest.mark.gpu

SENT = 0xA5


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def block(hip_lib):
    return cc.block(hip_lib)


def _word(fill):
    return int(np.array([fill] * 4, np.uint8).view(np.int32)[0])


class _Guarded:
    """A tensor inside a flat allocation with `pad` elements of 0xA5 bytes on either side; the tensor itself starts as
    0xA5 bytes too, or as `fill` bytes."""

    def __init__(self, shape, dtype, pad, fill=SENT):
        n = int(np.prod(shape))
        self.flat = torch.empty(n + 2 * pad, dtype=dtype, device="cuda")
        self.flat.view(torch.uint8).fill_(SENT)
        self.t = self.flat[pad:pad + n].view(shape)
        self.pad, self.n = pad, n
        self.t.view(torch.uint8).fill_(fill)

    def check(self, name):
        b = self.flat.view(torch.uint8)
        k = self.flat.element_size()
        assert (b[:self.pad * k] == SENT).all() and (b[(self.pad + self.n) * k:] == SENT).all(), f"wrote outside {name}"


def _launch(ops, ids, cap, max_edges, conn, pad=4, fill=SENT, ws_fill=SENT, repeat=1):
    """ops.seg_contours on `ids` (numpy int32 [B, H, W]) into guarded buffers pre-filled with a byte; `pad` words in front
    of the ids (4: 16-byte aligned, 61: not).  Returns numpy results after checking every guard, and the buffers."""
    B, H, W = ids.shape
    i32 = torch.int32
    bufs = dict(ids=_Guarded((B, H, W), i32, pad), verts=_Guarded((B, max_edges, 2), i32, 4, fill),
                rings=_Guarded((B, max_edges // 4, 4), i32, 4, fill), ring_off=_Guarded((B, cap + 1), i32, 4, fill),
                n=_Guarded((B, 4), i32, 4, fill),
                ws=_Guarded((ops.seg_contours_workspace(B, H, W, cap, max_edges),), torch.uint8, 64, ws_fill))
    bufs["ids"].t.copy_(torch.from_numpy(ids))
    g = {k: v.t for k, v in bufs.items()}
    for _ in range(repeat):
        ops.seg_contours(g["ids"], g["verts"], g["rings"], g["ring_off"], g["n"], g["ws"], cap, conn)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert np.array_equal(g["ids"].cpu().numpy(), ids), "the input was modified"
    return {k: g[k].cpu().numpy() for k in ("verts", "rings", "ring_off", "n")}, bufs


def _same(got, want, what, rest=_word(SENT)):
    """n and ring_off whole, rings and verts up to the kept rows; the rows behind hold `rest`, the buffers' fill."""
    for b, w in enumerate(want):
        assert got["n"][b].tolist() == w["n"].tolist(), (what, b, got["n"][b].tolist(), w["n"].tolist())
        assert np.array_equal(got["ring_off"][b], w["ring_off"]), (what, "ring_off", b)
        nr, nc = len(w["rings"]), len(w["verts"])
        assert np.array_equal(got["rings"][b, :nr], w["rings"]), (what, "rings", b)
        assert np.array_equal(got["verts"][b, :nc], w["verts"]), (what, "verts", b, int((got["verts"][b, :nc] != w["verts"]).any(1).sum()))
        assert (got["rings"][b, nr:] == rest).all() and (got["verts"][b, nc:] == rest).all(), (what, "rows behind the kept ones", b)


def _check(ops, ids, cap, conn, max_edges=None, what=None, **kw):
    want = ct.expected(ids, cap, conn, 1 << 30)
    found = max(int(w["n"][0]) for w in want)
    E = max(4, cc.up4(found)) if max_edges is None else max_edges
    if E < found:
        want = ct.expected(ids, cap, conn, E)
    got, _ = _launch(ops, ids, cap, E, conn, **kw)
    _same(got, want, what)
    return got, want


def _label(labels, conn, cap):
    from diffews_amd.objects import label_objects
    return label_objects(torch.from_numpy(labels).cuda(), connectivity=conn, max_components=cap)


# ------------------------------------------------------------------------------------------------ random maps

def _shapes(block):
    P, _ = block
    assert P % 64 == 0 and (P + 1) % 3 == 0
    return [(1, 1), (1, 2), (2, 3), (3, 5), (5, 5), (1, P - 1), (1, P), (1, P + 1), (P - 1, 1), (P, 1), (P + 1, 1), (2, P),
            (P // 64, 64), (3, (P + 1) // 3), (75, 3 * P // 75 + 2), (70, 60)]


@pytest.mark.parametrize("which", range(16), ids=["1x1", "1x2", "2x3", "3x5", "5x5", "1xP-1", "1xP", "1xP+1", "P-1x1", "Px1", "P+1x1",
                                                  "2xP", "block", "block+1", "3-blocks-odd-W", "W%4==0"])
def test_random_maps_equal_the_reference(ops, block, which):
    """B = 2, two different images, both connectivities: ids from label_objects of noise (cap above, at a few and at 1),
    and raw int32 maps with negatives and ids above cap, which match neither connectivity.  Where W is a multiple of 4 the
    aligned ids take the 16-byte loads and the ids 61 words into their allocation the scalar ones."""
    P, E = block
    H, W = _shapes(block)[which]
    rs = np.random.RandomState(1000 * H + W)
    c = rr.contents(H, W, rs)
    labels = np.stack([c["noise 0.5"], c["noise 0.3"]])
    for conn in (4, 8):
        o = _label(labels, conn, 8)
        ids = o["ids"].cpu().numpy()
        top = int(ids.max())
        for cap in sorted({1, 16, top + 3}):
            for pad in ((4, 61) if W % 4 == 0 else (4,)):
                _check(ops, ids, cap, conn, what=(H, W, conn, cap, pad), pad=pad)
        raw = rs.randint(-3, 9, (2, H, W)).astype(np.int32)
        _check(ops, raw, 5, conn, what=(H, W, conn, "raw"))
    if which == 14:
        assert ct.expected(ids, top + 3, 8, 1 << 30)[0]["n"][0] > 2 * E       # several blocks of edges


def test_objects_holes_and_islands_across_the_block_borders(ops, block):
    """Object, hole, island object, hole in the island, twice over, in maps whose blocks of P pixels end in the middle of
    a row (96 and 83 columns): every ring straddles every internal border of the pixel blocks, and a comb of thin holes
    has more edges than one block of the ring count."""
    P, E = block
    for H, W in ((70, 96), (75, 83)):
        assert H * W > 3 * P and P % W != 0
        a = np.zeros((H, W), np.int32)
        for k, m in enumerate((1, 6, 11, 16, 21, 26)):                       # frames 1, 2, 3, ..: each inside the hole before
            a[m:H - m, m:W - m] = k + 1
            a[m + 2:H - m - 2, m + 2:W - m - 2] = 0
        a[31:H - 31, 31:W - 31] = 7
        b = np.zeros((H, W), np.int32)
        b[2:H - 2, 1:W - 1] = 1
        b[4:H - 4:2, 3:W - 3] = 0                                          # a comb: long thin holes, thousands of edges
        b[10:H - 10, W // 2] = 1
        ids = np.stack([a, b])
        for conn in (4, 8):
            got, want = _check(ops, ids, 9, conn, what=(H, W, conn))
            assert want[0]["n"][2] == 13 and (want[0]["rings"][1::2, 3] < 0).all()
            assert want[1]["n"][0] > E
            # the same with every frame one object: one outer ring and the holes behind it
            _check(ops, np.minimum(ids, 1), 1, conn, what=(H, W, conn, "one id"))


# ------------------------------------------------------------------------------------------------ long rings

@pytest.mark.parametrize("name", ["row30", "row31", "row32", "serpentine", "row-above-block", "rowE-2", "rowE-1", "rowE"])
def test_one_long_ring(ops, hip_lib, block, name):
    """One ring of L edges with max_edges = L rounded up to a multiple of 4: L just below, at and above 64 and 2 E, where
    the number of doubling rounds changes, a serpentine, and a ring longer than a block of the ring count."""
    P, E = block
    rings = cc.long_rings(hip_lib)
    ids, L = rings[name.replace("E-2", str(E - 2)).replace("E-1", str(E - 1)).replace("rowE", f"row{E}")]
    for conn in (4, 8):
        got, want = _check(ops, ids[None], 1, conn, max_edges=cc.up4(L), what=(name, conn))
        assert got["n"][0].tolist() == [L, len(want[0]["verts"]), 1, 1]
        assert got["rings"][0, 0].tolist() == [1, 0, len(want[0]["verts"]), int(ids.sum())]
    # among other rings and in the second image, with room to spare
    two = np.zeros((2, ids.shape[0] + 4, ids.shape[1] + 3), np.int32)
    two[0, :2, :2], two[1, 2:2 + ids.shape[0], 1:1 + ids.shape[1]], two[1, -1, -1] = 2, ids, 3
    _check(ops, two, 3, 8, max_edges=cc.up4(L) + 64, what=(name, "two images"))


# ------------------------------------------------------------------------------------------------ overflow

def test_overflow_writes_the_count_and_nothing_else(ops, block):
    """The same batch with max_edges at the larger image's edge count, four below it, below the smaller image's, and 4."""
    rs = np.random.RandomState(5)
    c = rr.contents(41, 52, rs)
    ids = np.zeros((2, 41, 55), np.int32)
    ids[:, :, :52] = _label(np.stack([c["noise 0.5"], c["vertical stripes"]]), 8, 8)["ids"].cpu().numpy()
    cap = int(ids.max()) + 1
    if len(ct.edges(ids[0], cap)) % 4:                                     # a 2 x 1 object has six edges
        ids[0, :2, 54] = cap
    found = [int(w["n"][0]) for w in ct.expected(ids, cap, 8, 1 << 30)]
    assert found[0] % 4 == 0 and found[0] > cc.up4(found[1]) + 4 > 12
    for E, complete in ((found[0], [1, 1]), (found[0] - 4, [0, 1]), (cc.up4(found[1]) - 4, [0, 0]), (4, [0, 0])):
        got, want = _check(ops, ids, cap, 8, max_edges=E, what=E)
        assert got["n"][:, 3].tolist() == complete and got["n"][:, 0].tolist() == found
        for b in range(2):
            if not complete[b]:
                assert got["n"][b, 1:].tolist() == [0, 0, 0] and not got["ring_off"][b].any()
                assert (got["verts"][b] == _word(SENT)).all() and (got["rings"][b] == _word(SENT)).all()


# ------------------------------------------------------------------------------------------------ many rings

@pytest.mark.parametrize("case", cc.SORT_CASES, ids=[f"{h}x{w}-cap{c}" for h, w, c, _ in cc.SORT_CASES])
def test_checkerboards_across_the_sort_passes(ops, hip_lib, case):
    """A 4-connected checkerboard: every object one ring of four edges; cap = 255, 256 and 131072 give one, two and three
    sort passes (512 x 512: 131 072 objects, 524 288 edges).  The ids are permuted, so the sort has work to do."""
    H, W, cap, passes = case
    ids = cc.checkerboard(H, W)
    n = int(ids.max())
    assert cc.trips(hip_lib, 1, H, W, cap, 4 * n)["passes"] == passes
    perm = np.concatenate([[0], 1 + np.random.RandomState(n).permutation(n)]).astype(np.int32)
    ids = perm[ids]
    got, want = _check(ops, ids[None], cap, 4, max_edges=4 * n, what=case)
    assert got["n"][0].tolist() == [4 * n, 4 * n, n, 1] and (got["rings"][0, :n, 0] == np.arange(1, n + 1)).all()
    assert (np.diff(got["ring_off"][0, :n + 1]) == 1).all()


@pytest.mark.parametrize("name", ["block_scan", "block_scan-odd", "ring_scan", "table_scan", "offsets_scan", "corners_scan"])
def test_second_trip_of_every_scan(ops, hip_lib, name):
    case = cc.second_trip_cases(hip_lib)[name]
    H, W = case["ids"].shape
    assert cc.trips(hip_lib, 2, H, W, case["cap"], case["max_edges"])[case["field"]] == 2
    ids = np.stack([case["ids"], case["ids"][::-1, ::-1]])
    got, want = _check(ops, ids, case["cap"], 8, max_edges=case["max_edges"], what=name)
    assert got["n"][:, 3].tolist() == [1, 1] and got["n"][0, 2] == want[0]["n"][2] > 0


# ------------------------------------------------------------------------------------------------ poison, guards, repeats

def test_poisoned_workspaces_and_repeated_launches_give_the_same_bytes(ops, block):
    """The workspace filled with 0xFF and with 0x7B, the outputs with 0xA5 and 0x00: nothing is read before it is written,
    the kept rows do not depend on what lay there, the rows behind them and every guard stay as they were.  Five launches
    into the same buffers and a second run give equal bytes."""
    rs = np.random.RandomState(9)
    c = rr.contents(75, 83, rs)
    ids = _label(np.stack([c["noise 0.5"], c["snake"]]), 8, 8)["ids"].cpu().numpy()
    cap = int(ids.max()) + 2
    want = ct.expected(ids, cap, 8, 1 << 30)
    E = cc.up4(max(int(w["n"][0]) for w in want)) + 40
    runs = []
    for ws_fill, fill, repeat in ((0xFF, SENT, 1), (0x7B, SENT, 1), (0x00, 0x00, 1), (0xFF, SENT, 5), (0xFF, SENT, 1)):
        got, _ = _launch(ops, ids, cap, E, 8, fill=fill, ws_fill=ws_fill, repeat=repeat)
        _same(got, want, (ws_fill, fill, repeat), rest=_word(fill))
        runs.append(got)
    for k in ("verts", "rings", "ring_off", "n"):
        assert runs[0][k].tobytes() == runs[1][k].tobytes() == runs[3][k].tobytes() == runs[4][k].tobytes(), k
    # one image not complete among the poison: its rows stay
    small = cc.up4(min(int(w["n"][0]) for w in want))
    for ws_fill in (0xFF, 0x7B):
        got, _ = _launch(ops, ids, cap, small, 8, ws_fill=ws_fill)
        _same(got, ct.expected(ids, cap, 8, small), ("overflow", ws_fill))


def test_captured_call_follows_the_input(ops, hip_lib):
    """One capture on one stream, replayed on two different maps of one shape (and the first again): exact each time; the
    graph holds the launches the rounds query states and no memset node."""
    rs = np.random.RandomState(31)
    B, H, W, cap, E = 2, 41, 72, 300, 8192
    c = rr.contents(H, W, rs)
    maps = [np.stack([c["noise 0.5"], c["rings"]]), np.stack([c["snake"], c["background"]])]
    from diffews_amd.objects import ContourBuffers
    cb = ContourBuffers(B, H, W, cap, max_edges=E)
    ids = torch.zeros(B, H, W, dtype=torch.int32, device="cuda")

    def call():
        ops.seg_contours(ids, cb.verts, cb.rings, cb.ring_off, cb.n, cb.ws, cap, 8)
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    nodes = C.c_int32()
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0
    assert nodes.value == cc.trips(hip_lib, B, H, W, cap, E)["launches"] == 14 + 2 * 13 + 3 * 2
    graph.instantiate()
    for m in maps + maps[:1]:
        m = _label(m, 8, 8)["ids"]
        ids.copy_(m)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: getattr(cb, k).cpu().numpy() for k in ("verts", "rings", "ring_off", "n")}
        for b, w in enumerate(ct.expected(m.cpu().numpy(), cap, 8, E)):
            assert got["n"][b].tolist() == w["n"].tolist() and np.array_equal(got["ring_off"][b], w["ring_off"])
            assert np.array_equal(got["rings"][b, :len(w["rings"])], w["rings"])
            assert np.array_equal(got["verts"][b, :len(w["verts"])], w["verts"])


# ------------------------------------------------------------------------------------------------ with the other stages

def test_next_to_label_objects_and_fill_holes(ops):
    """The ring areas of every object sum to column 1 of stats, rings_to_mask gives ids == k, and after
    fill_holes(max_area=None) the ring count drops by the regions filled, in a map where every enclosed region is bordered
    by its owner only."""
    from diffews_amd.objects import (ContourBuffers, contours_to_host, fill_holes, label_objects, object_contours,
                                     rings_to_geojson, rings_to_mask)
    H, W = 90, 110
    rs = np.random.RandomState(17)
    lab = np.zeros((2, H, W), np.uint8)
    yy, xx = np.mgrid[:H, :W]
    for b in range(2):
        for i, (cy, cx) in enumerate(((20, 25), (22, 80), (65, 30), (62, 82))):
            lab[b][(yy - cy) ** 2 + (xx - cx) ** 2 <= 18 ** 2] = 1 + (i + b) % 3
            for _ in range(4 + b):                                           # pinholes well inside the disc, apart
                hy, hx = cy + rs.randint(-9, 10), cx + rs.randint(-9, 10)
                lab[b, hy:hy + 2, hx:hx + 1 + b] = 0
    for conn in (4, 8):
        o = label_objects(torch.from_numpy(lab).cuda(), connectivity=conn, max_components=16)
        c = object_contours(o, connectivity=conn)
        assert c["shape"] == (H, W) and c["connectivity"] == conn and c["verts"].shape == (2, 4096, 2)
        ids, stats, n = o["ids"].cpu().numpy(), o["stats"].cpu().numpy(), o["n"].cpu().numpy()
        for b, w in enumerate(ct.expected(ids, 16, conn, 4096)):
            assert c["n"][b].tolist() == w["n"].tolist() and np.array_equal(c["ring_off"][b].cpu().numpy(), w["ring_off"])
            assert np.array_equal(c["rings"][b, :len(w["rings"])].cpu().numpy(), w["rings"])
            assert np.array_equal(c["verts"][b, :len(w["verts"])].cpu().numpy(), w["verts"])
        host, incomplete = contours_to_host(c)
        assert not incomplete
        for b in range(2):
            assert len(host[b]) == n[b, 0] == 4
            for k, rings in enumerate(host[b], 1):
                assert sum(a for a, _ in rings) == stats[b, k - 1, 1]
                assert rings[0][0] > 0 and all(a < 0 for a, _ in rings[1:])
                assert np.array_equal(rings_to_mask(rings, H, W), ids[b] == k)
                assert len(rings_to_geojson(rings)["coordinates"]) == len(rings)
        f = fill_holes(o, max_area=None, connectivity=conn)
        holes = f["holes"].cpu().numpy()
        assert (holes[:, 0] == holes[:, 1]).all() and (holes[:, 0] > 0).all()
        cf = object_contours(f, connectivity=conn, buffers=ContourBuffers(2, H, W, 16))
        nc, nf = c["n"].cpu().numpy(), cf["n"].cpu().numpy()
        assert (nc[:, 2] - nf[:, 2] == holes[:, 0]).all() and (nf[:, 2] == 4).all() and (nf[:, 3] == 1).all()
        filled, _ = contours_to_host(cf)
        fids = f["ids"].cpu().numpy()
        for b in range(2):
            for k, rings in enumerate(filled[b], 1):
                assert len(rings) == 1 and np.array_equal(rings_to_mask(rings, H, W), fids[b] == k)
        # a [H, W] map, an id tensor with max_components, and a list: one call per item
        one = object_contours(o["ids"][1], connectivity=conn, max_components=16, max_edges=2048)
        assert one["n"].shape == (4,) and one["verts"].shape == (2048, 2)
        assert one["n"].tolist() == nc[1].tolist() and torch.equal(one["rings"][:nc[1, 2]], c["rings"][1, :nc[1, 2]])
        many = object_contours([o["ids"][0], o["ids"][1, :50, :60].contiguous()], connectivity=conn, max_components=16)
        assert many["shape"] == [(H, W), (50, 60)] and many["n"][0].tolist() == nc[0].tolist()
        want = ct.expected(ids[1:, :50, :60], 16, conn, 4096)[0]
        assert many["n"][1].tolist() == want["n"].tolist()
        assert np.array_equal(many["verts"][1][:len(want["verts"])].cpu().numpy(), want["verts"])
        with pytest.raises(ValueError):
            object_contours(o, connectivity=conn, buffers=ContourBuffers(2, H, W, 17))


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


def test_pipe_object_contours_agrees_with_objects(pipe):
    from diffews_amd.objects import object_contours
    from test_support_bank_gpu import _queries, _support_set
    sets = [_support_set(s, 64, seed=910 + 10 * c) for c, s in enumerate((1, 3, 2))]
    library = pipe.prepare_support_classes([a.cuda() for a, _ in sets], [m.cuda() for _, m in sets])
    r = pipe.segment_classes(library, _queries(2, 64, 77).cuda(), captured=False)
    o = pipe.objects(r, connectivity=8, max_components=256)
    a, b = pipe.object_contours(o, max_edges=8192), object_contours(o, max_edges=8192)
    assert a["shape"] == (64, 64) and a["ring_off"].shape == (2, 257)
    n = a["n"].cpu().numpy()
    assert torch.equal(a["n"], b["n"]) and torch.equal(a["ring_off"], b["ring_off"])
    want = ct.expected(o["ids"].cpu().numpy(), 256, 8, 8192)
    for i, w in enumerate(want):
        assert n[i].tolist() == w["n"].tolist()
        for x in (a, b):
            assert np.array_equal(x["rings"][i, :n[i, 2]].cpu().numpy(), w["rings"])
            assert np.array_equal(x["verts"][i, :n[i, 1]].cpu().numpy(), w["verts"])
