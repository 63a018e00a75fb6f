"""GPU tests of the simplified rings (ops.seg_contours with simp_verts / simp_rings / simp_n / tol4, csrc/seg_contours.hip)
against tests/simplify_ref.py; every comparison is exact.  Random maps of two images under both connectivities and nine
tolerances, with the four original outputs byte-equal to a call without the stage; the named shapes of the header and of
the tie rules; rings around the LDS block (dfw_seg_contours_simplify_block) in both tiers; a staircase that needs many
rounds and a triangle whose products pass 2^32; overflow; poisoned workspaces, guards and repeats; LDS poison; a captured
call; and the stage behind objects.object_contours and the pipeline."""
import ctypes as C

import numpy as np
import pytest
import torch

import contours_cases as cc
import contours_ref as ct
import simplify_ref as sr
import test_object_contours_gpu as tco
from test_object_simplify_cpu import diagonal_squares, plus, square, staircase

pytestmark = pytest.mark.gpu

SENT = tco.SENT
TOLS = (0, 1, 2, 4, 6, 10, 40, 4000, 32768)
ORIGINAL = ("verts", "rings", "ring_off", "n")
SIMP = ("simp_verts", "simp_rings", "simp_n")


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def lds_block(ops):
    L = ops.seg_contours_simplify_block()
    assert L >= 256 and L % 2 == 0
    return L


def _launch(ops, ids, cap, max_edges, conn, tol4=None, pad=4, fill=SENT, ws_fill=SENT, repeat=1):
    """ops.seg_contours on `ids` (numpy int32 [B, H, W]) into guarded buffers pre-filled with a byte, the three simplified
    outputs among them unless tol4 is None (the stage off).  Returns numpy results after checking every guard."""
    B, H, W = ids.shape
    i32, G = torch.int32, tco._Guarded
    bufs = dict(ids=G((B, H, W), i32, pad), verts=G((B, max_edges, 2), i32, 4, fill), rings=G((B, max_edges // 4, 4), i32, 4, fill),
                ring_off=G((B, cap + 1), i32, 4, fill), n=G((B, 4), i32, 4, fill),
                ws=G((ops.seg_contours_workspace(B, H, W, cap, max_edges),), torch.uint8, 64, ws_fill))
    if tol4 is not None:
        bufs.update(simp_verts=G((B, max_edges, 2), i32, 4, fill), simp_rings=G((B, max_edges // 4, 4), i32, 4, fill),
                    simp_n=G((B, 4), i32, 4, fill))
    bufs["ids"].t.copy_(torch.from_numpy(ids))
    g = {k: v.t for k, v in bufs.items()}
    extra = {} if tol4 is None else dict(simp_verts=g["simp_verts"], simp_rings=g["simp_rings"], simp_n=g["simp_n"], tol4=tol4)
    for _ in range(repeat):
        ops.seg_contours(g["ids"], g["verts"], g["rings"], g["ring_off"], g["n"], g["ws"], cap, conn, **extra)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert np.array_equal(g["ids"].cpu().numpy(), ids), "the input was modified"
    return {k: g[k].cpu().numpy() for k in ORIGINAL + (SIMP if tol4 is not None else ())}


def _same(got, base, want, what, rest=tco._word(SENT)):
    """The original tables against contours_ref and the simplified ones against simplify_ref; rows behind the kept ones
    hold `rest`, the buffers' fill."""
    tco._same(got, base, what, rest)
    for b, w in enumerate(want):
        assert got["simp_n"][b].tolist() == w["n"].tolist(), (what, b, got["simp_n"][b].tolist(), w["n"].tolist())
        nr, nc = len(w["rings"]), len(w["verts"])
        assert np.array_equal(got["simp_rings"][b, :nr], w["rings"]), (what, "simp_rings", b)
        assert np.array_equal(got["simp_verts"][b, :nc], w["verts"]), (what, "simp_verts", b, int((got["simp_verts"][b, :nc] != w["verts"]).any(1).sum()))
        assert (got["simp_rings"][b, nr:] == rest).all() and (got["simp_verts"][b, nc:] == rest).all(), (what, "rows behind the kept ones", b)


def _check(ops, ids, cap, conn, tols, max_edges=None, what=None, base=None, **kw):
    """One launch per tolerance of `tols` against the reference; returns the last result and the references."""
    if base is None:
        base = ct.expected(ids, cap, conn, 1 << 30)
        found = max(int(w["n"][0]) for w in base)
        max_edges = max(4, cc.up4(found)) if max_edges is None else max_edges
        if max_edges < found:
            base = ct.expected(ids, cap, conn, max_edges)
    got, want = None, None
    for tol4 in tols:
        want = sr.expected(ids, cap, conn, max_edges, tol4, base=base)
        got = _launch(ops, ids, cap, max_edges, conn, tol4, **kw)
        _same(got, base, want, (what, conn, tol4))
    return got, base, want


# ------------------------------------------------------------------------------------------------ random maps

@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("shape,pad", [((37, 45), 4), ((36, 44), 61)], ids=["odd-W", "W%4==0-unaligned"])
def test_random_maps_equal_the_reference(ops, shape, pad, conn):
    """B = 2, two different images: ids from label_objects of blobs, and raw int32 maps with negatives and ids above cap.
    Every tolerance: the simplified tables equal the reference, the four original outputs are byte-equal to a call without
    the stage, and at tol4 = 0 the simplified rows are the original rows."""
    H, W = shape
    rs = np.random.RandomState(100 * H + W + conn)
    labels = np.stack([cc.blobs(H, W, rs, n=14), cc.blobs(H, W, rs, n=9)])
    o = tco._label(labels, conn, 64)
    maps = [(o["ids"].cpu().numpy(), int(o["ids"].max()) + 3), (rs.randint(-3, 9, (2, H, W)).astype(np.int32), 5)]
    for ids, cap in maps:
        base = ct.expected(ids, cap, conn, 1 << 30)
        E = cc.up4(max(int(w["n"][0]) for w in base)) + 8
        off = _launch(ops, ids, cap, E, conn, None, pad=pad)
        tco._same(off, base, (shape, conn, "off"))
        for tol4 in TOLS:
            got, _, want = _check(ops, ids, cap, conn, (tol4,), max_edges=E, base=base, what=shape, pad=pad)
            for k in ORIGINAL:
                assert got[k].tobytes() == off[k].tobytes(), (k, tol4)
            kept = [int(w["n"][1]) for w in want]
            if tol4 == 0:
                for b, w in enumerate(base):
                    nr, nc = len(w["rings"]), len(w["verts"])
                    assert got["simp_n"][b].tolist() == [nc, nc, nr, 1]
                    assert np.array_equal(got["simp_rings"][b, :nr], got["rings"][b, :nr])
                    assert np.array_equal(got["simp_verts"][b, :nc], got["verts"][b, :nc])
            elif tol4 == 32768:
                assert kept == [3 * len(w["rings"]) for w in base]             # nothing but the anchors and rule 3
        assert sum(int(w["n"][2]) for w in base) > 10


# ------------------------------------------------------------------------------------------------ named shapes

def _frame():
    return np.array([[1, 1, 1, 1], [1, 0, 0, 1], [1, 1, 1, 1]], np.int32)


NAMED = {
    "one pixel": (np.ones((1, 1), np.int32), 8, (0, 4, 32768)),
    "frame with a hole two pixels wide": (_frame(), 8, (0, 2, 4, 8, 40)),                 # the leader's start is no corner
    "diamond": (np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], np.int32), 8, (0, 2, 4, 6, 40)),
    "diamond of four objects": (np.array([[0, 1, 0], [2, 0, 3], [0, 4, 0]], np.int32), 4, (0, 4)),
    "two pixels touching diagonally": (np.array([[1, 0], [0, 1]], np.int32), 8, (0, 2, 3, 4, 5, 40)),        # rule 3
    "two squares touching diagonally": (diagonal_squares(), 8, (0, 1, 2, 4, 12, 17, 40)),   # point mode
    "square": (square(5), 8, (0, 4, 14, 15, 40, 32768)),
    "plus sign": (plus(), 8, (0, 4, 8, 12, 13, 40)),
    "long rectangle": (np.ones((2, 40), np.int32), 4, (0, 4, 7, 8, 9, 40)),
    "unit staircase": (staircase(40), 8, (0, 1, 2, 3, 4)),
}


@pytest.mark.parametrize("name", list(NAMED))
def test_named_shapes(ops, name):
    ids, conn, tols = NAMED[name]
    cap = int(ids.max())
    got, base, want = _check(ops, ids[None], cap, conn, tols, what=name)
    if name == "two pixels touching diagonally":
        got, _, want = _check(ops, ids[None], 1, 8, (4,), what=name)
        assert got["simp_n"][0].tolist() == [8, 3, 1, 1] and got["simp_rings"][0, 0].tolist() == [1, 0, 3, 2]
        assert got["simp_verts"][0, :3].tolist() == [[0, 0], [1, 0], [2, 2]]               # ranks 0, 1, 4
    if name == "frame with a hole two pixels wide":
        assert got["simp_rings"][0, :2].tolist() == [[1, 0, 3, 12], [1, 3, 3, -2]]          # at 10 pixels: rule 3 twice
    if name == "unit staircase":
        assert sr.simplify_rounds(base[0]["verts"], 2)[1] <= 12 and got["simp_n"][0].tolist() == [82, 3, 1, 1]


# ------------------------------------------------------------------------------------------------ tiers

def comb(teeth, notch=False):
    """`teeth` teeth one pixel wide on a base two pixels thick: one ring of 4 * teeth corners, two more with the base's
    lower right pixel cut off."""
    a = np.zeros((4, 2 * teeth - 1), np.int32)
    a[2:], a[:2, ::2] = 1, 1
    if notch:
        a[3, -1] = 0
    return a


def _comb_of(corners):
    ids = comb(corners // 4, corners % 4 == 2)
    assert ct.trace(ids, 1, 8)["rings"].tolist() == [[1, 0, corners, int(ids.sum())]]
    return ids


@pytest.mark.parametrize("which", ["L-2", "L", "L+2", "3L", "short-and-long"])
def test_rings_around_the_lds_block(ops, lds_block, which):
    """A ring of L - 2 and of L corners keeps its state in LDS, one of L + 2 and of about 3 L in the workspace; every one has
    at least 257 corners, so the strided loops run a second trip.  The last case holds a short and a long ring in one
    image and the long one alone in the other."""
    L = lds_block
    if which == "short-and-long":
        long_, short = _comb_of(2 * L + 2), _comb_of(L // 2)
        ids = np.zeros((2, 10, long_.shape[1]), np.int32)
        ids[0, :4], ids[0, 6:, :short.shape[1]], ids[1, 3:7] = long_, 2 * short, long_
        cap = 2
    else:
        corners = {"L-2": L - 2, "L": L, "L+2": L + 2, "3L": 3 * L + 2}[which]
        assert corners >= 257
        ids, cap = _comb_of(corners)[None], 1
    _check(ops, ids, cap, 8, (0, 2, 4, 5, 8, 9, 40, 32768), what=which)


# ------------------------------------------------------------------------------------------------ many rounds, large products

def grown_staircase(steps):
    """A staircase whose k-th step is steps[k] wide and steps[k] high, filled below: the corners' distances from the
    diagonal grow with the steps, so a chain keeps splitting at its far end."""
    n = sum(steps)
    a = np.zeros((n, n), np.int32)
    at = 0
    for s in steps:
        a[at:, at:at + s] = 1
        at += s
    return a


def test_a_staircase_of_growing_steps_needs_many_rounds(ops):
    ids = grown_staircase([int(1.25 ** k) for k in range(26)])
    assert 1300 <= ids.shape[0] <= 1350
    base = ct.expected(ids[None], 1, 8, 1 << 30)
    rounds = max(sr.simplify_tables(base[0], tol4)["rounds"] for tol4 in (1, 2))
    assert rounds >= 24, rounds
    E = cc.up4(int(base[0]["n"][0]))
    _check(ops, ids[None], 1, 8, (1, 2, 8, 400), max_edges=E, base=base, what="grown staircase")


def test_a_triangle_whose_products_pass_32_bits(ops, lds_block):
    """np.tril(1500): 3002 corners in the workspace tier, |cross| up to 1500^2 and its square far above 2^32."""
    ids = staircase(1500)
    base = ct.expected(ids[None], 1, 8, 1 << 30)
    pts = base[0]["verts"]
    assert len(pts) == 3002 > lds_block
    far = max(sr.measure(tuple(pts[0]), tuple(pts[sr.anchor([tuple(p) for p in pts.tolist()])]), tuple(p))[0] for p in pts.tolist())
    assert far * far > 2 ** 32 and far > 2 ** 20
    _check(ops, ids[None], 1, 8, (1, 2, 3, 4000, 4244), max_edges=cc.up4(int(base[0]["n"][0])), base=base, what="triangle")


# ------------------------------------------------------------------------------------------------ overflow

def test_an_image_that_is_not_complete_writes_zeros_and_no_row(ops):
    rs = np.random.RandomState(5)
    ids = np.zeros((2, 41, 55), np.int32)
    ids[0] = tco._label(cc.blobs(41, 55, rs, n=30)[None], 8, 64)["ids"].cpu().numpy()[0]
    ids[1, 5:30, 5:40], ids[1, 10:20, 10:30] = 1, 0
    cap = int(ids.max()) + 1
    found = [int(w["n"][0]) for w in ct.expected(ids, cap, 8, 1 << 30)]
    E = cc.up4(found[1]) + 4
    assert found[0] > E >= found[1]
    for order in (ids, ids[::-1].copy()):
        got, base, want = _check(ops, order, cap, 8, (0, 4, 40), max_edges=E, what="overflow")
        b = 0 if order is ids else 1
        assert got["n"][b].tolist() == [found[0], 0, 0, 0] and got["simp_n"][b].tolist() == [0, 0, 0, 0]
        assert (got["simp_verts"][b] == tco._word(SENT)).all() and (got["simp_rings"][b] == tco._word(SENT)).all()
        assert got["simp_n"][1 - b, [0, 2, 3]].tolist() == [8, 2, 1] and 6 <= got["simp_n"][1 - b, 1] <= 8


# ------------------------------------------------------------------------------------------------ poison, guards, repeats

def test_poisoned_workspaces_and_repeated_launches_give_the_same_bytes(ops, lds_block):
    """A long comb (the workspace tier) and blobs (the LDS tier) in one batch; the workspace filled with 0xFF and with
    0x7B, the outputs with 0xA5 and 0x00; five launches into the same buffers."""
    rs = np.random.RandomState(9)
    long_ = _comb_of(lds_block + 6)
    H, W = 40, long_.shape[1]
    ids = np.zeros((2, H, W), np.int32)
    ids[0] = tco._label(cc.blobs(H, W, rs, n=40)[None], 8, 255)["ids"].cpu().numpy()[0]
    ids[1, 2:6], ids[1, 10:30, 4:60], ids[1, 15:20, 10:40] = long_, 2, 0
    cap = int(ids.max()) + 2
    base = ct.expected(ids, cap, 8, 1 << 30)
    E = cc.up4(max(int(w["n"][0]) for w in base)) + 40
    want = sr.expected(ids, cap, 8, E, 6, base=base)
    runs = []
    for ws_fill, fill, repeat in ((0xFF, SENT, 1), (0x7B, SENT, 1), (0x00, 0x00, 1), (0xFF, SENT, 5), (0xFF, SENT, 1)):
        got = _launch(ops, ids, cap, E, 8, 6, fill=fill, ws_fill=ws_fill, repeat=repeat)
        _same(got, base, want, (ws_fill, fill, repeat), rest=tco._word(fill))
        runs.append(got)
    for k in ORIGINAL + SIMP:
        assert runs[0][k].tobytes() == runs[1][k].tobytes() == runs[3][k].tobytes() == runs[4][k].tobytes(), k


# ------------------------------------------------------------------------------------------------ LDS poison

@pytest.mark.parametrize("tier", ["lds", "workspace"])
def test_lds_poison(ops, lds_block, tier):
    """Plain, then with every CU's LDS filled with 0xFF, 0x7B and 0x00 in front of the call: byte-equal, and equal to the
    reference.  The LDS tier reads coordinates, state and slots from LDS, the workspace tier its reduction words."""
    from test_lds_poison_gpu import four_runs
    rs = np.random.RandomState(3)
    if tier == "lds":
        labels = np.stack([cc.blobs(37, 45, rs, n=14), cc.blobs(37, 45, rs, n=9)])
        ids = tco._label(labels, 8, 64)["ids"].cpu().numpy()
    else:
        ids = np.stack([_comb_of(lds_block + 2), _comb_of(lds_block + 2)[::-1, ::-1]])
    cap = int(ids.max()) + 1
    base = ct.expected(ids, cap, 8, 1 << 30)
    E = cc.up4(max(int(w["n"][0]) for w in base))
    want = sr.expected(ids, cap, 8, E, 4, base=base)
    four_runs("dfw_seg_contours", lambda: _launch(ops, ids, cap, E, 8, 4, pad=61),
              lambda got: _same(got, base, want, ("lds poison", tier)), ("seg_contours simplify", tier))


# ------------------------------------------------------------------------------------------------ capture

def test_captured_call_follows_the_input(ops, hip_lib):
    """One capture replayed on two maps: exact each time; the graph holds launches + simplify_launches kernel nodes and no
    memset node."""
    import rle_ref as rr
    from diffews_amd.objects import ContourBuffers
    rs = np.random.RandomState(31)
    B, H, W, cap, E = 2, 41, 72, 300, 8192
    c = rr.contents(H, W, rs)
    maps = [np.stack([c["noise 0.5"], c["rings"]]), np.stack([c["snake"], cc.blobs(H, W, rs, n=20)])]
    cb = ContourBuffers(B, H, W, cap, max_edges=E, simplify=True)
    ids = torch.zeros(B, H, W, dtype=torch.int32, device="cuda")

    def call():
        ops.seg_contours(ids, cb.verts, cb.rings, cb.ring_off, cb.n, cb.ws, cap, 8, cb.simp_verts, cb.simp_rings, cb.simp_n, 4)
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    nodes = C.c_int32()
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0
    t = cc.trips(hip_lib, B, H, W, cap, E)
    assert nodes.value == t["launches"] + t["simplify_launches"] == 14 + 2 * 13 + 3 * 2 + 3
    graph.instantiate()
    for m in maps + maps[:1]:
        m = tco._label(m, 8, 8)["ids"]
        ids.copy_(m)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: getattr(cb, k).cpu().numpy() for k in ORIGINAL + SIMP}
        base = ct.expected(m.cpu().numpy(), cap, 8, E)
        for b, w in enumerate(sr.expected(m.cpu().numpy(), cap, 8, E, 4, base=base)):
            assert got["n"][b].tolist() == base[b]["n"].tolist() and got["simp_n"][b].tolist() == w["n"].tolist()
            assert np.array_equal(got["verts"][b, :len(base[b]["verts"])], base[b]["verts"])
            assert np.array_equal(got["simp_rings"][b, :len(w["rings"])], w["rings"])
            assert np.array_equal(got["simp_verts"][b, :len(w["verts"])], w["verts"])


# ------------------------------------------------------------------------------------------------ the Python layer

pipe = tco.pipe          # the tiny-config engine, once for this module


def _host_equals(c, want):
    """A [B, ..] result's simplified tables against the reference's."""
    s = c["simplified"]
    for b, w in enumerate(want):
        assert s["n"][b].tolist() == w["n"].tolist()
        assert np.array_equal(s["rings"][b, :len(w["rings"])].cpu().numpy(), w["rings"])
        assert np.array_equal(s["verts"][b, :len(w["verts"])].cpu().numpy(), w["verts"])


def test_object_contours_with_a_tolerance(ops):
    from diffews_amd.objects import (ContourBuffers, contours_to_host, fill_holes, label_objects, object_contours, rings_to_coco,
                                     rings_to_geojson)
    H, W = 60, 75
    rs = np.random.RandomState(17)
    lab = np.stack([cc.blobs(H, W, rs, n=20), cc.blobs(H, W, rs, n=12)])
    o = label_objects(torch.from_numpy(lab).cuda(), connectivity=8, max_components=32)
    plain = object_contours(o)
    assert sorted(plain) == ["connectivity", "n", "ring_off", "rings", "shape", "verts"]                # today's keys
    for src in (o, fill_holes(o, max_area=None, connectivity=8)):
        c = object_contours(src, tolerance=1.0)
        s = c["simplified"]
        assert sorted(s) == ["connectivity", "n", "ring_off", "rings", "shape", "tolerance", "verts"]
        assert s["tolerance"] == 1.0 and s["shape"] == (H, W) and s["ring_off"] is c["ring_off"] and s["verts"].shape == c["verts"].shape
        ids = src["ids"].cpu().numpy()
        base = ct.expected(ids, 32, 8, c["verts"].shape[1])
        _host_equals(c, sr.expected(ids, 32, 8, 0, 4, base=base))
        host, incomplete = contours_to_host(s)
        full, _ = contours_to_host(c)
        assert not incomplete and [len(h) for h in host] == [len(h) for h in full]
        for b in range(2):
            for k, rings in enumerate(host[b], 1):
                assert [a for a, _ in rings] == [a for a, _ in full[b][k - 1]] and sum(a for a, _ in rings) == (ids[b] == k).sum()
                g = rings_to_geojson(rings)
                assert all(r[0] == r[-1] and len(r) >= 4 for r in g["coordinates"])
                assert len(rings_to_coco(rings)) >= 6
    # [H, W], a list, and reused buffers that alias the result
    one = object_contours(o["ids"][1], max_components=32, tolerance=0.5, max_edges=2048)
    want = sr.expected(o["ids"][1:].cpu().numpy(), 32, 8, 2048, 2)[0]
    assert one["simplified"]["n"].tolist() == want["n"].tolist() and one["simplified"]["verts"].shape == (2048, 2)
    assert np.array_equal(one["simplified"]["verts"][:len(want["verts"])].cpu().numpy(), want["verts"])
    many = object_contours([o["ids"][0], o["ids"][1, :50, :60].contiguous()], max_components=32, tolerance=2)
    assert many["simplified"]["tolerance"] == [2, 2] and many["simplified"]["shape"] == [(H, W), (50, 60)]
    want = sr.expected(o["ids"][1:, :50, :60].cpu().numpy(), 32, 8, 4096, 8)[0]
    assert many["simplified"]["n"][1].tolist() == want["n"].tolist()
    assert np.array_equal(many["simplified"]["verts"][1][:len(want["verts"])].cpu().numpy(), want["verts"])
    hosts, incomplete = contours_to_host(many["simplified"])
    assert not incomplete and len(hosts) == 2 and contours_to_host(many)[1] is False
    bufs = ContourBuffers(2, H, W, 32, simplify=True)
    r = object_contours(o, buffers=bufs, tolerance=1)
    assert r["simplified"]["verts"].data_ptr() == bufs.simp_verts.data_ptr() and r["simplified"]["n"].data_ptr() == bufs.simp_n.data_ptr()
    assert r["simplified"]["rings"].data_ptr() == bufs.simp_rings.data_ptr() and r["verts"].data_ptr() == bufs.verts.data_ptr()
    again = object_contours(o, buffers=bufs)                                       # the same buffers without the stage
    assert "simplified" not in again and torch.equal(again["verts"][0, :5], plain["verts"][0, :5])
    with pytest.raises(ValueError, match="simplify=True"):
        object_contours(o, buffers=ContourBuffers(2, H, W, 32), tolerance=1)


def test_pipe_object_contours_agrees_with_objects(pipe):
    from diffews_amd.objects import object_contours
    from test_support_bank_gpu import _queries, _support_set
    sets = [_support_set(s, 64, seed=910 + 10 * c) for c, s in enumerate((1, 3, 2))]
    library = pipe.prepare_support_classes([a.cuda() for a, _ in sets], [m.cuda() for _, m in sets])
    r = pipe.segment_classes(library, _queries(2, 64, 77).cuda(), captured=False)
    o = pipe.objects(r, connectivity=8, max_components=256)
    a, b = pipe.object_contours(o, max_edges=8192, tolerance=1.0), object_contours(o, max_edges=8192, tolerance=1.0)
    ids = o["ids"].cpu().numpy()
    want = sr.expected(ids, 256, 8, 8192, 4)
    for x in (a, b):
        _host_equals(x, want)
    assert torch.equal(a["simplified"]["n"], b["simplified"]["n"]) and a["simplified"]["tolerance"] == 1.0

