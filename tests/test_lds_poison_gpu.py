"""LDS poison on the device (tests/lds_poison.py): proof that the method works, then the integer stages under it.

Proof: one `fill` reaches every CU (a condition: GRID_MULTIPLE and STAY_TICKS are what it takes on an idle card); what a
`fill` wrote is still there for the next kernel of the stream (measured in profiles/lds_poison.md, the floor asserted here
is half the measured minimum because the cards are shared); three planted defects -- `0 x` a word never written, a
histogram never zeroed, staging rows skipped at a ragged edge and summed anyway -- are right on zeroed LDS and are reported
by launch_guard.check_launches with their entry point's name under the poison, the first one under 0xFF only.

The integer stages (seg_*, tiles_*, the input transforms) allocate nothing through torch and run under 0xA5 harnesses of
their own, so check_launches does not reach them.  Here each runs four times on the smallest cases of its own test module
that have a partial last block and an odd width -- plain, then with every CU's LDS filled with 0xFF, 0x7B and 0x00 in front
of the call -- through that module's own launch helper (its memory guards are checked as always); every output must be
byte-equal to the plain run and equal to the stage's exact reference.  CASES_DECLARED lists the entry points that have such a
case; tests/test_lds_poison_cpu.py holds it against the header.
"""
import functools

import numpy as np
import pytest
import torch

import launch_guard as lg
import lds_poison as lp

pytestmark = pytest.mark.gpu

# Persistence floor: half of the smallest share of probe workgroups that found ALL of their 40960 words unchanged, over ten
# fill -> probe repetitions per pattern on an MI355X (profiles/lds_poison.md).
PERSISTENCE_FLOOR = 0.5


@pytest.fixture(scope="module")
def poisoner(hip_lib):
    return lp.handle()


# ------------------------------------------------------------------------------------------------ the method

def test_one_fill_reaches_every_cu(poisoner):
    grid = lp.GRID_MULTIPLE * lp.cu_count()
    where = torch.full((grid, 2), -1, dtype=torch.int32, device="cuda")
    lp.fill(lp.word_of(0x7B), where=where)
    torch.cuda.synchronize()
    assert int((where[:, 1] == -1).sum()) == 0, "a workgroup did not record where it ran"
    cus = lp.cus_of(where)
    print(f"fill: {grid} workgroups on {len(cus)} distinct CUs of {lp.cu_count()}, {len({x for x, _ in cus})} XCCs "
          f"(GRID_MULTIPLE {lp.GRID_MULTIPLE}, STAY_TICKS {lp.STAY_TICKS})")
    assert len(cus) == lp.cu_count(), (len(cus), lp.cu_count())


def persistence_share(pattern):
    """fill(P) then probe(P) on one stream: the share of probe workgroups whose whole LDS still holds P, and the CUs probed."""
    word = lp.word_of(pattern)
    lp.fill(word)
    counts, where = lp.probe(word)
    torch.cuda.synchronize()
    return float((counts == lp.LDS_WORDS).double().mean()), len(lp.cus_of(where))


@pytest.mark.parametrize("pattern", lp.PATTERNS, ids=["0xFF", "0x7B"])
def test_a_fill_is_still_there_for_the_next_kernel(poisoner, pattern):
    share, cus = persistence_share(pattern)
    print(f"pattern 0x{pattern:02X}: {share:.4f} of the probe workgroups ({cus} CUs) found all {lp.LDS_WORDS} words; floor {PERSISTENCE_FLOOR}")
    assert share >= PERSISTENCE_FLOOR, (share, PERSISTENCE_FLOOR)
    other = lp.word_of(0x00)
    lp.fill(other)
    counts, _ = lp.probe(lp.word_of(pattern))
    torch.cuda.synchronize()
    assert int(counts.sum()) == 0, "the probe counts words that are not the pattern"


def _planted(poisoner, name):
    """(call(run) for check_launches, the exact result on zeroed LDS) of one planted defect."""
    from diffews_amd import _lib as L
    g = torch.Generator().manual_seed(5)
    if name == "lds_planted_zero_times":
        x = torch.randn(200, generator=g).cuda()
        want, out, n = 2.0 * x, (200,), 200
    elif name == "lds_planted_histogram":
        x = torch.randint(0, 256, (1000,), generator=g, dtype=torch.uint8).cuda()
        want, out, n = torch.bincount((x & 15).long(), minlength=16).to(torch.int32), (16,), 1000
    else:
        x = torch.randn(16, 64, generator=g).cuda()
        rows = 11
        want, out, n = torch.zeros(64, device="cuda"), (64,), rows
        for r in range(rows):                       # the kernel's order of additions
            want = want + x[r]

    def call(run):
        plain = run.pattern is None
        if plain:
            lp.fill(0)                              # the plain launch is the one on zeroed LDS
        fn = getattr(poisoner if plain else L.lib(), name)
        px, y = run.place(x), run.empty(*out, dtype=want.dtype, device="cuda")
        assert fn(px.data_ptr(), y.data_ptr(), n, torch.cuda.current_stream().cuda_stream) == 0
        return y

    return call, want


@pytest.mark.parametrize("name", lp.PLANTED)
def test_planted_defects_pass_on_zeroed_lds_and_are_reported_under_the_poison(poisoner, name):
    call, want = _planted(poisoner, name)
    got = call(lg.Plain())
    torch.cuda.synchronize()
    assert torch.equal(got, want), name
    lds = functools.partial(lp.installed, real=poisoner, names=lp.PLANTED)
    lg.check_launches([], call, patterns=(0x00,), lds=lds)                  # zeroed LDS: bit-equal
    for pattern in lp.PATTERNS:
        if name == "lds_planted_zero_times" and pattern == 0x7B:
            lg.check_launches([], call, patterns=(pattern,), lds=lds)       # 0 x (large, finite) = 0: invisible
            continue
        with pytest.raises(lg.GuardError, match=rf"LDS pattern 0x{pattern:02X} .* in front of {name}\): result 0 .* reads LDS it has not written"):
            lg.check_launches([], call, patterns=(pattern,), lds=lds)
    with pytest.raises(lg.GuardError, match=rf"LDS pattern 0xFF .*{name}"):
        lg.check_launches([], call, lds=lds)                                # the default: both patterns


def test_a_memory_fault_is_not_blamed_on_lds(hip_lib):
    """An accumulate target nobody initialised differs under the memory pattern whatever LDS holds: the message says so."""
    from diffews_amd import ops_bwd as ob
    x = torch.randn(64, 24, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()

    def stale(run):
        return ob.colsum(run.place(x), out=run.empty(1, 24, dtype=torch.float32, device="cuda"), accumulate=True)

    with pytest.raises(lg.GuardError, match=r"pattern 0xFF \(in memory and in LDS; the difference stays with LDS zero-filled.*allocated by stale"):
        lg.check_launches([ob], stale)


# ------------------------------------------------------------------------------------------------ the integer stages

import ctypes as C

import boundary_ref as br
import cand_native_ref as cn
import components_ref as cr
import contours_cases as cc
import contours_ref as ct
import holes_ref as hr
import match_ref as mr
import native_ref as nr
import nway_native_ref as nn
import query_loader_ref as qr
import rle_ref as rr
import scores_ref as sr
import tiles_cand_ref as tcr
import tiles_ref as tr
import test_candidates_native_gpu as tcn
import test_components_gpu as tc
import test_input_route_gpu as tir
import test_nway_native_gpu as tnn
import test_object_boundaries_gpu as tb
import test_object_contours_gpu as tco
import test_object_holes_gpu as th
import test_object_match_gpu as tm
import test_object_runs_gpu as tru
import test_object_scores_gpu as ts
import test_query_loader_gpu as tq
import test_tiled_candidates_gpu as ttc
import test_tiled_gpu as tt

LDS_RUNS = (0xFF, 0x7B, 0x00)
CASES_DECLARED = set()


def E(name):
    """An entry point the cases below launch under the poison."""
    CASES_DECLARED.add(name)
    return name


E_COMPONENTS, E_HOLES, E_RLE, E_CONTOURS = E("dfw_seg_components"), E("dfw_seg_holes"), E("dfw_seg_rle"), E("dfw_seg_contours")
E_MATCH, E_SCORES = E("dfw_seg_match"), E("dfw_seg_scores")
E_BOUNDARY, E_BOUNDARY_COUNTS = E("dfw_seg_boundary"), E("dfw_seg_boundary_counts")
E_NATIVE, E_LABELS_NATIVE, E_CAND_NATIVE = E("dfw_seg_native"), E("dfw_seg_labels_native"), E("dfw_seg_labels_cand_native")
E_CUT, E_MERGE, E_TILES_CAND = E("dfw_tiles_cut"), E("dfw_tiles_merge"), E("dfw_tiles_labels_cand")
E_INPUTS, E_IMAGE, E_MASK = E("dfw_inputs_to_tensor"), E("dfw_image_to_tensor"), E("dfw_mask_to_tensor")


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


def _pair(fn):
    a, b = C.c_int32(), C.c_int32()
    assert fn(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _arrays(out):
    """Every array of what a launch helper returned, in a fixed order, on the host."""
    if isinstance(out, torch.Tensor):
        return [out.detach().cpu().contiguous().numpy()]
    if isinstance(out, np.ndarray):
        return [out]
    if isinstance(out, dict):
        return [a for k in sorted(out) for a in _arrays(out[k])]
    if isinstance(out, (list, tuple)):
        return [a for o in out for a in _arrays(o)]
    return []


def four_runs(entry, launch, check, what):
    """launch() plain, then with every CU's LDS filled with 0xFF, 0x7B and 0x00 in front of `entry`: the arrays it returns
    are byte-equal to the plain run's, and check(plain result) holds them against the stage's reference."""
    raw = launch()
    torch.cuda.synchronize()
    plain = _arrays(raw)
    assert plain, what
    for pattern in LDS_RUNS:
        with lp.installed(pattern) as proxy:
            got = launch()
            torch.cuda.synchronize()
        assert entry in proxy.poisoned, (what, entry, sorted(proxy.poisoned))
        got = _arrays(got)
        assert len(got) == len(plain), what
        for i, (a, b) in enumerate(zip(got, plain)):
            assert a.dtype == b.dtype and a.shape == b.shape, (what, f"LDS 0x{pattern:02X}", i)
            if a.tobytes() != b.tobytes():
                ne = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
                raise AssertionError(f"{what}: with LDS filled with 0x{pattern:02X} in front of {entry}, output {i} {a.shape} differs "
                                     f"from the plain run in {ne.size} element(s), first at {int(ne[0])}, last at {int(ne[-1])}")
    check(raw)


def _ids_of(labels, conn):
    """The ids dfw_seg_components gives, from the flood fill (no filter, a cap above every id)."""
    return np.ascontiguousarray(cr.components(labels, conn, 0, labels[0].size + 1)["ids"])


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("plus", (0, 1), ids=["tile", "tile+row+column"])
def test_seg_components(ops, hip_lib, plus, conn):
    tH, tW = _pair(hip_lib.dfw_seg_components_tile)
    H, W = tH + plus, tW + plus
    rs = np.random.RandomState(H * W + conn)
    c = tc._contents(H, W, rs)
    labels, gt = np.stack([c["noise 0.5"], c["snake"]]), tc._gt((2, H, W), rs)
    want = cr.components(labels, conn, 2, 16, gt, tc.NLAB)
    four_runs(E_COMPONENTS, lambda: tc._launch(ops, labels, conn, 2, 16, gt, pad=61)[0],
              lambda got: tc._same(got, want, (H, W, conn)), ("seg_components", H, W, conn))


@pytest.mark.parametrize("conn", (4, 8))
def test_seg_holes(ops, hip_lib, conn):
    """Holes inside a tile, across x = 63 | 64, across y = 31 | 32 and over the four-tile corner, on a width with W % 4 == 1."""
    H, W = 70, 141
    assert W % 4 != 0 and _pair(hip_lib.dfw_seg_components_tile) == (32, 64)       # th.BORDER_BOXES is written for this tile
    rs = np.random.RandomState(conn)
    labs = np.stack([th._holes_at(H, W, list(th.BORDER_BOXES.values())), th._noise(H, W, 0.85, rs)])
    comp = cr.components(labs, conn, 0, 2048)
    gt = th._gt(labs.shape, rs)
    want = hr.holes(comp["filtered"], comp["ids"], conn, 50, comp["stats"], gt, th.NLAB)
    assert want["holes"][0].tolist() == [4, 4] and want["holes"][1, 0] > 0
    four_runs(E_HOLES, lambda: th._launch(ops, comp["filtered"], comp["ids"], conn, 50, comp["stats"], gt, off=1)[0],
              lambda got: th._same(got, want, ("holes", conn)), ("seg_holes", conn))


@pytest.mark.parametrize("order", rr.ORDERS)
def test_seg_rle(ops, hip_lib, order):
    P, _ = _pair(hip_lib.dfw_seg_rle_block)
    H, W = 3, (P + 1) // 3
    assert H * W == P + 1 and W % 2 == 1
    rs = np.random.RandomState(W)
    c = rr.contents(H, W, rs)
    ids = _ids_of(np.stack([c["noise 0.5"], c["checkerboard"]]), 8)
    cap = int(ids.max()) + 3
    want = rr.rle(ids, cap, H * W, order)
    four_runs(E_RLE, lambda: tru._launch(ops, ids, cap, H * W, order, pad=61, ws_pad=60)[0],
              lambda got: tru._same(got, want, ("rle", order)), ("seg_rle", order))


@pytest.mark.parametrize("conn", (4, 8))
def test_seg_contours(ops, hip_lib, conn):
    """A block of pixels plus one; max_edges is the count found rounded up to 4, which is more than one block of edges."""
    P, Eb = cc.block(hip_lib)
    H, W = 3, (P + 1) // 3
    assert H * W == P + 1 and W % 2 == 1
    rs = np.random.RandomState(W + conn)
    c = rr.contents(H, W, rs)
    ids = _ids_of(np.stack([c["noise 0.5"], c["noise 0.3"]]), conn)
    cap = int(ids.max()) + 3
    want = ct.expected(ids, cap, conn, 1 << 30)
    found = max(int(w["n"][0]) for w in want)
    assert found > Eb, (found, Eb)
    Emax = max(4, cc.up4(found))
    four_runs(E_CONTOURS, lambda: tco._launch(ops, ids, cap, Emax, conn, pad=61)[0],
              lambda got: tco._same(got, want, ("contours", conn)), ("seg_contours", conn))


@pytest.mark.parametrize("cap", (15, 255), ids=["1 table pass", "2 table passes"])
def test_seg_match(ops, hip_lib, cap):
    """More records than one chunk holds, cut at one chunk plus one record; ids up to the cap and above it."""
    P, R = _pair(hip_lib.dfw_seg_match_block)
    H, W = 37, R // 37 + 25
    rs = np.random.RandomState(cap)
    pids = rs.randint(0, cap + 2, (2, H, W)).astype(np.int32)
    gids = rs.randint(0, cap + 2, (2, H, W)).astype(np.int32)
    M = R + 1
    want = mr.match(pids, gids, cap, cap, 1, M, 100)
    assert (want["n"][:, 2] == M).all() and want["n"][:, 3].min() > M, want["n"].tolist()      # kept M of the records found
    four_runs(E_MATCH, lambda: tm._launch(ops, pids, gids, cap, cap, 1, M, 100, odd=True)[0],
              lambda got: tm._same(got, want, ("match", cap)), ("seg_match", cap))


@pytest.mark.parametrize("which", (5, 6), ids=["block+1", "3-blocks-odd-W"])
def test_seg_scores(ops, which):
    P = ops.seg_scores_block()
    H, W = ts._shapes(P)[which]
    assert W % 2 == 1 and H * W > P
    rs = np.random.RandomState(1000 * H + W)
    lab = ts._three(rr.contents(H, W, rs)["noise 0.5"])[None]
    ids = _ids_of(lab, 8)
    cap = int(ids.max()) + 3
    u8 = rs.randint(0, 256, (3, 1, 3, H, W)).astype(np.uint8)
    table = ts._class_table(3, 1)
    want = sr.scores(ids, lab, u8.reshape(-1, 3, H, W), table, cap)

    def check(got):
        assert np.array_equal(got, want), int((got != want).sum())

    four_runs(E_SCORES, lambda: ts._launch(ops, ids, lab, u8, table, cap, id_pad=61, byte_pad=3, ws_pad=60)[0], check, ("seg_scores", H, W))


def _boundary_shapes(ops):
    R, Cc, _ = ops.seg_boundary_block()
    return {"tile+row": (R + 1, Cc), "tile+column": (R, Cc + 1)}


@pytest.mark.parametrize("dtype", (np.uint8, np.int32), ids=["uint8", "int32"])
@pytest.mark.parametrize("dmax", (1, 7))
@pytest.mark.parametrize("shape", ("tile+row", "tile+column"))
def test_seg_boundary(ops, shape, dmax, dtype):
    H, W = _boundary_shapes(ops)[shape]
    rs = np.random.RandomState(H * 1000 + W)
    m = np.stack([mr.blobs(H, W, rs), rr.contents(H, W, rs)["rings"]]).astype(dtype)
    want = br.dist_ref(m, dmax)
    band = br.band_ref(m, want, dmax)

    def check(got):
        assert np.array_equal(got[0], want) and got[1].dtype == m.dtype and np.array_equal(got[1], band)

    four_runs(E_BOUNDARY, lambda: tb._launch(ops, m, dmax, dmax, off=True), check, ("seg_boundary", shape, dmax, str(m.dtype)))


@pytest.mark.parametrize("d", (1, 7))
@pytest.mark.parametrize("shape", ("tile+row", "tile+column"))
def test_seg_boundary_counts(ops, shape, d):
    H, W = _boundary_shapes(ops)[shape]
    rs = np.random.RandomState(H * 1000 + W + d)
    pred = np.stack([mr.blobs(H, W, rs, nlabels=5), mr.blobs(H, W, rs, nlabels=5)])
    gt = mr.perturb(pred, rs)
    pdist, gdist = br.dist_ref(pred, 7), br.dist_ref(gt, 7)
    want = br.counts_ref(pred, pdist, gt, gdist, d, 3)
    assert want[:, 0, 1:].sum() > 0

    def check(got):
        assert np.array_equal(got, want)

    four_runs(E_BOUNDARY_COUNTS, lambda: tb._counts(ops, pred, pdist, gt, gdist, d, 3, off=True), check, ("seg_boundary_counts", shape, d))


# ---- the native-size routes: the two-image batch of tests/test_nway_native_gpu.py (40 x 72 -> 41 x 50 and 23 x 37)

NATIVE_SRC, NATIVE_SIZES = tnn.SOURCES[1], list(tnn.PAIR)
PAD = 256


class _NativeBuffers:
    """tmp, out_u8 and labels / pred of a native-size call, K strides each where the route has a class or entry dimension,
    filled with 0xA5 with PAD bytes around and the targets' 64 guard bytes after every image."""

    def __init__(self, t, K, Hs):
        n = dict(tmp=K * t.tmp_bytes, u8=K * t.u8_bytes, labels=t.pred_bytes)
        self.bufs = {k: torch.full((v + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda") for k, v in n.items()}
        self.view = {k: self.bufs[k][PAD:PAD + v] for k, v in n.items()}
        self.regions = dict(tmp=[(PAD + k * t.tmp_bytes + it.tmp_off, 3 * Hs * it.w) for k in range(K) for it in t.items],
                            u8=[(PAD + k * t.u8_bytes + it.u8_off, 3 * it.h * it.w) for k in range(K) for it in t.items],
                            labels=[(PAD + it.pred_off, it.h * it.w) for it in t.items])

    def check(self):
        torch.cuda.synchronize()
        for k, b in self.bufs.items():
            assert tq._untouched(b, self.regions[k]), f"wrote outside {k}"


def _masks(sizes, seed):
    rs = np.random.RandomState(seed)
    out = []
    for h, w in sizes:
        m = (rs.rand(h, w) > 0.5).astype(np.uint8)
        m[rs.rand(h, w) < 0.07] = 255
        out.append(m)
    return out


def test_seg_native(ops):
    from diffews_amd.input_pipeline import NativeTargets
    x = tnn._input(1, NATIVE_SRC, tuple(NATIVE_SIZES))[0]
    xd, gts = x.cuda(), _masks(NATIVE_SIZES, 5)
    t = NativeTargets(NATIVE_SRC, NATIVE_SIZES, gt=gts, class_value=1, ignore_value=255, guard=64)
    ref = nr.native_ref(x, NATIVE_SIZES, gts, 1, 255, 0.25, 0.0, False)

    def launch():
        nb = _NativeBuffers(t, 1, NATIVE_SRC[0])
        r = ops.seg_native(xd, t, 0.25, 0.0, False, u8_out=nb.view["u8"], pred_out=nb.view["labels"], tmp=nb.view["tmp"])
        nb.check()
        return dict(r=r, u8=nb.bufs["u8"], pred=nb.bufs["labels"])

    def check(got):
        r = got["r"]
        for i, (h, w) in enumerate(NATIVE_SIZES):
            assert torch.equal(r["seg_u8"][i].cpu(), nr.resize_u8(x[i], h, w)) and torch.equal(r["pred"][i].cpu(), ref["pred"][i]), i
        assert torch.equal(r["counts"].cpu(), ref["counts"])

    four_runs(E_NATIVE, launch, check, "seg_native")


def test_seg_labels_native(ops):
    from diffews_amd.input_pipeline import NativeTargets
    N = 3
    x = tnn._input(N, NATIVE_SRC, tuple(NATIVE_SIZES))
    xd, gts = x.cuda(), tnn._gts(N, NATIVE_SIZES, "labels")
    t = NativeTargets(NATIVE_SRC, NATIVE_SIZES, gt=gts, ignore_value=255, guard=64)
    res = tnn._resized(N, NATIVE_SRC, tuple(NATIVE_SIZES))
    ref = nn.nway_native_ref(x, NATIVE_SIZES, gts, None, 255, 0.25, 0.0, False, res=res)

    def launch():
        nb = _NativeBuffers(t, N, NATIVE_SRC[0])
        r = ops.seg_labels_native(xd, t, 0.25, 0.0, False, want_u8=True, labels_out=nb.view["labels"], u8_out=nb.view["u8"], tmp=nb.view["tmp"])
        nb.check()
        return dict(r=r, u8=nb.bufs["u8"], labels=nb.bufs["labels"])

    def check(got):
        tnn._same(got["r"], ref, "seg_labels_native")
        for i in range(len(NATIVE_SIZES)):
            assert torch.equal(got["r"]["seg_u8"][i].cpu(), torch.stack([res[c][i] for c in range(N)])), i

    four_runs(E_LABELS_NATIVE, launch, check, "seg_labels_native")


def test_seg_labels_cand_native(ops):
    """The first two queries of the discriminating input of tests/cand_native_ref.py: lists (0, 2) and (), 41 x 50 and 23 x 37."""
    off, sizes = cn.DISC_OFF[:3], cn.DISC_SIZES[:2]
    assert off == [0, 2, 2]
    x = cn.discriminating_input()[:2].contiguous()
    lab, nlabels, _ = cn.disc_tables("set")
    lab, gts = lab[:2], cn.disc_gts("labels")[:2]
    want = cn.cand_native_ref(x, off, lab, nlabels, sizes, gts, ignore_value=cn.DISC_IGNORE, r_threshold=0.25)
    t = tcn._targets(sizes, gts, guard=64)
    tab = tcn._tab(off, lab)
    xd, tabd = x.cuda(), tab.cuda()

    def launch():
        nb = _NativeBuffers(t, 2, cn.DISC_SRC[0])
        r = ops.seg_labels_cand_native(xd, t, tabd, tab, nlabels, want_area=True, want_u8=True, r_threshold=0.25,
                                       labels_out=nb.view["labels"], u8_out=nb.view["u8"], tmp=nb.view["tmp"])
        nb.check()
        return dict(r=r, u8=nb.bufs["u8"], labels=nb.bufs["labels"])

    def check(got):
        tcn._same(got["r"], want)
        for p, w in zip(got["r"]["seg_u8"], want["seg_u8"]):
            assert torch.equal(p.cpu(), torch.from_numpy(w))

    four_runs(E_CAND_NATIVE, launch, check, "seg_labels_cand_native")


# ---- tiles

@pytest.mark.parametrize("tile,hw,ov", tt.CUT_CASES[:3], ids=[f"{t[0]}x{t[1]}-on-{s[0]}x{s[1]}" for t, s, _ in tt.CUT_CASES[:3]])
def test_tiles_cut(ops, tile, hw, ov):
    from diffews_amd.input_pipeline import DeviceImageTransform
    img = np.random.RandomState(hw[1]).randint(0, 256, hw + (3,)).astype(np.uint8)
    p, tf = tt._plan(hw, tile, ov), DeviceImageTransform(tile)
    dev, lut = torch.from_numpy(img).cuda(), tf.lut.cpu().numpy()
    per = 3 * tile[0] * tile[1]

    def launch():
        flat = torch.full(((p.T + 2) * per + 1,), 777.0, device="cuda")           # one float in front: not 16-byte aligned
        ops.tiles_cut(p, dev, tf.lut, out=flat[1 + per:1 + (p.T + 1) * per].view(p.T, 3, *tile))
        torch.cuda.synchronize()
        assert (flat[:1 + per] == 777.0).all() and (flat[1 + (p.T + 1) * per:] == 777.0).all(), "tiles_cut wrote outside out"
        return flat

    def check(flat):
        got = flat[1 + per:1 + (p.T + 1) * per].view(p.T, 3, *tile).cpu()
        for t, (y, x) in enumerate(tr.windows(p.ys, p.xs)):
            assert torch.equal(got[t], torch.from_numpy(lut[img[y:y + tile[0], x:x + tile[1]]].transpose(2, 0, 1).copy())), t

    four_runs(E_CUT, launch, check, ("tiles_cut", tile, hw))


@pytest.mark.parametrize("tile,hw,ov", tt.MERGE_CASES[:5], ids=tt.IDS[:5])
def test_tiles_merge(ops, tile, hw, ov):
    rs = np.random.RandomState(hw[0] * 1000 + hw[1])
    p = tt._plan(hw, tile, ov, ov)
    win = rs.randint(0, 256, (3, p.T, 3) + tile).astype(np.uint8)
    want, want_mx = tr.merge(win, hw, p.ys, p.xs, ov)
    wd = torch.from_numpy(win).cuda()

    def check(got):
        assert torch.equal(got[0], torch.from_numpy(want)) and got[1].tolist() == want_mx.tolist()

    four_runs(E_MERGE, lambda: tt._merge_guarded(ops, p, wd, 61), check, ("tiles_merge", tile, hw))


def _twenty_windows():
    """The hand-made plan of test_more_windows_over_a_pixel_than_one_table_chunk_holds: 8 x 8 windows one pixel apart on
    12 x 11, N = 254 -- cells with 20 windows need more table words than one chunk of the kernel's LDS table holds, so the
    table is rebuilt per pixel step."""
    from diffews_amd import _lib as L
    tile, hw, N = (8, 8), (12, 11), 254
    ys, xs = [0, 1, 2, 3, 4], [0, 1, 2, 3]
    c = L.TilePlan()
    c.img_h, c.img_w, c.tile_h, c.tile_w, c.ny, c.nx, c.ramp = 12, 11, 8, 8, 5, 4, 3
    c.ys[:5], c.xs[:4] = ys, xs
    rs = np.random.RandomState(20)
    lists = [sorted(rs.choice(N, 12, replace=False).tolist()) for _ in range(20)]
    lists[7] = []
    lists[3] = sorted(set(lists[3]) | {0, 253})
    off = np.cumsum([0] + [len(l) for l in lists])
    tab = torch.tensor(off.tolist() + [v for l in lists for v in l], dtype=torch.int32)
    ent = rs.randint(0, 256, (int(off[-1]), 3) + tile).astype(np.uint8)
    return c, ent, tab, N, ttc._gt(hw, N, rs), hw, ys, xs, 3


def _small_plan():
    tile, hw, ov = ttc.CASES[3]
    assert tile[0] != tile[1]
    N = 3
    rs = np.random.RandomState(hw[0] * 1000 + hw[1])
    p = ttc._plan(hw, tile, ov, ov)
    lists, _ = ttc._random_lists(p.T, N, rs)
    tab = p.candidate_table(lists, N)
    ent = rs.randint(0, 256, (tab["E"], 3) + tile).astype(np.uint8)
    return p, ent, tab["tab"], N, ttc._gt(hw, N, rs), hw, p.ys, p.xs, ov


@pytest.mark.parametrize("case", (_twenty_windows, _small_plan), ids=["12x11-20-windows-N254", "8x16-on-19x37-gt-area"])
def test_tiles_labels_cand(ops, case):
    plan, ent, tab, N, gt, hw, ys, xs, ramp = case()
    want = tcr.labels_cand(ent, tab, N, hw, ys, xs, ramp, gt, r_threshold=0.25, threshold=0.0)
    assert (want[0] > 0).any()
    four_runs(E_TILES_CAND, lambda: ttc._run_guarded(ops, plan, ent, tab, N, gt, 61, hw, r_threshold=0.25, threshold=0.0, want_area=True),
              lambda got: ttc._check(got, want, case.__name__), ("tiles_labels_cand", case.__name__))


# ---- the input transforms

def test_inputs_to_tensor(hip_lib):
    """Two small images and two class-id maps (9 x 13 and 20 x 7 -> 32 x 32) in one call, 0xA5 around every item."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    out_hw = (32, 32)
    src = tir._small_sources(2, seed=3)
    images, masks, cls = [s[0] for s in src], [s[1] for s in src], [1, 2]
    tf = DeviceImageTransform(out_hw)
    plan = DeviceImageTransform(out_hw, device=None).batch(images, masks, cls, True, True, guard=64)
    oh, ow = out_hw

    def launch():
        bufs = {k: tq._fill(getattr(plan, k + "_bytes")) for k in ("tmp", "dst", "pm1", "bin")}
        r = tf.batch(images, masks, cls, True, True, guard=64, buffers=bufs)
        torch.cuda.synchronize()
        lay = r["layout"]
        items, mitems = lay.img_items[:lay.n_img], lay.mask_items[:lay.n_mask]
        regions = dict(tmp=[(it.tmp_off, 3 * it.H * ow) for it in items], dst=[(it.dst_off, 12 * oh * ow) for it in items],
                       pm1=[(it.pm1_off, 12 * oh * ow) for it in mitems], bin=[(it.bin_off, oh * ow) for it in mitems])
        for name, regs in regions.items():
            assert tq._untouched(bufs[name], regs), name
        return dict(images=r["images"], pm1=r["pm1"], bin=r["bin"], dst=bufs["dst"], pm1_buf=bufs["pm1"], bin_buf=bufs["bin"])

    def check(got):
        for i in range(2):
            ref = qr.host_mask(masks[i], cls[i], out_hw)
            assert torch.equal(got["images"][i].cpu(), qr.host_image(images[i], out_hw)), i
            assert torch.equal(got["bin"][i].cpu().float(), ref) and torch.equal(got["pm1"][i].cpu(), ref[None].repeat(3, 1, 1) * 2 - 1), i

    four_runs(E_INPUTS, launch, check, "inputs_to_tensor")


@pytest.mark.parametrize("i", (0, 1, 2), ids=["1x1", "2x3", "37x41"])
def test_image_and_mask_to_tensor(hip_lib, i):
    """The per-item entry points on the three smallest sources of tests/query_loader_ref.py (a uint8, an int32 and a uint8
    class-id map), 64 x 64 out."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    out_hw = qr.OUT_SIZES[0]
    d = qr.ragged(out_hw)
    lut = DeviceImageTransform(out_hw).lut
    im, m, value, ref = d["images"][i], d["masks"][i], d["mask_class"][i], d["ref_masks"][i]

    def check_image(got):
        assert torch.equal(got.cpu(), d["ref_images"][i])

    def check_mask(got):
        assert torch.equal(got[0].cpu(), ref[None].repeat(3, 1, 1) * 2 - 1) and torch.equal(got[1].cpu().float(), ref)

    four_runs(E_IMAGE, lambda: qr.per_item_image(im, out_hw, lut), check_image, ("image_to_tensor", im.shape))
    four_runs(E_MASK, lambda: qr.per_item_mask(m, value, out_hw, lut.device), check_mask, ("mask_to_tensor", m.shape, str(m.dtype)))


# ---- entry points no wrapper of the launch-guard cases reaches: their exact cases of tests/test_glue_exact_gpu.py

E_POSTPROCESS, E_METER, E_TO_F32 = E("dfw_seg_postprocess"), E("dfw_meter_update"), E("dfw_convert_to_f32")


def test_seg_postprocess_first_form(hip_lib):
    """dfw_seg_postprocess (the form without threshold / batch_max, which the package no longer calls) through ctypes, on the
    (3, 7, 9) case of test_seg_scalar_paths_caps_and_gt_forms: scalar loops, image bases at odd offsets, garbage in counts
    and scratch, a sentinel byte on either side of seg_u8."""
    import test_glue_exact_gpu as tg
    from diffews_amd import _lib as L
    B, H, W = 3, 7, 9
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(B * 1000 + H)) * 2.4 - 1.2
    gt = tg.gt_pattern((B, H, W))
    u8_ref = torch.from_numpy(tg.seg_u8_ref(x))
    xg, gg, n = x.cuda(), gt.cuda(), x.numel()

    def launch():
        ub = torch.full((n + 2,), 77, dtype=torch.uint8, device="cuda")
        counts = torch.full((B, 4), -12345678901, dtype=torch.int64, device="cuda")
        scratch = torch.full((B,), 0x7fffffff, dtype=torch.int32, device="cuda")
        L.check(L.lib().dfw_seg_postprocess(xg.data_ptr(), ub[1:].data_ptr(), gg.data_ptr(), counts.data_ptr(), scratch.data_ptr(),
                                            B, H, W, 0.25, torch.cuda.current_stream().cuda_stream), "dfw_seg_postprocess")
        return ub, counts

    def check(got):
        ub, counts = got
        assert int(ub[0]) == 77 and int(ub[-1]) == 77 and torch.equal(ub[1:n + 1].view(B, 3, H, W).cpu(), u8_ref)
        assert counts.cpu().tolist() == tg.seg_counts_ref(u8_ref, gt, r_threshold=0.25)

    four_runs(E_POSTPROCESS, launch, check, "seg_postprocess")


def test_meter_update(ops):
    """test_meter_update_exact's (37, 5): ids -1 and nclass ignored, repeated ids, B no multiple of 32."""
    B, nclass = 37, 5
    g = torch.Generator().manual_seed(B)
    counts = torch.randint((1 << 40) - 1000, (1 << 40) + 1000, (B, 4), generator=g, dtype=torch.int64)
    cls = torch.randint(-1, nclass + 1, (B,), generator=g, dtype=torch.int64)
    cls[0], cls[-1] = -1, nclass
    ib = torch.randint(0, 1 << 33, (2, nclass), generator=g, dtype=torch.int64)
    ub = torch.randint(0, 1 << 33, (2, nclass), generator=g, dtype=torch.int64)
    ok = (cls >= 0) & (cls < nclass)
    want_i = ib.clone().index_add_(1, cls[ok], counts[ok, 0:2].t().contiguous())
    want_u = ub.clone().index_add_(1, cls[ok], counts[ok, 2:4].t().contiguous())
    cg, kg = counts.cuda(), cls.cuda()

    def launch():
        ibg, ubg = ib.cuda(), ub.cuda()
        ops.meter_update(cg, kg, ibg, ubg)
        return ibg, ubg

    def check(got):
        assert torch.equal(got[0].cpu(), want_i) and torch.equal(got[1].cpu(), want_u)

    four_runs(E_METER, launch, check, "meter_update")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_to_f32(hip_lib, dtype):
    """test_storage_to_fp32_every_pattern's operand: all 65536 bit patterns of the storage dtype, scale 0.25."""
    import test_glue_exact_gpu as tg
    from diffews_amd import ops_bwd as ob
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    want = x.float() * torch.tensor(0.25, dtype=torch.float32)
    xg = x.cuda()

    def launch():
        out = torch.full((65536,), 5.0, dtype=torch.float32, device="cuda")
        ob.to_f32(xg, out, scale=0.25)
        return out

    four_runs(E_TO_F32, launch, lambda got: tg.assert_bits_equal(got, want, "to_f32"), ("to_f32", str(dtype)))
