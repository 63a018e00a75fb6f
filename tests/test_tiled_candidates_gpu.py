"""GPU tests of per-window candidate classes in tiled segmentation: ops.tiles_labels_cand against the host reference
(tests/tiles_cand_ref.py: the entries scattered into a zero window buffer, tiles_ref.merge, nway_ref.seg_labels) on random
bytes at the smallest shapes that reach every path of the kernel (one window, cells narrower than four pixels, three windows
over a pixel per axis, a non-square tile, several workgroups per cell, a table that needs more than one chunk of classes),
against the dense kernels on full lists, and pipe.segment_tiled(candidates=) / propose_tile_candidates /
evaluate.evaluate_tiled on the tiny engine.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import tiles_cand_ref as tcr
from test_support_bank_gpu import models, _support_set  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

# (tile, image, overlap): 8 x 8 on 13 x 13 with overlap 4 has origins [0, 2, 5]: three windows over a pixel per axis
CASES = [((8, 8), (8, 8), 2), ((8, 8), (13, 29), 2), ((8, 8), (13, 13), 4), ((8, 16), (19, 37), 3), ((64, 64), (88, 150), 8)]
IDS = [f"{t[0]}x{t[1]}-on-{s[0]}x{s[1]}" for t, s, _ in CASES]
SENT = 0xA5


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


def _plan(hw, tile, ov, ramp=None):
    from diffews_amd.input_pipeline import TilePlan
    return TilePlan(hw, tile, ov, ramp)


def _gt(hw, N, rs):
    """0..N, some 255 (ignore) and some values above N that have no bin."""
    g = rs.randint(0, N + 1, hw).astype(np.uint8)
    g[rs.rand(*hw) < 0.05] = 255
    g[rs.rand(*hw) < 0.05] = min(N + 3, 254)
    return g


def _random_lists(T, N, rs):
    """Random lists with at least one empty window (when T > 1) and, when N > 1, one class listed nowhere."""
    absent = rs.randint(0, N) if N > 1 else -1
    lists = [[c for c in range(N) if c != absent and rs.rand() < 0.6] for _ in range(T)]
    if T > 1:
        lists[rs.randint(0, T)] = []
    if not any(lists):
        lists[0] = [c for c in range(N) if c != absent][:1]
    return lists, absent


def _run_guarded(ops, plan, ent, tab_host, N, gt, guard, hw, **kw):
    """tiles_labels_cand into buffers with sentinels before and after labels, mx, counts and area; everything on the host."""
    h, w = hw
    flat = torch.full((h * w + 2 * guard,), SENT, dtype=torch.uint8, device="cuda")
    mxb = torch.full((N + 2,), -7, dtype=torch.int32, device="cuda")
    cb = torch.full((2 * (N + 1) + 2,), -7, dtype=torch.int64, device="cuda")
    ab = torch.full((2 * N + 2,), -7, dtype=torch.int64, device="cuda")
    lab, cnt, mx, area = ops.tiles_labels_cand(
        plan, None if ent is None else torch.from_numpy(ent).cuda(), tab_host.cuda(), tab_host, N,
        None if gt is None else torch.from_numpy(gt).cuda(), labels_out=flat[guard:guard + h * w].view(h, w),
        mx_out=mxb[1:N + 1], counts_out=None if gt is None else cb[1:-1].view(2, N + 1), area_out=ab[1:-1].view(N, 2), **kw)
    torch.cuda.synchronize()
    assert (flat[:guard] == SENT).all() and (flat[guard + h * w:] == SENT).all(), "wrote outside labels"
    assert mxb[0].item() == -7 and mxb[-1].item() == -7, "wrote outside mx"
    assert cb[0].item() == -7 and cb[-1].item() == -7, "wrote outside counts"
    assert ab[0].item() == -7 and ab[-1].item() == -7, "wrote outside area"
    if gt is None:
        assert cnt is None and (cb == -7).all()
    return lab.cpu(), None if cnt is None else cnt.cpu(), mx.cpu(), area.cpu()


def _check(got, want, what):
    lab, cnt, mx, area = got
    wlab, wcnt, wmx, warea = want
    assert torch.equal(lab, wlab), (what, int((lab != wlab).sum()))
    assert mx.tolist() == wmx.tolist(), what
    assert (cnt is None) == (wcnt is None) and (cnt is None or torch.equal(cnt, wcnt)), what
    assert torch.equal(area, warea), what


@pytest.mark.parametrize("tile,hw,ov", CASES, ids=IDS)
def test_labels_cand_equals_reference_on_random_bytes(ops, tile, hw, ov):
    rs = np.random.RandomState(hw[0] * 1000 + hw[1])
    for N in (1, 3, 7):
        for ramp in sorted({1, ov, min(tile) // 2}):
            p = _plan(hw, tile, ov, ramp)
            lists, absent = _random_lists(p.T, N, rs)
            ct = p.candidate_table(lists, N)
            ent = rs.randint(0, 256, (ct["E"], 3) + tile).astype(np.uint8)
            gt = _gt(hw, N, rs)
            for flags in (dict(r_threshold=0.25, threshold=0.0), dict(r_threshold=0.0, threshold=0.45)):
                want = tcr.labels_cand(ent, ct["tab"], N, hw, p.ys, p.xs, ramp, gt, **flags)
                if absent >= 0:
                    assert want[2][absent] == 0 and not (want[0] == absent + 1).any()
                for guard in (64, 61):            # 61: labels itself is not word-aligned
                    _check(_run_guarded(ops, p, ent, ct["tab"], N, gt, guard, hw, **flags), want, (tile, hw, N, ramp, flags, guard))
            got = _run_guarded(ops, p, ent, ct["tab"], N, None, 64, hw, **flags)      # without gt: no counts, the rest the same
            _check(got, (want[0], None, want[2], want[3]), (tile, hw, N, ramp, "no gt"))


@pytest.mark.parametrize("tile,hw,ov", CASES, ids=IDS)
def test_full_lists_equal_the_dense_kernels(ops, tile, hw, ov):
    """Every class listed in every window: labels, counts and mx are torch.equal to ops.tiles_merge + ops.seg_labels on the
    same bytes, class-major."""
    rs = np.random.RandomState(hw[1])
    for N in (1, 3, 7):
        p = _plan(hw, tile, ov)
        win = rs.randint(0, 256, (N, p.T, 3) + tile).astype(np.uint8)
        gt = torch.from_numpy(_gt(hw, N, rs)).cuda()
        ct = p.candidate_table([range(N)] * p.T, N)
        ent = torch.from_numpy(np.ascontiguousarray(win.transpose(1, 0, 2, 3, 4)).reshape(-1, 3, *tile)).cuda()
        for flags in (dict(r_threshold=0.25, threshold=0.0), dict(r_threshold=0.0, threshold=0.45)):
            merged, mx = ops.tiles_merge(p, torch.from_numpy(win).cuda())
            lab, cnt = ops.seg_labels(merged.view(N, 1, 3, *hw), mx, gt[None], **flags)
            got = ops.tiles_labels_cand(p, ent, ct["tab"].cuda(), ct["tab"], N, gt, **flags)
            assert torch.equal(got[0], lab[0]) and torch.equal(got[1], cnt[0]) and torch.equal(got[2], mx), (tile, hw, N, flags)
            assert got[3] is None


def test_254_classes_in_both_windows(ops):
    """8 x 8 on 8 x 9, both windows carry all 254 classes; class 200 is 255 everywhere in window 1 and nothing else reaches
    255: mx is 255 for that class only, and its area is the reference's."""
    tile, hw, N = (8, 8), (8, 9), 254
    p = _plan(hw, tile, 2)
    assert p.T == 2
    rs = np.random.RandomState(254)
    ct = p.candidate_table([range(N)] * 2, N)
    ent = rs.randint(0, 200, (2 * N, 3) + tile).astype(np.uint8)
    ent[N + 200] = 255
    gt = _gt(hw, N, rs)
    want = tcr.labels_cand(ent, ct["tab"], N, hw, p.ys, p.xs, p.ramp, gt)
    got = _run_guarded(ops, p, ent, ct["tab"], N, gt, 64, hw)
    _check(got, want, "N=254")
    assert got[2][200] == 255 and int((got[2] == 255).sum()) == 1
    assert got[3][200].tolist() == want[3][200].tolist() and got[3][200, 0] > 0


def test_more_windows_over_a_pixel_than_one_table_chunk_holds(ops):
    """A hand-made plan with five windows over a row and four over a column (origins one pixel apart) and N = 254: cells
    with 20 windows need 254 * 20 table words, more than one chunk of the kernel's LDS table, so the classes go through it
    in chunks.  Sparse lists, against the reference."""
    from diffews_amd import _lib as L
    tile, hw, N = (8, 8), (12, 11), 254
    ys, xs = [0, 1, 2, 3, 4], [0, 1, 2, 3]
    c = L.TilePlan()
    c.img_h, c.img_w, c.tile_h, c.tile_w, c.ny, c.nx, c.ramp = 12, 11, 8, 8, 5, 4, 3
    c.ys[:5], c.xs[:4] = ys, xs
    T = 20
    rs = np.random.RandomState(20)
    lists = [sorted(rs.choice(N, 12, replace=False).tolist()) for _ in range(T)]
    lists[7] = []
    lists[3] = sorted(set(lists[3]) | {0, 253})
    off = np.cumsum([0] + [len(l) for l in lists])
    tab = torch.tensor(off.tolist() + [v for l in lists for v in l], dtype=torch.int32)
    ent = rs.randint(0, 256, (int(off[-1]), 3) + tile).astype(np.uint8)
    gt = _gt(hw, N, rs)
    for flags in (dict(r_threshold=0.25, threshold=0.0), dict(r_threshold=0.0, threshold=0.2)):
        want = tcr.labels_cand(ent, tab, N, hw, ys, xs, 3, gt, **flags)
        assert (want[0] > 0).any()
        _check(_run_guarded(ops, c, ent, tab, N, gt, 61, hw, **flags), want, flags)


@pytest.mark.parametrize("tile,hw,ov", CASES[1:], ids=IDS[1:])
def test_one_bright_entry_ramps_toward_the_absent_neighbours(ops, tile, hw, ov):
    """The last window lists class 0 with all bytes 255, nothing else is listed anywhere: the reference for every ramp."""
    for ramp in sorted({1, ov, min(tile) // 2}):
        p = _plan(hw, tile, ov, ramp)
        lists = [[] for _ in range(p.T)]
        lists[-1] = [0]
        ct = p.candidate_table(lists, 2)
        ent = np.full((1, 3) + tile, 255, np.uint8)
        for flags in (dict(r_threshold=0.25, threshold=0.0), dict(r_threshold=0.0, threshold=0.5)):
            want = tcr.labels_cand(ent, ct["tab"], 2, hw, p.ys, p.xs, ramp, **flags)
            got = _run_guarded(ops, p, ent, ct["tab"], 2, None, 64, hw, **flags)
            _check(got, want, (tile, hw, ramp, flags))
            assert got[2].tolist() == [255, 0]


def test_the_ramp_toward_an_absent_neighbour_is_half_up(ops):
    """8 x 8 on 8 x 9 with ramp 1: columns 1..7 are covered by both windows, only window 1 lists the class, all 255.  The
    virtual byte there is (2 * 255 + 2) / 4 = 128 -- half, rounded up -- which the fixed threshold brackets: foreground
    above 127.5 / 255, background above 128.5 / 255; column 8 (window 1 alone) stays 255, column 0 (window 0 alone) 0."""
    p = _plan((8, 9), (8, 8), 2, 1)
    assert p.xs == [0, 1]
    ct = p.candidate_table([[], [0]], 1)
    ent = torch.full((1, 3, 8, 8), 255, dtype=torch.uint8, device="cuda")
    tab = ct["tab"].cuda()
    lo = ops.tiles_labels_cand(p, ent, tab, ct["tab"], 1, r_threshold=0.0, threshold=127.5 / 255)[0].cpu()
    hi = ops.tiles_labels_cand(p, ent, tab, ct["tab"], 1, r_threshold=0.0, threshold=128.5 / 255)[0].cpu()
    assert (lo[:, 0] == 0).all() and (lo[:, 1:] == 1).all()
    assert (hi[:, :8] == 0).all() and (hi[:, 8] == 1).all()


@pytest.mark.parametrize("tile,hw,ov", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_no_entry_anywhere(ops, tile, hw, ov):
    """E = 0 (ent is None): labels are all 0, mx and area are 0, counts are the reference's for an all-background map."""
    N = 3
    p = _plan(hw, tile, ov)
    ct = p.candidate_table([()] * p.T, N)
    gt = _gt(hw, N, np.random.RandomState(5))
    want = tcr.labels_cand(None, ct["tab"], N, hw, p.ys, p.xs, p.ramp, gt, tile=tile)
    for flags in (dict(r_threshold=0.25, threshold=0.0), dict(r_threshold=0.0, threshold=0.45)):
        got = _run_guarded(ops, p, None, ct["tab"], N, gt, 61, hw, **flags)
        _check(got, want, flags)
        assert not got[0].any() and not got[2].any() and not got[3].any()
        assert got[1][0, 0] == int((gt == 0).sum()) and got[1][0, 1:].sum() == 0


# ------------------------------------------------------------------------------------------------ the route, tiny engine

HW, TILE = (88, 150), (64, 64)
SHOTS = (1, 3, 2)
LISTS = [(0, 2), (1,), (), (0, 1, 2), (2,), ()]


def _image(hw, seed):
    return np.random.RandomState(seed).randint(0, 256, hw + (3,)).astype(np.uint8)


def _label_gt(hw, N, seed):
    rs = np.random.RandomState(seed)
    g = rs.randint(0, N + 1, hw).astype(np.uint8)
    g[rs.rand(*hw) < 0.05] = 255
    return g


def _library(pipe):
    sets = [_support_set(s, 64, seed=910 + 10 * c) for c, s in enumerate(SHOTS)]
    return pipe.prepare_support_classes([a.cuda() for a, _ in sets], [m.cuda() for _, m in sets])


def _replayed_entries(pipe, ops, library, plan, img, groups, entry_batch, captured):
    """The entry bytes of the route: every group of r["groups"] through segment_candidates again."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    q = ops.tiles_cut(plan, torch.from_numpy(img).cuda(), DeviceImageTransform(TILE).lut)
    parts = []
    for ws, ls in groups:
        r = pipe.segment_candidates(library, q[list(ws)].contiguous(), ls, entry_batch=entry_batch, captured=captured)
        assert r["entries"] == [(i, c) for i, cs in enumerate(ls) for c in cs]
        parts.append(r["seg_u8"].cpu())
    return torch.cat(parts).numpy()


@pytest.mark.parametrize("batch", [2, 3], ids=["b2", "b3-padded"])
def test_segment_tiled_with_candidates_equals_the_reference_on_its_entries(models, ops, batch):
    """88 x 150 against a ragged 3-class library, windows 2 and 5 without a candidate, eager and captured: the groups are the
    non-empty windows in order in runs of `batch` (the last padded by its last window with an empty list); replaying them
    through segment_candidates gives the entry bytes, and the reference on those gives labels, counts, mx and area.  A
    captured run passes the capture's no-memset-node check; all-empty lists run no UNet."""
    pipe = models["pipe"]
    pipe._graphs = {}
    library = _library(pipe)
    N = len(SHOTS)
    img, gt = _image(HW, 5), _label_gt(HW, N, 6)
    try:
        for captured in (False, True):
            pipe.graph_nodes = 0
            r = pipe.segment_tiled(library, img, gt, batch=batch, captured=captured, candidates=LISTS, entry_batch=2)
            r = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}
            assert (pipe.graph_nodes > 0) == captured             # every capture is checked for memset nodes
            assert "seg_u8" not in r
            p = r["plan"]
            assert (p.ys, p.xs, p.T) == ([0, 24], [0, 43, 86], 6)
            assert r["entries"] == [(t, c) for t, cs in enumerate(LISTS) for c in cs] and r["offsets"] == [0, 2, 3, 3, 6, 7, 7]
            # the groups: every non-empty window once, in order, at most `batch` per group, padding = last window, ()
            seen = []
            for ws, ls in r["groups"]:
                assert len(ws) == len(ls) == batch
                real = [(t, l) for t, l in zip(ws, ls) if l]
                assert all(l == LISTS[t] for t, l in real) and [l for _, l in real] == list(ls[:len(real)])
                assert all(l == () and t == real[-1][0] for t, l in list(zip(ws, ls))[len(real):])
                seen += [t for t, _ in real]
            assert seen == [0, 1, 3, 4]
            ngraphs = len(pipe._graphs)
            ent = _replayed_entries(pipe, ops, library, p, img, r["groups"], 2, captured)
            assert len(pipe._graphs) == ngraphs                   # the same keys: nothing new was captured
            assert ent.shape == (7, 3) + TILE
            tab = p.candidate_table(LISTS, N)["tab"]
            want = tcr.labels_cand(ent, tab, N, HW, p.ys, p.xs, p.ramp, gt)
            assert r["labels"].shape == HW and r["labels"].dtype == torch.uint8 and r["counts"].shape == (2, N + 1)
            assert r["mx"].dtype == torch.int32 and r["area"].shape == (N, 2)
            _check((r["labels"].cpu(), r["counts"].cpu(), r["mx"].cpu(), r["area"].cpu()), want, (batch, captured))
            # a callable on the plan gives the same result; without gt there are no counts
            r2 = pipe.segment_tiled(library, img, batch=batch, captured=captured, candidates=lambda plan: LISTS[:plan.T],
                                    entry_batch=2)
            assert r2["counts"] is None and torch.equal(r2["labels"], r["labels"])
        called = []
        orig = pipe.segment_candidates
        pipe.segment_candidates = lambda *a, **k: called.append(1) or orig(*a, **k)
        try:
            r = pipe.segment_tiled(library, img, gt, batch=batch, candidates=[()] * 6, entry_batch=2)
        finally:
            del pipe.segment_candidates
        assert not called and r["groups"] == [] and r["entries"] == [] and not r["labels"].any() and not r["mx"].any()
        want = tcr.labels_cand(None, p.candidate_table([()] * 6, N)["tab"], N, HW, p.ys, p.xs, p.ramp, gt, tile=TILE)
        assert torch.equal(r["counts"].cpu(), want[1])
        sup, msk = _support_set(2, 64, seed=900)
        bank = pipe.prepare_support(sup.cuda(), msk.cuda())
        with pytest.raises(ValueError, match="SupportBankSet"):
            pipe.segment_tiled(bank, img, candidates=LISTS)
        with pytest.raises(ValueError, match="candidate lists"):
            pipe.segment_tiled(library, img, candidates=LISTS[:5])
    finally:
        pipe._graphs = {}


def test_propose_tile_candidates_is_its_composition(models):
    """One squeeze to the processing size, one segment_classes call with b = 1, candidates_from_labels on its labels."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    pipe = models["pipe"]
    library = _library(pipe)
    img = _image(HW, 21)
    args, lists = pipe.propose_tile_candidates(library, img, min_pixels=3, margin=2, captured=False)
    assert args == dict(overlap=8, ramp=None)
    q = DeviceImageTransform(TILE).image(img)
    coarse = pipe.segment_classes(library, q[None], captured=False)["labels"][0].cpu().numpy()
    p = _plan(HW, TILE, 8)
    assert lists == p.candidates_from_labels(coarse, min_pixels=3, margin=2) and len(lists) == p.T
    args, lists = pipe.propose_tile_candidates(library, img, overlap=16, ramp=4, captured=False, r_threshold=0.0, threshold=0.4)
    coarse = pipe.segment_classes(library, q[None], captured=False, r_threshold=0.0, threshold=0.4)["labels"][0].cpu().numpy()
    p = _plan(HW, TILE, 16, 4)
    assert args == dict(overlap=16, ramp=4) and lists == p.candidates_from_labels(coarse, min_pixels=1, margin=1)
    r = pipe.segment_tiled(library, img, captured=False, candidates=lists, **args)      # usable as they come
    assert r["plan"].T == len(lists) and r["labels"].shape == HW


def test_evaluate_tiled_with_candidates_sums_the_calls_counts(models):
    from diffews_amd.evaluate import evaluate_tiled
    from diffews_amd.metrics import nway_iou
    pipe = models["pipe"]
    pipe._graphs = {}
    library = _library(pipe)
    N = len(SHOTS)
    items = [(_image(HW, 11), _label_gt(HW, N, 12), LISTS), (_image((64, 100), 13), _label_gt((64, 100), N, 14), [(1,), (0, 2)]),
             (_image((64, 100), 15), _label_gt((64, 100), N, 16))]
    try:
        total = sum(pipe.segment_tiled(library, it[0], it[1], batch=2, captured=True, entry_batch=2,
                                       **(dict(candidates=it[2]) if len(it) > 2 else {}))["counts"].clone() for it in items)
        miou, iou, counts = evaluate_tiled(pipe, library, items, batch=2, entry_batch=2)
        assert torch.equal(counts, total)
        ref_iou, ref_miou = nway_iou(total)
        assert miou == ref_miou and torch.equal(iou, ref_iou)
    finally:
        pipe._graphs = {}
