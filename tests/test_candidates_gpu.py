"""GPU tests of candidate classes per query -- every query against a handful of a SupportBankSet's classes, a different
handful per query, fused into one label map.

Kernel: ops.seg_labels_cand against the independent numpy reference tests/cand_ref.py, exactly (labels, counts, area), on
the word path (8 x 12), the scalar path (7 x 9) and the alignment fallback (8 x 12 at a 1-byte offset), with an empty query,
padding entries, ties, label 254, every byte value, both threshold forms and a ground truth that holds every kind of value;
against ops.seg_labels on full lists; and one captured launch replayed after the device table was rewritten in place.

Pipeline (tiny config, 64 x 64, library shots (1, 3, 2) and a uniform one, b = 3, candidates ((2, 0), (1,), (0, 1, 2)),
entry_batch 2 and 4): segment_candidates per pass against segment_routed on the same pass batch (exact), per entry against
segment_queries at batch 1 (TOL_EP), labels / counts / area against cand_ref on the call's own seg_u8 (exact), captured
against eager with ONE graph for two candidate assignments, through segment_stream(candidates=...) and
evaluate_candidates."""
import numpy as np
import pytest
import torch

import cand_ref
import test_query_loader_gpu as ql
from test_model_gpu import TOL_EP
from test_ragged_sets_gpu import _classes, _cuda
from test_support_bank_gpu import models, ops, rel, _queries  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

OFF = [0, 2, 2, 5]                                      # B = 3, k = (2, 0, 3)
MODES = [dict(r_threshold=0.25), dict(r_threshold=0.55), dict(r_threshold=0.0, threshold=0.5)]
MODE_IDS = ["dyn.25", "dyn.55", "fixed.5"]


def _entries(H, W, E_cap, seed):
    """Random bytes, with ties: entry 1 is entry 0 (query 0), entry 4 is entry 2 on the upper half (query 2), entry 3 has a
    dark left half so that it loses its threshold there."""
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, size=(E_cap, 3, H, W), dtype=np.uint8)
    u8[1] = u8[0]
    u8[4, :, :H // 2] = u8[2, :, :H // 2]
    u8[3, :, :, :W // 2] //= 8
    return u8


def _gt(H, W, values, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array(values, np.uint8), size=(3, H, W))


def _offset_view(t):
    """The same bytes at a 1-byte offset into a larger buffer."""
    buf = torch.empty(t.numel() + 5, dtype=torch.uint8, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 4 == 1 and v.is_contiguous()
    return v


def _run(ops, u8, mx, off, lab, nlabels, gt, flags, offset=False):
    E_cap, _, H, W = u8.shape
    B = len(off) - 1
    tab_host = torch.tensor(list(off) + list(lab) + [0] * (E_cap - len(lab)), dtype=torch.int32)
    d_u8 = torch.from_numpy(u8).cuda()
    d_gt = None if gt is None else torch.from_numpy(gt).cuda()
    lab_out = None
    if offset:
        d_u8, d_gt = _offset_view(d_u8), None if d_gt is None else _offset_view(d_gt)
        lab_out = _offset_view(torch.zeros(B, H, W, dtype=torch.uint8, device="cuda"))
    d_mx = None if mx is None else torch.from_numpy(mx).cuda()
    labels, counts, area = ops.seg_labels_cand(d_u8, d_mx, tab_host.cuda(), tab_host, nlabels, d_gt, want_area=True,
                                               labels_out=lab_out, **flags)
    torch.cuda.synchronize()
    return labels, counts, area


def _same(got, want):
    for g, w, what in zip(got, want, ("labels", "counts", "area")):
        if w is None:
            assert g is None, what
        else:
            assert torch.equal(g.cpu(), torch.from_numpy(w)), what


KERNEL_SHAPES = [(8, 12, False), (7, 9, False), (8, 12, True)]
SHAPE_IDS = ["8x12-words", "7x9-scalar", "8x12-offset1"]


@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nlabels", [9, 254])
@pytest.mark.parametrize("E_cap", [6, 8])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=SHAPE_IDS)
def test_kernel_equals_reference(ops, shape, E_cap, nlabels, flags):
    """B = 3 with k = (2, 0, 3) out of E_cap entries (one or three of padding), labels up to nlabels, ties, the dynamic
    threshold and the fixed one with mx = None; gt holds 0, candidate labels, a label that is no candidate of the query, a
    value in (nlabels, 255) where there is one, and 255.  Exact on labels, counts and area."""
    H, W, offset = shape
    top = nlabels
    lab = [top, 3, 1, 7, top]
    values = [0, 3, top, 1, 7, 5, 255] + ([40] if nlabels < 254 else [])
    u8 = _entries(H, W, E_cap, seed=H * 100 + E_cap)
    gt = _gt(H, W, values, seed=3)
    mx = cand_ref.maxima(u8) if flags["r_threshold"] > 0 else None
    want = cand_ref.seg_labels_cand(u8, cand_ref.maxima(u8), OFF, lab + [0] * (E_cap - 5), nlabels, gt, **flags)
    got = _run(ops, u8, mx, OFF, lab, nlabels, gt, flags, offset)
    _same(got, want)
    lw = want[0]
    assert not lw[1].any() and (lw[0] == top).any() and not (lw[0] == 3).any()      # empty query; the tie went to entry 0
    assert (lw[2] == 1).any() and (want[2][5:] == 0).all()
    # without gt: no counts, the same labels and area
    got = _run(ops, u8, mx, OFF, lab, nlabels, None, flags, offset)
    _same(got, (want[0], None, want[2]))


@pytest.mark.parametrize("flags", MODES[1:], ids=MODE_IDS[1:])
def test_kernel_every_byte_value(ops, flags):
    """16 x 16: every channel of every entry holds each of the 256 byte values once, in different orders."""
    i = np.arange(256)
    perm = lambda a, c: ((i * a + c) % 256).astype(np.uint8).reshape(16, 16)
    u8 = np.stack([np.stack([perm(1, 0), perm(7, 3), perm(255, 255)]),
                   np.stack([perm(3, 1), perm(1, 0), perm(5, 9)]),
                   np.stack([perm(11, 4), perm(13, 77), perm(1, 128)]),
                   np.stack([perm(1, 0), perm(1, 0), perm(1, 0)])])
    for e in range(4):
        for c in range(3):
            assert len(np.unique(u8[e, c])) == 256
    off, lab = [0, 3, 4], [2, 1, 3, 2]
    gt = np.random.default_rng(1).choice(np.array([0, 1, 2, 3, 200, 255], np.uint8), size=(2, 16, 16))
    mx = cand_ref.maxima(u8)
    want = cand_ref.seg_labels_cand(u8, mx, off, lab, 3, gt, **flags)
    _same(_run(ops, u8, mx if flags["r_threshold"] > 0 else None, off, lab, 3, gt, flags), want)
    assert len(np.unique(want[0][0])) >= 3


@pytest.mark.parametrize("flags", MODES[::2], ids=MODE_IDS[::2])
@pytest.mark.parametrize("hw", [(8, 12), (7, 9)], ids=["8x12", "7x9"])
def test_full_lists_equal_seg_labels(ops, hw, flags):
    """off = (0, N, 2N, ...), lab[qN + c] = 1 + c, seg_u8 / mx permuted from class-major to query-major: labels and counts
    are ops.seg_labels' (batch_max = False), bit for bit.  N = 3, B = 2."""
    N, B, (H, W) = 3, 2, hw
    rng = np.random.default_rng(11)
    u8 = rng.integers(0, 256, size=(N, B, 3, H, W), dtype=np.uint8)
    u8[1, 0] = u8[0, 0]
    u8[2, 1, :, :3] = u8[1, 1, :, :3]
    gt = torch.from_numpy(rng.choice(np.array([0, 1, 2, 3, 9, 255], np.uint8), size=(B, H, W))).cuda()
    cls = torch.from_numpy(u8).cuda()
    mx_c = torch.from_numpy(u8.reshape(N, B, -1).max(-1).astype(np.int32)).cuda()
    lab_n, cnt_n = ops.seg_labels(cls, mx_c if flags["r_threshold"] > 0 else None, gt, batch_max=False, **flags)
    ent = cls.transpose(0, 1).contiguous().view(B * N, 3, H, W)
    mx_e = mx_c.t().contiguous().view(-1)
    tab = torch.tensor([q * N for q in range(B + 1)] + [1 + c for _ in range(B) for c in range(N)], dtype=torch.int32)
    lab_c, cnt_c, _ = ops.seg_labels_cand(ent, mx_e if flags["r_threshold"] > 0 else None, tab.cuda(), tab, N, gt, **flags)
    assert torch.equal(lab_c, lab_n) and torch.equal(cnt_c, cnt_n)
    assert (lab_n[0] == 1).any() and not (lab_n[0] == 2).any()


def test_captured_launch_follows_the_table(ops):
    """One launch captured in a torch.cuda.graph, replayed after the device table was rewritten in place to another
    partition of the same E_cap (and other labels): each replay equals the reference of the table it found."""
    H, W, E_cap, nlabels = 8, 12, 6, 9
    u8 = _entries(H, W, E_cap, seed=21)
    gt = _gt(H, W, [0, 1, 2, 3, 4, 7, 9, 40, 255], seed=4)
    mx = cand_ref.maxima(u8)
    tables = [(OFF, [9, 3, 1, 7, 9, 0]), ([0, 1, 4, 6], [2, 4, 1, 9, 3, 7]), ([0, 0, 6, 6], [1, 2, 3, 4, 7, 9]),
              (OFF, [9, 3, 1, 7, 9, 0])]
    words = lambda t: torch.tensor(list(t[0]) + list(t[1]), dtype=torch.int32)
    mirror = words(tables[0])
    tab = mirror.cuda()
    d_u8, d_mx, d_gt = torch.from_numpy(u8).cuda(), torch.from_numpy(mx).cuda(), torch.from_numpy(gt).cuda()
    labels = torch.empty(3, H, W, dtype=torch.uint8, device="cuda")
    counts = torch.empty(3, 2, nlabels + 1, dtype=torch.int64, device="cuda")
    launch = lambda: ops.seg_labels_cand(d_u8, d_mx, tab, mirror, nlabels, d_gt, want_area=True, labels_out=labels,
                                         counts_out=counts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, _, area = launch()
    seen = []
    for t in tables:
        tab.copy_(words(t))
        graph.replay()
        torch.cuda.synchronize()
        want = cand_ref.seg_labels_cand(u8, mx, t[0], t[1], nlabels, gt)
        _same((labels, counts, area), want)
        seen.append(labels.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and torch.equal(seen[0], seen[3])


# ------------------------------------------------------------------------------------------------ pipeline

SHOTS, RES, B_Q = (1, 3, 2), 64, 3
CAND = ((2, 0), (1,), (0, 1, 2))
KEYS = ("z0", "dec", "seg_u8", "labels", "counts", "area")


def _label_gt(b, seed, values=(0, 1, 2, 3, 40, 255)):
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(values, dtype=torch.uint8)
    return v[torch.randint(0, len(values), (b, RES, RES), generator=g)]


def _library(pipe, library, seed):
    shots = SHOTS if library == "ragged" else (2, 2, 2)
    sup, msk = _classes(seed=seed, shots=shots)
    if library == "ragged":
        return pipe.prepare_support_classes(_cuda(sup), _cuda(msk))
    return pipe.prepare_support_classes(torch.stack(sup).cuda(), torch.stack(msk).cuda())


def _ref_of(r, gt, nlabels, tab, flags):
    """cand_ref on the call's own seg_u8 and maxima."""
    u8 = r["seg_u8"].cpu().numpy()
    E, b = u8.shape[0], len(r["offsets"]) - 1
    return cand_ref.seg_labels_cand(u8, cand_ref.maxima(u8), r["offsets"], tab[b + 1:b + 1 + E].tolist(), nlabels,
                                    None if gt is None else gt.numpy(), **flags)


def _pass_sets(r, E_pad):
    """The set of every entry, padding included (padding repeats the last real entry)."""
    sets = [c for _, c in r["entries"]]
    return sets + [sets[-1]] * (E_pad - len(sets))


@pytest.mark.parametrize("entry_batch", [2, 4])
@pytest.mark.parametrize("library", ["ragged", "uniform"])
def test_segment_candidates_equals_segment_routed_per_pass(models, library, entry_batch):
    """z0 / dec / seg_u8 of every pass are torch.equal to segment_routed run on the same pass batch: the same entry_batch
    entries, the same rows, the query images gathered with the entries' indices.  The relative distance of every pass' z0
    is printed before it is asserted.  It holds because the queries are encoded in chunks of entry_batch: the VAE
    encoder's GEMM plans depend on its batch (at this size batch 2 and 3 give the same bits per image, batch 4 others), and
    segment_routed encodes at the pass batch."""
    pipe, dt = models["pipe"], models["dt"]
    bankset = _library(pipe, library, 1000)
    qry = _queries(B_Q, RES, seed=1010).cuda()
    r = pipe.segment_candidates(bankset, qry, CAND, entry_batch=entry_batch, captured=False)
    ct = bankset.candidate_tables(CAND, entry_batch)
    E, E_pad = ct["E"], ct["E_pad"]
    sets, ent = _pass_sets(r, E_pad), ct["entries"].tolist()
    ones = []
    for e0 in range(0, E_pad, entry_batch):
        e1, n = e0 + entry_batch, min(E, e0 + entry_batch) - e0
        one = pipe.segment_routed(bankset, qry[ent[e0:e1]], sets[e0:e1], captured=False)
        if n > 0:
            print(f"[candidates] {library} eb {entry_batch} pass at entry {e0} {dt}: z0 vs segment_routed on the pass batch "
                  f"{rel(r['z0'][e0:e0 + n], one['z0'][:n]):.3e}, seg_u8 bytes that differ "
                  f"{int((r['seg_u8'][e0:e0 + n] != one['seg_u8'][:n]).sum())}")
        ones.append((e0, n, {k: one[k].clone() for k in ("z0", "dec", "seg_u8")}))
    for e0, n, one in ones:
        for k in ("z0", "dec", "seg_u8"):
            assert torch.equal(r[k][e0:e0 + n], one[k][:n]), (e0, k)


@pytest.mark.parametrize("entry_batch", [2, 4])
@pytest.mark.parametrize("library", ["ragged", "uniform"])
def test_segment_candidates_vs_references(models, library, entry_batch):
    """segment_candidates(bankset, qry, CAND): shapes and bookkeeping; every entry is within TOL_EP of
    segment_queries(bankset.bank(set), query) at batch 1 (printed); labels, counts and area are cand_ref's on the call's own
    seg_u8 and maxima, exactly, with the dynamic and the fixed threshold and with local labels."""
    pipe, dt = models["pipe"], models["dt"]
    bankset = _library(pipe, library, 1000)
    qry = _queries(B_Q, RES, seed=1010).cuda()
    gt = _label_gt(B_Q, 5)
    r = pipe.segment_candidates(bankset, qry, CAND, gt.cuda(), entry_batch=entry_batch, captured=False)
    assert set(r) == set(KEYS) | {"entries", "offsets"}
    ct = bankset.candidate_tables(CAND, entry_batch)
    E, E_pad = 6, ct["E_pad"]
    assert E_pad == {2: 6, 4: 8}[entry_batch] and ct["nlabels"] == 3
    h, w = bankset.hw
    assert r["z0"].shape == (E, 4, h, w) and r["dec"].shape == (E, 3, RES, RES) and r["seg_u8"].shape == (E, 3, RES, RES)
    assert r["labels"].shape == (B_Q, RES, RES) and r["labels"].dtype == torch.uint8
    assert r["counts"].shape == (B_Q, 2, 4) and r["area"].shape == (E, 2) and r["area"].dtype == torch.int64
    assert r["entries"] == [(0, 0), (0, 2), (1, 1), (2, 0), (2, 1), (2, 2)] and r["offsets"] == [0, 2, 3, 6]
    worst = 0.0
    for e, (i, c) in enumerate(r["entries"]):
        solo = pipe.segment_queries(bankset.bank(c), qry[i:i + 1], captured=False)
        d = rel(r["z0"][e:e + 1], solo["z0"])
        worst = max(worst, d)
        print(f"[candidates] {library} eb {entry_batch} entry {e} = (query {i}, set {c}) {dt}: z0 vs segment_queries at "
              f"batch 1 {d:.3e} (TOL_EP {TOL_EP[dt]:.1e})")
    assert worst < TOL_EP[dt], worst
    _same((r["labels"], r["counts"], r["area"]), _ref_of(r, gt, 3, ct["tab"], dict(r_threshold=0.25)))
    assert int(r["area"][:, 1].sum()) == int((r["labels"] != 0).sum())
    nogt = pipe.segment_candidates(bankset, qry, CAND, entry_batch=entry_batch, captured=False)
    assert nogt["counts"] is None and torch.equal(nogt["labels"], r["labels"]) and torch.equal(nogt["area"], r["area"])
    flags = dict(r_threshold=0.0, threshold=0.3)
    rf = pipe.segment_candidates(bankset, qry, CAND, gt.cuda(), entry_batch=entry_batch, captured=False, **flags)
    _same((rf["labels"], rf["counts"], rf["area"]), _ref_of(rf, gt, 3, ct["tab"], flags))
    assert torch.equal(rf["z0"], r["z0"])
    # local labels: 1 + position in the query's list
    rl = pipe.segment_candidates(bankset, qry, CAND, gt.cuda(), entry_batch=entry_batch, labels="local", captured=False)
    lt = bankset.candidate_tables(CAND, entry_batch, labels="local")
    assert rl["counts"].shape == (B_Q, 2, 4) and torch.equal(rl["seg_u8"], r["seg_u8"])
    _same((rl["labels"], rl["counts"], rl["area"]), _ref_of(rl, gt, 3, lt["tab"], dict(r_threshold=0.25)))


def test_segment_candidates_errors(models):
    pipe = models["pipe"]
    bankset = _library(pipe, "ragged", 1000)
    qry = _queries(B_Q, RES, seed=1010).cuda()
    for bad in (CAND[:2], CAND + ((0,),), (), ((2, 0), (1,), (0, 3)), ((2, 2), (1,), (0,)), ((), (), ())):
        with pytest.raises(ValueError):                              # wrong number of lists, and candidate_tables' errors
            pipe.segment_candidates(bankset, qry, bad, captured=False)
    with pytest.raises(ValueError):                                  # a SupportBank
        pipe.segment_candidates(bankset.bank(0), qry, CAND, captured=False)
    qs = ql._host_queries(2, seed=3, with_gt=False)
    for q in qs:
        q["cand"], q["cls"] = (0, 1), 0
    with pytest.raises(ValueError):                                  # route and candidates together
        next(pipe.segment_stream(bankset, qs, size=RES, route="cls", candidates="cand"))
    with pytest.raises(ValueError):                                  # a SupportBank
        next(pipe.segment_stream(bankset.bank(0), qs, size=RES, candidates="cand"))


def test_full_lists_against_segment_classes(models):
    """Candidates = all N sets for every query, one query per pass: the labels are compared with segment_classes.  The
    number of differing pixels is printed, not asserted -- GEMM plans depend on the pass batch (b entries of one class
    there, the N classes of one query here), so single pixels may fall on the other side of a threshold; the label rule
    itself is held exactly by test_full_lists_equal_seg_labels."""
    pipe, dt = models["pipe"], models["dt"]
    bankset = _library(pipe, "ragged", 1020)
    qry = _queries(B_Q, RES, seed=1030).cuda()
    gt = _label_gt(B_Q, 6).cuda()
    full = [tuple(range(3))] * B_Q
    r = pipe.segment_candidates(bankset, qry, full, gt, entry_batch=3, captured=False)
    c = pipe.segment_classes(bankset, qry, gt, captured=False)
    assert r["labels"].shape == c["labels"].shape and r["counts"].shape == c["counts"].shape
    diff = int((r["labels"] != c["labels"]).sum())
    z = max(rel(r["z0"][q * 3 + k:q * 3 + k + 1], c["z0"][k, q:q + 1]) for q in range(B_Q) for k in range(3))
    print(f"[candidates] full lists vs segment_classes {dt}: {diff} of {r['labels'].numel()} label pixels differ, "
          f"largest z0 distance of an entry {z:.3e}")


def test_segment_candidates_captured_equals_eager(models):
    """captured=True replays the same kernels: identical bits on every returned tensor, and ONE graph serves further
    candidate assignments with the same number of passes (the candidates are not in the key; indices, rows and the label
    table are static inputs copied per call) -- each replay equals its own eager call."""
    pipe = models["pipe"]
    pipe._graphs = {}
    bankset = _library(pipe, "ragged", 1040)
    gt = _label_gt(B_Q, 8).cuda()
    assignments = [CAND, ((0, 1), (1, 2, 0), (2,)), ((1, 2), (), (2, 0, 1)), CAND]    # E = 6, 6, 5 (a query with none), 6: E_pad 8
    try:
        labels = []
        for n, cand in enumerate(assignments):
            qry = _queries(B_Q, RES, 1050 + n % 2).cuda()
            e = pipe.segment_candidates(bankset, qry, cand, gt, entry_batch=4, captured=False)
            e = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in e.items()}
            c = pipe.segment_candidates(bankset, qry, cand, gt, entry_batch=4, captured=True)
            for k in KEYS:
                assert e[k].shape == c[k].shape and torch.equal(e[k], c[k]), (cand, k)
            assert e["entries"] == c["entries"] and e["offsets"] == c["offsets"]
            assert len(pipe._graphs) == 1, list(pipe._graphs)
            labels.append(e["labels"])
        key = next(iter(pipe._graphs))
        assert key[:3] == ("queries", "candidates", bankset.uid)
        assert not any(x in (CAND, list(CAND)) for x in key)
        assert not torch.equal(labels[0], labels[1])
        assert not labels[2][1].any()                                    # the query without candidates
        # another number of passes is another graph, and it is a query graph like the others
        pipe.segment_candidates(bankset, _queries(B_Q, RES, 1050).cuda(), CAND, gt, entry_batch=2, captured=True)
        assert sum(1 for k in pipe._graphs if k[:2] == ("queries", "candidates")) == 2
    finally:
        pipe._graphs = {}


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_stream_and_evaluate_candidates(models, captured):
    """segment_stream(bankset, queries, candidates=...) over five queries in batches of three (the last one short): per
    batch the dict of segment_candidates on the hand-built batch plus `candidates`, no `native`; a key name and a callable
    agree; evaluate_candidates over the same batches returns their summed counts and metrics.nway_iou of them."""
    from diffews_amd import evaluate
    from diffews_amd.input_pipeline import DeviceImageTransform
    from diffews_amd.metrics import nway_iou
    pipe = models["pipe"]
    pipe._graphs = {}
    try:
        bankset = _library(pipe, "ragged", 1060)
        tf = DeviceImageTransform(RES)
        qs = ql._host_queries(5, seed=61, with_gt=False)
        lists = [(2, 0), (1,), (0, 1, 2), (1, 2), (0,)]
        maps = _label_gt(5, 9)
        for q, cs, m in zip(qs, lists, maps):
            q["cand"], q["labels"] = cs, m.numpy()
        kw = dict(batch=3, size=RES, depth=1, entry_batch=4, captured=captured)
        got = []
        for index, r in pipe.segment_stream(bankset, qs, candidates="cand", **kw):
            assert set(r) == set(KEYS) | {"entries", "offsets", "candidates"} and "native" not in r
            got.append((index, r["candidates"], {k: r[k].clone() for k in KEYS}))
        assert [g[0] for g in got] == [[0, 1, 2], [3, 4]]
        assert [g[1] for g in got] == [[list(c) for c in lists[:3]], [list(c) for c in lists[3:]]]
        items, total = [], torch.zeros(2, 4, dtype=torch.int64, device=pipe.device)
        for index, cands, out in got:
            qry = torch.stack([tf.image(qs[i]["query_img"]) for i in index])
            r = pipe.segment_candidates(bankset, qry, cands, maps[index], entry_batch=4, captured=captured)
            for k in KEYS:
                assert torch.equal(out[k], r[k]), (index, k)
            total += r["counts"].sum(0)
            items.append((qry, cands, maps[index]))
        assert int(total[1, 1:].sum()) > 0
        again = [r["counts"].clone() for _, r in pipe.segment_stream(bankset, qs, candidates=lambda q: q["cand"], **kw)]
        assert all(torch.equal(a, g[2]["counts"]) for a, g in zip(again, got))
        miou, iou, counts = evaluate.evaluate_candidates(pipe, bankset, items, entry_batch=4, captured=captured)
        assert counts.dtype == torch.int64 and torch.equal(counts, total)
        want_iou, want_miou = nway_iou(total)
        assert miou == want_miou and torch.equal(iou, want_iou)
        # without `labels` on the queries: no counts
        for q in qs:
            del q["labels"]
        index, r = next(pipe.segment_stream(bankset, qs, candidates="cand", **kw))
        assert r["counts"] is None and torch.equal(r["labels"], got[0][2]["labels"])
    finally:
        pipe._graphs = {}
