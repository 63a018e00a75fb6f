"""GPU tests of candidate classes per query at native size: ops.seg_labels_cand_native / dfw_seg_labels_cand_native and the
plumbing above it.  Everything is integer or fixed-expression fp32 work, so every comparison is torch.equal.

Kernels, on tests/cand_native_ref.py's discriminating input (32 x 32 -> (41, 50), (23, 37) on the scalar path and (40, 48)
on the word path; lists (0, 2), (), (0, 1, 3) of 4 classes, E = 5 of E_cap = 8, a tie, an overshooting block, padding planes
of 255): against the CPU reference in every form of threshold, id table, ground-truth width and output; against
ops.seg_labels_native on full lists; against ops.seg_labels_cand at equal sizes (the resize is then the identity); with a
device table rewritten after the host validated it, inside 0xA5 guards; with other bytes in the padding.

Pipeline (tiny config, 64 x 64): segment_candidates_native is the op on its own seg_u8 and the CPU reference of it,
adds nothing but `native`, agrees captured and eager with the same graphs; segment_stream(candidates=, native=True) and
evaluate_candidates(use_original_imgsize=True) are the hand-built calls."""
import numpy as np
import pytest
import torch

import cand_native_ref as cn
import nway_native_ref as nn
import test_query_loader_gpu as ql
from test_candidates_gpu import B_Q, CAND, KEYS, RES, _library
from test_support_bank_gpu import models, ops, _queries  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

FLAGS = [dict(r_threshold=0.25), dict(r_threshold=0.0, threshold=0.3)]
FLAG_IDS = ["dyn.25", "fixed.3"]
GUARD = 0xA5


def _targets(sizes, gts=None, src=cn.DISC_SRC, ignore=cn.DISC_IGNORE, guard=0):
    from diffews_amd.input_pipeline import NativeTargets
    return NativeTargets(src, sizes, gt=gts, ignore_value=ignore, guard=guard)


def _tab(off, lab):
    return torch.tensor(list(off) + list(lab), dtype=torch.int32)


def _same(got, want):
    """The op's dict against cand_native_ref's."""
    for i, (g, w) in enumerate(zip(got["labels"], want["labels"])):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), ("labels", i)
    if want["counts"] is None:
        assert got["counts"] is None
    else:
        assert torch.equal(got["counts"].cpu(), torch.from_numpy(want["counts"])), "counts"
    assert torch.equal(got["area"].cpu(), torch.from_numpy(want["area"])), "area"
    assert torch.equal(got["mx"].cpu(), torch.from_numpy(want["mx"])), "mx"


_REF = {}


def _disc_ref(mode, flags, wide):
    """The reference on the discriminating input, computed once per form and shared (never written)."""
    key = (mode, tuple(sorted(flags.items())), wide)
    if key not in _REF:
        if "x" not in _REF:
            _REF["x"] = cn.discriminating_input()
            _REF["res"] = cn.resized(_REF["x"], cn.DISC_OFF, cn.DISC_SIZES)
        dtype = np.int32 if wide else np.uint8
        labels = "local" if mode == "entry_ids" else "set"
        lab, nlabels, entry_ids = cn.disc_tables(labels)
        gts = cn.disc_gts("labels" if mode == "none" else "ids", dtype)
        kw = dict(none={}, class_ids=dict(class_ids=cn.DISC_CLASS_IDS), entry_ids=dict(entry_ids=entry_ids))[mode]
        want = cn.cand_native_ref(_REF["x"], cn.DISC_OFF, lab, nlabels, cn.DISC_SIZES, gts, ignore_value=cn.DISC_IGNORE,
                                  res=_REF["res"], **kw, **flags)
        _REF[key] = (lab, nlabels, gts, kw, want)
    return (_REF["x"],) + _REF[key]


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("want_u8", [False, True], ids=["staged", "out_u8"])
@pytest.mark.parametrize("wide", [False, True], ids=["gt-u8", "gt-i32"])
@pytest.mark.parametrize("mode", ["none", "class_ids", "entry_ids"])
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_op_equals_reference(ops, flags, mode, wide, want_u8):
    x, lab, nlabels, gts, kw, want = _disc_ref(mode, flags, wide)
    t = _targets(cn.DISC_SIZES, gts)
    assert [it.gt_elem for it in t.items] == [4 if wide else 1] * 3
    tab = _tab(cn.DISC_OFF, lab)
    got = ops.seg_labels_cand_native(x.cuda(), t, tab.cuda(), tab, nlabels, want_area=True, want_u8=want_u8, **kw, **flags)
    torch.cuda.synchronize()
    _same(got, want)
    assert got["sizes"] == cn.DISC_SIZES and [tuple(l.shape) for l in got["labels"]] == cn.DISC_SIZES
    if want_u8:
        assert [tuple(p.shape) for p in got["seg_u8"]] == [(2, 3, 41, 50), (0, 3, 23, 37), (3, 3, 40, 48)]
        for p, w in zip(got["seg_u8"], want["seg_u8"]):
            assert torch.equal(p.cpu(), torch.from_numpy(w))
    else:
        assert got["seg_u8"] is None
    assert not got["labels"][1].any() and (got["labels"][2] == lab[2]).any()       # the empty query; the tie's winner


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_op_without_ground_truth_or_area(ops, flags):
    x, lab, nlabels, gts, kw, want = _disc_ref("class_ids", flags, False)
    tab = _tab(cn.DISC_OFF, lab)
    got = ops.seg_labels_cand_native(x.cuda(), _targets(cn.DISC_SIZES), tab.cuda(), tab, nlabels, **flags)
    assert got["counts"] is None and got["area"] is None
    for g, w in zip(got["labels"], want["labels"]):
        assert torch.equal(g.cpu(), torch.from_numpy(w))
    assert torch.equal(got["mx"].cpu(), torch.from_numpy(want["mx"]))


# ------------------------------------------------------------------------------------------------ 2. full lists
@pytest.mark.parametrize("ids", [None, [5, 200, 5, 77]], ids=["labelmaps", "class_ids"])
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_full_lists_equal_seg_labels_native(ops, flags, ids):
    """off = (0, N, 2N, ...), lab = 1 + c, seg_u8 permuted from class-major: ops.seg_labels_native(batch_max=False) bit for
    bit -- labels, counts and mx (permuted) -- on nway_native_ref's discriminating input."""
    x = nn.discriminating_input().cuda()
    N, B = x.shape[:2]
    rng = np.random.default_rng(3)
    gts = [rng.choice(np.array([0, 1, 2, 3, 4, 5, 77, 200, 255], np.uint8), size=s) for s in nn.DISC_SIZES]
    a = ops.seg_labels_native(x, _targets(nn.DISC_SIZES, gts), batch_max=False, class_ids=ids, **flags)
    ent = x.transpose(0, 1).contiguous().view(B * N, *x.shape[2:])
    tab = _tab([q * N for q in range(B + 1)], [1 + c for _ in range(B) for c in range(N)])
    b = ops.seg_labels_cand_native(ent, _targets(nn.DISC_SIZES, gts), tab.cuda(), tab, N, class_ids=ids, **flags)
    for la, lb in zip(a["labels"], b["labels"]):
        assert torch.equal(la, lb)
    assert torch.equal(a["counts"], b["counts"]) and torch.equal(a["mx"].t().contiguous().view(-1), b["mx"])
    assert int(a["counts"][:, 0, 1:].sum()) > 0
    if ids is not None:       # every class is a candidate: entry_ids says the same
        e = ops.seg_labels_cand_native(ent, _targets(nn.DISC_SIZES, gts), tab.cuda(), tab, N,
                                       entry_ids=[ids[c] for _ in range(B) for c in range(N)], **flags)
        assert torch.equal(e["counts"], a["counts"])


# ------------------------------------------------------------------------------------------------ 3. equal sizes
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_equal_sizes_equal_seg_labels_cand(ops, flags):
    """Every native size = (Hs, Ws): the bicubic taps at scale 1 fall on integer distances, where the kernel is 1 at 0 and 0
    elsewhere, so the resize is the identity and labels, counts and area are ops.seg_labels_cand's bit for bit."""
    x = cn.discriminating_input().cuda()
    lab, nlabels, _ = cn.disc_tables("set")
    tab = _tab(cn.DISC_OFF, lab)
    rng = np.random.default_rng(5)
    gt = rng.choice(np.array([0, 1, 2, 3, 4, 77, 255], np.uint8), size=(3,) + cn.DISC_SRC)
    mx = x.view(cn.DISC_E_CAP, -1).max(1).values.to(torch.int32)
    l0, c0, a0 = ops.seg_labels_cand(x, mx, tab.cuda(), tab, nlabels, torch.from_numpy(gt).cuda(), want_area=True, **flags)
    t = _targets([cn.DISC_SRC] * 3, list(gt), ignore=255)
    n = ops.seg_labels_cand_native(x, t, tab.cuda(), tab, nlabels, want_area=True, want_u8=True, **flags)
    assert torch.equal(torch.stack(n["labels"]), l0) and torch.equal(n["counts"], c0) and torch.equal(n["area"], a0)
    assert torch.equal(n["mx"][:cn.DISC_E], mx[:cn.DISC_E]) and not n["mx"][cn.DISC_E:].any()
    for q in range(3):
        assert torch.equal(n["seg_u8"][q], x[cn.DISC_OFF[q]:cn.DISC_OFF[q + 1]])
    assert int(c0[:, 0, 1:].sum()) > 0


# ------------------------------------------------------------------------------------------------ 4. table edits
def _writable(total, regions):
    m = torch.zeros(total, dtype=torch.bool)
    for o, n in regions:
        m[o:o + n] = True
    return m


EDITS = {
    "out-of-order": [0, 5, 1, 3],                       # offsets decrease
    "range-300": [0, 300, 300, 300],                    # one query claims 300 entries
    "end-past-E_cap": [0, 2, 2, 400],                   # off[B] > E_cap
    "negative": [-7, -2, 1 << 30, -(1 << 31)],
}


@pytest.mark.parametrize("edit", list(EDITS))
def test_table_rewritten_after_validation_stays_inside_its_buffers(ops, edit):
    """The device table differs from the host mirror the call validated (E_cap = 264, so that a range above 254 fits the
    table).  What the kernels read they clamp -- query inside 0..B-1, position inside 0..K-1, ranges inside E_cap and
    254 -- so the numbers are wrong but the run finishes and every byte outside the (position, image) regions of tmp /
    out_u8 / labels keeps its 0xA5: 64 guard bytes after every image, 256 around every buffer.  Inputs are unchanged."""
    E_cap, PAD = 264, 256
    x = torch.full((E_cap, 3) + cn.DISC_SRC, 255, dtype=torch.uint8)
    x[:cn.DISC_E] = cn.discriminating_input()[:cn.DISC_E]
    lab = cn.disc_tables("set")[0][:cn.DISC_E] + [0] * (E_cap - cn.DISC_E)
    gts = cn.disc_gts("ids")
    t = _targets(cn.DISC_SIZES, gts, guard=64)
    K, Hs = 3, cn.DISC_SRC[0]
    host = _tab(cn.DISC_OFF, lab)
    dev_words = host.clone()
    dev_words[:4] = torch.tensor(EDITS[edit], dtype=torch.int64).to(torch.int32)
    dev_words[4:] = torch.arange(E_cap, dtype=torch.int32) * 37 - 900          # labels of every kind, negative included
    tab = dev_words.cuda()
    n_tmp, n_u8, n_lab = K * t.tmp_bytes, K * t.u8_bytes, t.pred_bytes
    bufs = {k: torch.full((n + 2 * PAD,), GUARD, dtype=torch.uint8, device="cuda") for k, n in
            (("tmp", n_tmp), ("u8", n_u8), ("labels", n_lab))}
    view = lambda k, n: bufs[k][PAD:PAD + n]
    d_x, dev_before = x.cuda(), t.dev.clone()
    got = ops.seg_labels_cand_native(d_x, t, tab, host, 4, class_ids=cn.DISC_CLASS_IDS, want_area=True, want_u8=True,
                                     tmp=view("tmp", n_tmp), u8_out=view("u8", n_u8), labels_out=view("labels", n_lab))
    torch.cuda.synchronize()                                                    # it finishes
    regions = dict(
        tmp=[(PAD + k * t.tmp_bytes + it.tmp_off, 3 * Hs * it.w) for k in range(K) for it in t.items],
        u8=[(PAD + k * t.u8_bytes + it.u8_off, 3 * it.h * it.w) for k in range(K) for it in t.items],
        labels=[(PAD + it.pred_off, it.h * it.w) for it in t.items])
    for k, b in bufs.items():
        keep = ~_writable(b.numel(), regions[k])
        assert keep.sum() >= 2 * PAD and bool((b.cpu()[keep] == GUARD).all()), (edit, k)
    assert torch.equal(d_x.cpu(), x) and torch.equal(tab.cpu(), dev_words) and torch.equal(t.dev, dev_before)
    assert got["counts"].shape == (3, 2, 5) and got["area"].shape == (E_cap, 2) and got["mx"].shape == (E_cap,)
    assert int(got["counts"].min()) >= 0 and int(got["area"].min()) >= 0
    # the same buffers with the table the host saw: the reference's numbers, and the guards again
    tab.copy_(host)
    good = ops.seg_labels_cand_native(d_x, t, tab, host, 4, class_ids=cn.DISC_CLASS_IDS, want_area=True, want_u8=True,
                                      tmp=view("tmp", n_tmp), u8_out=view("u8", n_u8), labels_out=view("labels", n_lab))
    torch.cuda.synchronize()
    want = _disc_ref("class_ids", FLAGS[0], False)[-1]
    for g, w in zip(good["labels"], want["labels"]):
        assert torch.equal(g.cpu(), torch.from_numpy(w))
    assert torch.equal(good["counts"].cpu(), torch.from_numpy(want["counts"]))
    assert torch.equal(good["area"][:8].cpu(), torch.from_numpy(want["area"])) and not good["area"][8:].any()
    for k, b in bufs.items():
        assert bool((b.cpu()[~_writable(b.numel(), regions[k])] == GUARD).all()), (edit, k, "second run")


# ------------------------------------------------------------------------------------------------ 5. padding
def test_padding_entries_influence_nothing(ops):
    """Padding planes of 255 (the discriminating input's) against padding planes of other bytes and other labels in the
    table's padding: the same labels, counts, area and maxima; area and mx rows e >= E stay 0."""
    x, lab, nlabels, gts, kw, want = _disc_ref("class_ids", FLAGS[0], False)
    assert bool((x[cn.DISC_E:] == 255).all())
    outs = []
    for fill, tail in ((None, [0, 0, 0]), (9, [4, 1, 2])):
        y = x.clone()
        if fill is not None:
            y[cn.DISC_E:] = fill
        host = _tab(cn.DISC_OFF, lab[:cn.DISC_E] + [0, 0, 0])                  # the mirror is validated: padding labels 0 ...
        dev = _tab(cn.DISC_OFF, lab[:cn.DISC_E] + tail).cuda()                 # ... whatever the device holds there
        outs.append(ops.seg_labels_cand_native(y.cuda(), _targets(cn.DISC_SIZES, gts), dev, host, nlabels, want_area=True, **kw))
    for o in outs:
        _same(o, want)
        assert not o["area"][cn.DISC_E:].any() and not o["mx"][cn.DISC_E:].any()


# ------------------------------------------------------------------------------------------------ 6. pipeline
NATIVE_SIZES = [(70, 90), (64, 64), (50, 61)]
SET_IDS = [9, 3, 7]


def _native_gts(sizes, seed, dtype=np.uint8):
    rs = np.random.RandomState(seed)
    out = []
    for h, w in sizes:
        g = rs.choice([0, 9, 9, 3, 7, 40], size=(h, w)).astype(dtype)
        g[rs.rand(h, w) < 0.07] = 255
        out.append(g)
    return out


def _eq(a, b):
    return (a is None and b is None) or torch.equal(a, b)


def _native_same(a, b):
    assert set(a) == set(b) == {"labels", "counts", "area", "mx", "sizes"}
    assert a["sizes"] == b["sizes"] and len(a["labels"]) == len(b["labels"])
    for x, y in zip(a["labels"], b["labels"]):
        assert torch.equal(x, y)
    for k in ("counts", "area", "mx"):
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("labels", ["set", "local"])
def test_segment_candidates_native_is_the_op_on_its_own_seg_u8(models, ops, labels):
    pipe = models["pipe"]
    bankset = _library(pipe, "ragged", 1000)
    qry = _queries(B_Q, RES, seed=1010).cuda()
    gts = _native_gts(NATIVE_SIZES, 7)
    plain = pipe.segment_candidates(bankset, qry, CAND, entry_batch=4, labels=labels, captured=False)
    plain = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in plain.items()}
    assert set(plain) == set(KEYS) | {"entries", "offsets"}
    r = pipe.segment_candidates_native(bankset, qry, CAND, _targets(NATIVE_SIZES, gts, src=(RES, RES)), SET_IDS,
                                       entry_batch=4, labels=labels, captured=False)
    assert set(r) == set(plain) | {"native"}
    for k in plain:                                                  # nothing else changes
        assert _eq(r[k], plain[k]) if k in KEYS else r[k] == plain[k], k
    ct = bankset.candidate_tables(CAND, 4, labels)
    E, nlabels = ct["E"], ct["nlabels"]
    tab = torch.cat([ct["tab"][:B_Q + 1], ct["tab"][B_Q + 1:B_Q + 1 + E]])           # E_cap = E: the padding dropped
    entry_ids = [SET_IDS[c] for c in ct["entry_sets"][:E].tolist()]
    kw = dict(class_ids=SET_IDS) if labels == "set" else dict(entry_ids=entry_ids)
    op = ops.seg_labels_cand_native(r["seg_u8"].contiguous(), _targets(NATIVE_SIZES, gts, src=(RES, RES)), tab.cuda(), tab,
                                    nlabels, want_area=True, **kw)
    n = r["native"]
    assert n["area"].shape == (E, 2) and n["mx"].shape == (E,) and n["counts"].shape == (B_Q, 2, nlabels + 1)
    _native_same(n, {k: op[k] for k in n})
    want = cn.cand_native_ref(r["seg_u8"].cpu(), r["offsets"], tab[B_Q + 1:].tolist(), nlabels, NATIVE_SIZES, gts,
                              ignore_value=cn.DISC_IGNORE, **kw)
    _same(n, want)
    assert int(n["counts"][:, 1, 1:].sum()) > 0
    with pytest.raises(ValueError):                                  # no targets
        pipe.segment_candidates_native(bankset, qry, CAND, None, SET_IDS, entry_batch=4, captured=False)
    with pytest.raises(ValueError):                                  # one id per set
        pipe.segment_candidates_native(bankset, qry, CAND, _targets(NATIVE_SIZES, gts, src=(RES, RES)), SET_IDS[:2],
                                       entry_batch=4, captured=False)


def test_segment_candidates_native_captured_equals_eager(models):
    """Eager and captured agree on `native` and on everything else, for two candidate assignments, and `native` adds no
    graph and is in no key: the count of graphs is what the same calls without `native` leave."""
    pipe = models["pipe"]
    pipe._graphs = {}
    bankset = _library(pipe, "ragged", 1040)
    gts = _native_gts(NATIVE_SIZES, 8, np.int64)
    try:
        for n, cand in enumerate((CAND, ((1, 2), (), (2, 0, 1)))):
            qry = _queries(B_Q, RES, 1050 + n).cuda()
            tg = lambda: _targets(NATIVE_SIZES, gts, src=(RES, RES))
            e = pipe.segment_candidates_native(bankset, qry, cand, tg(), SET_IDS, entry_batch=4, captured=False)
            e = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in e.items()}
            c = pipe.segment_candidates_native(bankset, qry, cand, tg(), SET_IDS, entry_batch=4, captured=True)
            for k in KEYS:
                assert _eq(e[k], c[k]), (cand, k)
            _native_same(e["native"], c["native"])
            assert len(pipe._graphs) == 1
            keys = list(pipe._graphs)
            p = pipe.segment_candidates(bankset, qry, cand, entry_batch=4, captured=True)      # the same graph without native
            assert list(pipe._graphs) == keys and "native" not in p
            for k in KEYS:
                assert _eq(p[k], c[k]), (cand, k)
        assert not e["native"]["labels"][1].any()                        # the query without candidates
    finally:
        pipe._graphs = {}


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_stream_and_evaluate_candidates_native(models, captured):
    """segment_stream(candidates=, native=True, class_ids=) over five ragged queries in batches of three (the last one
    short): per batch the dict of segment_candidates_native on the hand-built batch with hand-built NativeTargets;
    evaluate_candidates(use_original_imgsize=True) over the same batches returns the summed native counts and
    metrics.nway_iou of them.  Without native=True the stream's dicts have no `native`."""
    from diffews_amd import evaluate
    from diffews_amd.input_pipeline import DeviceImageTransform
    from diffews_amd.metrics import nway_iou
    pipe = models["pipe"]
    pipe._graphs = {}
    try:
        bankset = _library(pipe, "ragged", 1060)
        tf = DeviceImageTransform(RES)
        qs = ql._host_queries(5, seed=61, with_gt=True)
        lists = [(2, 0), (1,), (0, 1, 2), (1, 2), (0,)]
        for q, cs in zip(qs, lists):
            q["cand"] = cs
        kw = dict(batch=3, size=RES, depth=1, entry_batch=4, captured=captured, ignore_value=255)
        got = []
        for index, r in pipe.segment_stream(bankset, qs, candidates="cand", native=True, class_ids=ql.CLASS_IDS, **kw):
            assert set(r) == set(KEYS) | {"entries", "offsets", "candidates", "native"}
            n = r["native"]
            got.append((index, r["candidates"], dict(labels=[l.clone() for l in n["labels"]], counts=n["counts"].clone(),
                                                     area=n["area"].clone(), mx=n["mx"].clone(), sizes=n["sizes"])))
        assert [g[0] for g in got] == [[0, 1, 2], [3, 4]]
        items, total = [], torch.zeros(2, 4, dtype=torch.int64, device=pipe.device)
        for index, cands, out in got:
            qry = torch.stack([tf.image(qs[i]["query_img"]) for i in index])
            sizes = [qs[i]["query_img"].shape[:2] for i in index]
            assert out["sizes"] == [tuple(s) for s in sizes]
            tg = lambda: _targets(sizes, [qs[i]["gt"] for i in index], src=(RES, RES))
            r = pipe.segment_candidates_native(bankset, qry, cands, tg(), ql.CLASS_IDS, entry_batch=4, captured=captured)
            _native_same(out, r["native"])
            total += r["native"]["counts"].sum(0)
            items.append((qry, cands, tg()))
        assert int(total[0, 1:].sum()) >= 0 and int(total[1, 1:].sum()) > 0
        miou, iou, counts = evaluate.evaluate_candidates(pipe, bankset, items, entry_batch=4, captured=captured,
                                                         use_original_imgsize=True, class_ids=ql.CLASS_IDS)
        assert counts.dtype == torch.int64 and torch.equal(counts, total)
        want_iou, want_miou = nway_iou(total)
        assert miou == want_miou and torch.equal(iou, want_iou)
        index, r = next(pipe.segment_stream(bankset, qs, candidates="cand", **kw))
        assert "native" not in r and set(r) == set(KEYS) | {"entries", "offsets", "candidates"}
        with pytest.raises(ValueError):
            next(pipe.segment_stream(bankset, qs, candidates="cand", class_ids=ql.CLASS_IDS, **kw))
    finally:
        pipe._graphs = {}
