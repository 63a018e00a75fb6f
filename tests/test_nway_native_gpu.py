"""GPU tests of N-way labels and counts at native size (ops.seg_labels_native, dfw_seg_labels_native) against
tests/nway_native_ref.py -- Pillow's own resize, nway_ref's fp32 expressions: every comparison is torch.equal.  Ragged
batches, 0xA5 guards around every (class, image) region, the three thresholding modes, the three ground-truth forms, N = 1
against ops.seg_native, a fixed launch count, segment_classes(native=) eager and captured on the tiny pipeline, and
evaluate_class_set under use_original_imgsize."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import nway_native_ref as nn
from test_native_gpu import MODES, models, ops, _support_set  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SOURCES = [(32, 32), (40, 72)]
PAIR = [(41, 50), (23, 37)]
RAGGED = [(97, 131), (23, 37), (64, 50), (64, 64), (24, 40)]     # odd widths, w % 4 == 0 and == 2, up, down, identity size
SINGLE = [(1, 7)]
CLASSES = [1, 3, 4]
FORMS = ["labels", "ids8", "ids32"]
IDS = {"ids8": [7, 3, 9, 7], "ids32": [7, 1000, 9, 7]}           # class 3 repeats class 0's id: the lowest class is meant

CASES = [(N, src, tuple(sizes)) for N in CLASSES for src in SOURCES for sizes in (PAIR, RAGGED, SINGLE)]
CASE_IDS = [f"N{N}-{s[0]}x{s[1]}-b{len(z)}" for N, s, z in CASES]


@functools.lru_cache(maxsize=None)
def _input(N, src, sizes):
    """uint8 [N, b, 3, Hs, Ws] on the host.  (32, 32) with the two-image batch: the first N classes of the discriminating
    input.  Otherwise noise whose level differs per class and image under a ramp (so maxima, thresholds and the winning
    class all vary); with N >= 3 class 1 is all zero."""
    if src == nn.DISC_SRC and list(sizes) == nn.DISC_SIZES:
        return nn.discriminating_input()[:N].contiguous()
    b = len(sizes)
    g = torch.Generator().manual_seed(1000 * N + 10 * src[1] + b)
    lvl = 0.5 + 0.5 * torch.rand(N, b, 1, 1, 1, generator=g)
    ramp = torch.linspace(0.0, 1.0, src[0] * src[1]).view(1, 1, 1, *src)
    x = (torch.rand(N, b, 3, *src, generator=g) * lvl * (0.15 + 0.85 * ramp) * 255).to(torch.uint8)
    if N >= 3:
        x[1] = 0
    return x


@functools.lru_cache(maxsize=None)
def _resized(N, src, sizes):
    """Pillow's resize of every (class, image) of the case, computed once and shared (never written)."""
    return nn.resized(_input(N, src, sizes), sizes)


def _gts(N, sizes, form, seed=0):
    """Ground truth per query.  'labels': uint8 0..N, some N + 1 (above N: dropped) and 255.  'ids8' / 'ids32': class-id maps
    for IDS[form] -- ids of the table, ids outside it (40; -5 and 70000 in int32) and 255."""
    rs = np.random.RandomState(17 + seed + N)
    out = []
    for h, w in sizes:
        if form == "labels":
            g = rs.randint(0, N + 2, size=(h, w)).astype(np.uint8)
        elif form == "ids8":
            g = rs.choice([0, 3, 7, 9, 40], size=(h, w)).astype(np.uint8)
        else:
            g = rs.choice([0, 7, 9, 1000, 40, -5, 70000], size=(h, w)).astype(np.int32)
        g[rs.rand(h, w) < 0.07] = 255
        out.append(g)
    return out


def _ids(N, form):
    return None if form == "labels" else IDS[form][:N]


def _same(r, ref, what):
    for i, want in enumerate(ref["labels"]):
        got = r["labels"][i].cpu()
        assert got.shape == want.shape and torch.equal(got, want), (what, i, int((got != want).sum()))
    assert r["mx"].dtype == torch.int32 and torch.equal(r["mx"].cpu(), ref["mx"]), (what, r["mx"].tolist(), ref["mx"].tolist())
    if ref["counts"] is None:
        assert r["counts"] is None, what
    else:
        assert r["counts"].dtype == torch.int64 and torch.equal(r["counts"].cpu(), ref["counts"]), \
            (what, r["counts"].tolist(), ref["counts"].tolist())


@pytest.mark.parametrize("N,src,sizes", CASES, ids=CASE_IDS)
def test_labels_mx_counts_equal_reference(ops, N, src, sizes):
    """labels, mx and counts == nway_native_ref in the three threshold modes, for ground truth as uint8 labels, uint8 class-id
    map + class_ids and int32 class-id map + class_ids, ignore_value 255 and -1; without ground truth counts is None.  An
    all-zero class never labels a pixel; on the discriminating input label 4 never appears while label 1 does."""
    from diffews_amd.input_pipeline import NativeTargets
    x = _input(N, src, sizes)
    xd = x.cuda()
    sizes = list(sizes)
    res = _resized(N, src, tuple(sizes))
    disc = src == nn.DISC_SRC and sizes == nn.DISC_SIZES
    for form in FORMS:
        gts, ids = _gts(N, sizes, form), _ids(N, form)
        for ign in (255, -1):
            t = NativeTargets(src, sizes, gt=gts, ignore_value=ign)
            for mode in MODES:
                r = ops.seg_labels_native(xd, t, *mode, class_ids=ids)
                ref = nn.nway_native_ref(x, sizes, gts, ids, ign, *mode, res=res)
                _same(r, ref, (form, ign, mode))
                assert r["seg_u8"] is None and r["sizes"] == sizes
                for lab in r["labels"]:
                    if N >= 3 and not disc:
                        assert not bool((lab == 2).any())
                    if disc and N == 4:
                        assert not bool((lab == 4).any()) and bool((lab == 1).any())
    r = ops.seg_labels_native(xd, NativeTargets(src, sizes), 0.25, 0.0, False)
    _same(r, nn.nway_native_ref(x, sizes, res=res), "no gt")


@pytest.mark.parametrize("N,src,sizes", CASES, ids=CASE_IDS)
def test_resized_bytes_and_guards(ops, N, src, sizes):
    """want_u8: the resized bytes of every (class, image) == Pillow's.  tmp, labels and out_u8 are pre-filled with 0xA5 and
    laid out with 64 guard bytes after every image: no byte outside a (class, image) region is written, and the views are
    views of the caller's buffers.  Without want_u8 (the bytes staged behind tmp) labels and maxima are the same."""
    from diffews_amd.input_pipeline import NativeTargets
    sizes = list(sizes)
    x = _input(N, src, tuple(sizes)).cuda()
    t = NativeTargets(src, sizes, guard=64)
    fill = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    u8, lab, tmp = fill(N * t.u8_bytes), fill(t.pred_bytes), fill(N * t.tmp_bytes)
    r = ops.seg_labels_native(x, t, 0.25, 0.0, False, want_u8=True, labels_out=lab, u8_out=u8, tmp=tmp)
    res = _resized(N, src, tuple(sizes))
    for i, (h, w) in enumerate(sizes):
        assert r["seg_u8"][i].shape == (N, 3, h, w) and r["labels"][i].shape == (h, w)
        want = torch.stack([res[c][i] for c in range(N)])
        assert torch.equal(r["seg_u8"][i].cpu(), want), (i, h, w, int((r["seg_u8"][i].cpu() != want).sum()))
    for buf, stride, offs, per, ncls in (
            (u8.cpu(), t.u8_bytes, [it.u8_off for it in t.items], [3 * h * w for h, w in sizes], N),
            (lab.cpu(), 0, [it.pred_off for it in t.items], [h * w for h, w in sizes], 1),
            (tmp.cpu(), t.tmp_bytes, [it.tmp_off for it in t.items], [3 * src[0] * w for _, w in sizes], N)):
        inside = torch.zeros(buf.numel(), dtype=torch.bool)
        for c in range(ncls):
            ends = [c * stride + o for o in offs[1:]] + [(c + 1) * stride if stride else buf.numel()]
            for o, n, e in zip(offs, per, ends):
                assert e - (c * stride + o + n) >= 64
                inside[c * stride + o:c * stride + o + n] = True
        assert bool((buf[~inside] == 0xA5).all()), int((buf[~inside] != 0xA5).sum())
        assert not bool((buf[inside] == 0xA5).all())
    assert r["seg_u8"][0].data_ptr() == u8.data_ptr() + t.items[0].u8_off
    assert r["labels"][-1].data_ptr() == lab.data_ptr() + t.items[-1].pred_off
    r2 = ops.seg_labels_native(x, t, 0.25, 0.0, False)
    assert r2["seg_u8"] is None and torch.equal(r2["mx"], r["mx"])
    for a, b_ in zip(r2["labels"], r["labels"]):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("src,sizes", [(s, z) for s in SOURCES for z in (PAIR, RAGGED, SINGLE)],
                         ids=[f"{s[0]}x{s[1]}-b{len(z)}" for s in SOURCES for z in (PAIR, RAGGED, SINGLE)])
def test_one_class_is_seg_native(ops, src, sizes):
    """N = 1 on the device, 0/1/255 masks, ignore_value 255: labels[i] == ops.seg_native's pred[i] and counts.view(b, 4) its
    counts, in the three modes."""
    from diffews_amd.input_pipeline import NativeTargets
    x = _input(1, src, tuple(sizes)).cuda()
    rs = np.random.RandomState(5)
    gts = []
    for h, w in sizes:
        m = (rs.rand(h, w) > 0.5).astype(np.uint8)
        m[rs.rand(h, w) < 0.07] = 255
        gts.append(m)
    t = NativeTargets(src, sizes, gt=gts, class_value=1, ignore_value=255)
    for mode in MODES:
        want = ops.seg_native(x[0], t, *mode)
        got = ops.seg_labels_native(x, t, *mode)
        for a, b_ in zip(got["labels"], want["pred"]):
            assert torch.equal(a, b_), mode
        assert torch.equal(got["counts"].view(len(sizes), 4), want["counts"]), mode
        assert torch.equal(got["mx"][0], want["mx"]), mode


def test_four_launches_whatever_n_and_b(ops, hip_lib):
    """Captured with (N, b) = (1, 1) and (4, 5): 4 nodes both times (zero, horizontal, vertical + maximum, label + count),
    none of them a memset node; a replay equals eager."""
    from diffews_amd.input_pipeline import NativeTargets
    nodes = []
    for N, sizes in ((1, RAGGED[:1]), (4, RAGGED)):
        x = _input(N, (40, 72), tuple(sizes)).cuda()
        gts = _gts(N, sizes, "ids8")
        ids = torch.tensor(_ids(N, "ids8"), dtype=torch.int32, device="cuda")
        t = NativeTargets((40, 72), sizes, gt=gts, ignore_value=255)
        eager = ops.seg_labels_native(x, t, class_ids=ids, want_u8=True)      # also warms the allocator
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = ops.seg_labels_native(x, t, class_ids=ids, want_u8=True)
        n = C.c_int32(0)
        assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(n)) == 0
        nodes.append(n.value)
        graph.instantiate()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["counts"], eager["counts"]) and torch.equal(out["mx"], eager["mx"])
        for a, b_ in zip(out["labels"] + out["seg_u8"], eager["labels"] + eager["seg_u8"]):
            assert torch.equal(a, b_)
    assert nodes[0] == nodes[1] == 4, nodes


def test_bad_arguments_raise(ops):
    from diffews_amd.input_pipeline import NativeTargets
    x = _input(3, (32, 32), tuple(PAIR)).cuda()
    with pytest.raises(ValueError, match="targets were built"):
        ops.seg_labels_native(x, NativeTargets((32, 32), RAGGED))
    with pytest.raises(ValueError, match="class_ids"):
        ops.seg_labels_native(x, NativeTargets((32, 32), PAIR), class_ids=[1, 2])


# ------------------------------------------------------------------------------------------------ the tiny pipeline

N_CLS, RES = 3, 64
CLASS_IDS = [7, 3, 9]


def _classes(s, seed):
    sets = [_support_set(s, RES, seed=seed + 10 * c) for c in range(N_CLS)]
    return torch.stack([a for a, _ in sets]).cuda(), torch.stack([m for _, m in sets]).cuda()


def _queries(b, seed):
    return (torch.rand(b, 3, RES, RES, generator=torch.Generator().manual_seed(seed)) * 2 - 1).cuda()


def _check_native(r, sizes, gts, ids, ign, flags):
    ref = nn.nway_native_ref(r["seg_u8"].cpu(), sizes, gts, ids, ign, *flags)
    _same(r["native"], ref, (sizes, flags))
    return ref


def test_segment_classes_native(models):
    """segment_classes(..., native=t): z0, dec, seg_u8, labels and counts are bit-equal to the call without `native`;
    r["native"] == nway_native_ref(r["seg_u8"]) exactly; captured equals eager; a second batch of other native sizes reuses
    the captured graph (the stage is outside the graph and its key)."""
    from diffews_amd.input_pipeline import NativeTargets
    pipe = models["pipe"]
    pipe._graphs = {}
    b = 2
    bankset = pipe.prepare_support_classes(*_classes(1, seed=600))
    gt = torch.randint(0, N_CLS + 1, (b, RES, RES), generator=torch.Generator().manual_seed(2)).to(torch.uint8).cuda()
    clone = lambda r: {k: v.clone() for k, v in r.items()}
    cached = []
    flags = MODES[0]
    for sizes, seed in (([(48, 64), (97, 131)], 61), ([(80, 56), (64, 64)], 62)):
        qry = _queries(b, seed)
        gts = _gts(N_CLS, sizes, "ids8", seed)
        t = NativeTargets((RES, RES), sizes, gt=gts, ignore_value=255)
        eager = None
        for captured in (False, True):
            plain = clone(pipe.segment_classes(bankset, qry, gt, captured=captured))
            assert set(plain) == {"z0", "dec", "seg_u8", "labels", "counts"}
            r = pipe.segment_classes(bankset, qry, gt, captured=captured, native=t, class_ids=CLASS_IDS)
            assert set(r) == set(plain) | {"native"}
            for k in plain:
                assert torch.equal(plain[k], r[k]), (captured, k)
            _check_native(r, sizes, gts, CLASS_IDS, 255, flags)
            if eager is None:
                eager = r
                continue
            assert torch.equal(eager["seg_u8"], r["seg_u8"])
            assert torch.equal(eager["native"]["counts"], r["native"]["counts"])
            for a, b_ in zip(eager["native"]["labels"], r["native"]["labels"]):
                assert torch.equal(a, b_)
        cached.append(len(pipe._graphs))
    assert cached == [1, 1]                  # native sizes are not part of the key: the second batch replays the first graph
    # the call's flags reach the native stage
    t = NativeTargets((RES, RES), [(48, 64), (97, 131)], gt=_gts(N_CLS, [(48, 64), (97, 131)], "labels"), ignore_value=255)
    for flags in (MODES[1], MODES[2]):
        r = pipe.segment_classes(bankset, _queries(b, 63), None, *flags, captured=False, native=t)
        assert r["counts"] is None
        _check_native(r, t.sizes, _gts(N_CLS, t.sizes, "labels"), None, 255, flags)
    pipe._graphs = {}


def test_evaluate_class_set_at_native_size(models):
    """Two batches of different b and native sizes through evaluate_class_set(use_original_imgsize=True, class_ids=...):
    the totals are the summed reference counts on the pipeline's own seg_u8 (recorded per step)."""
    from diffews_amd import evaluate
    from diffews_amd.input_pipeline import NativeTargets
    from diffews_amd.metrics import nway_iou
    pipe = models["pipe"]
    pipe._graphs = {}
    sup, msk = _classes(1, seed=700)
    plan = [([(48, 64), (97, 131)], 71), ([(80, 56), (64, 64), (23, 37)], 72)]
    batches, truth = [], []
    for sizes, seed in plan:
        gts = _gts(N_CLS, sizes, "ids32", seed)
        batches.append((_queries(len(sizes), seed), NativeTargets((RES, RES), sizes, gt=gts, ignore_value=255)))
        truth.append((sizes, gts))
    seen, inner = [], pipe.segment_classes

    def recording(*a, **kw):
        r = inner(*a, **kw)
        seen.append(r["seg_u8"].clone().cpu())
        return r
    pipe.segment_classes = recording
    ids = [7, 1000, 9]
    try:
        miou, iou, total = evaluate.evaluate_class_set(pipe, sup, msk, batches, use_original_imgsize=True, class_ids=ids)
    finally:
        del pipe.segment_classes
        pipe._graphs = {}
    assert len(seen) == 2
    want = torch.zeros(2, N_CLS + 1, dtype=torch.int64)
    for seg, (sizes, gts) in zip(seen, truth):
        want += nn.nway_native_ref(seg, sizes, gts, ids, 255)["counts"].sum(0)
    assert total.dtype == torch.int64 and torch.equal(total.cpu(), want)
    assert int(want[1].sum()) > 0
    ref_iou, ref_miou = nway_iou(want)
    assert torch.equal(iou.cpu(), ref_iou)               # per label one IEEE multiplication and one division of exact integers
    # miou is a float64 mean of N_CLS values summed on the device: the order of the additions is the device's, each of the
    # N_CLS - 1 additions and the division rounds by at most 2^-53 relative on either side
    assert abs(float(miou) - float(ref_miou)) <= 2 * N_CLS * 2.0 ** -53 * float(ref_miou), (miou, ref_miou)
