"""CPU tests (no GPU) of candidate classes per query -- every query against a handful of a SupportBankSet's classes, fused
into one label map: the properties of the rule on the independent numpy reference (tests/cand_ref.py, which
tests/test_candidates_gpu.py holds the kernel to), SupportBankSet.candidate_tables on host tensors, and the C entry point
through the header, the ctypes table and its host-side validation (every error is returned before any launch)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cand_ref
import nway_ref

DFW_EINVAL, DFW_ERANGE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(rng, *shape):
    return rng.integers(0, 256, size=shape, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- the reference's properties
@pytest.mark.parametrize("flags", [dict(r_threshold=0.25), dict(r_threshold=0.0, threshold=0.4)])
def test_ref_equals_nway_on_full_lists(flags):
    """off = (0, N, 2N, ...), lab[qN + c] = 1 + c, seg_u8 / mx permuted from class-major to query-major: labels and counts
    are tests/nway_ref.py's (batch_max = False) on random bytes."""
    rng = np.random.default_rng(5)
    N, B, H, W = 3, 2, 7, 9
    u8 = _bytes(rng, N, B, 3, H, W)
    u8[1, 0] = u8[0, 0]                                           # a whole image of ties between classes 0 and 1
    gt = rng.choice(np.array([0, 1, 2, 3, 7, 255], np.uint8), size=(B, H, W))
    lab_n, cnt_n = nway_ref.seg_labels(torch.from_numpy(u8), torch.from_numpy(gt), flags.get("r_threshold", 0.25),
                                       flags.get("threshold", 0.0), False)
    ent = np.ascontiguousarray(u8.transpose(1, 0, 2, 3, 4)).reshape(B * N, 3, H, W)
    off, lab = [q * N for q in range(B + 1)], [1 + c for _ in range(B) for c in range(N)]
    labels, counts, area = cand_ref.seg_labels_cand(ent, cand_ref.maxima(ent), off, lab, N, gt, **flags)
    assert np.array_equal(labels, lab_n.numpy()) and np.array_equal(counts, cnt_n.numpy())
    assert (labels[0] != 2).all() and (labels[0] == 1).any()      # the tie went to the earlier entry everywhere


def test_ref_tie_empty_padding_and_missing_label():
    rng = np.random.default_rng(6)
    H, W = 5, 6
    plane = _bytes(rng, 3, H, W)
    plane[:, 0, 0] = 255
    # entries: query 0 -> (e0, e1) with equal planes; query 1 -> none; query 2 -> e2; e3 is padding
    u8 = np.stack([plane, plane, _bytes(rng, 3, H, W), _bytes(rng, 3, H, W)])
    off, lab = [0, 2, 2, 3], [4, 2, 3, 0]
    gt = np.zeros((3, H, W), np.uint8)
    gt[2, :2] = 1                                                 # label 1 is not among query 2's candidates (its only one is 3)
    mx = cand_ref.maxima(u8)
    labels, counts, area = cand_ref.seg_labels_cand(u8, mx, off, lab, 4, gt, r_threshold=0.25)
    assert set(np.unique(labels[0])) <= {0, 4} and (labels[0] == 4).any()     # earliest entry on a tie, never label 2
    assert area[1, 0] == area[0, 0] and area[1, 1] == 0 and area[0, 1] == area[0, 0]
    assert not labels[1].any() and counts[1, 0, 0] == H * W and counts[1, 1, 0] == H * W and counts[1, :, 1:].sum() == 0
    assert not area[3].any()                                      # padding rows stay 0 ...
    u8b, mxb = u8.copy(), mx.copy()
    u8b[3], mxb[3], lab2 = 255 - u8[3], 7, [4, 2, 3, 9]           # ... and nothing of a padding entry is looked at
    again = cand_ref.seg_labels_cand(u8b, mxb, off, lab2, 4, gt, r_threshold=0.25)
    assert all(np.array_equal(a, b) for a, b in zip((labels, counts, area), again))
    short = cand_ref.seg_labels_cand(u8[:3], mx[:3], off, lab[:3], 4, gt, r_threshold=0.25)
    assert np.array_equal(short[0], labels) and np.array_equal(short[1], counts) and np.array_equal(short[2], area[:3])
    # the gt label outside the candidates: in that label's union only (2 * W pixels), never in an intersection
    assert counts[2, 0, 1] == 0 and counts[2, 1, 1] == 2 * W
    assert counts[2, 1, 3] == (labels[2] == 3).sum() and counts[2, 0, 3] == 0
    # area: won <= foreground on its own, and a query's wins add up to its non-zero labels
    assert (area[:, 1] <= area[:, 0]).all()
    for q in range(3):
        assert area[off[q]:off[q + 1], 1].sum() == (labels[q] != 0).sum()
    # area does not depend on gt, ignore pixels included
    gt255 = np.full_like(gt, 255)
    l2, c2, a2 = cand_ref.seg_labels_cand(u8, mx, off, lab, 4, gt255, r_threshold=0.25)
    assert np.array_equal(a2, area) and np.array_equal(l2, labels) and not c2.any()
    assert np.array_equal(cand_ref.seg_labels_cand(u8, mx, off, lab, 4, None, r_threshold=0.25)[2], area)


# ---------------------------------------------------------------------------------------------- candidate_tables
def _sets(nsets=3, shots=(1, 3, 2)):
    from diffews_amd import config
    from diffews_amd.unet import SupportBankSet, bank_layout
    cfg = config.get("tiny_unet")
    dt, hw = torch.bfloat16, (8, 8)
    layout = bank_layout(cfg, *hw)
    n = sum(shots) if hasattr(shots, "__iter__") else nsets * shots
    kv = lambda: [torch.zeros(n, t, c, dtype=dt) for t, c in layout]
    return SupportBankSet(kv(), kv(), nsets, shots, hw, dt, dt, (1.0, "folded", 1), 1, layout)


def test_candidate_tables():
    ragged, uniform = _sets(), _sets(3, 2)
    cand = ((2, 0), (1,), (0, 2, 1))
    for eb, E_pad in ((1, 6), (3, 6), (8, 8), (4, 8)):
        t = ragged.candidate_tables(cand, eb)
        assert t["E"] == 6 and t["E_pad"] == E_pad and t["nlabels"] == 3
        assert t["sets"] == ((0, 2), (1,), (0, 1, 2))                           # sorted: the lowest class wins a tie
        pad = E_pad - 6
        assert t["entries"].dtype == torch.int64 and t["entries"].tolist() == [0, 0, 1, 2, 2, 2] + [2] * pad
        assert t["rows"].dtype == torch.int32 and t["rows"].is_contiguous() and tuple(t["rows"].shape) == (E_pad, 2)
        assert t["rows"].tolist() == [[0, 1], [4, 2], [1, 3], [0, 1], [1, 3], [4, 2]] + [[4, 2]] * pad
        assert t["tab"].dtype == torch.int32 and t["tab"].tolist() == [0, 2, 3, 6] + [1, 3, 2, 1, 2, 3] + [0] * pad
        for x in ("entries", "rows", "tab"):
            assert t[x].device.type == "cpu"
        for first, n in t["rows"].tolist():                                      # every row inside the stack, padding too
            assert first >= 0 and n >= 1 and first + n <= ragged.k[0].shape[0]
        rt = ragged.route_table([c for cs in t["sets"] for c in cs])
        assert torch.equal(t["rows"][:6], rt)
    t = uniform.candidate_tables(cand, 4)
    assert t["rows"].tolist() == [[0, 2], [4, 2], [2, 2], [0, 2], [2, 2], [4, 2], [4, 2], [4, 2]]
    # "local": 1 + position in the query's sorted list, nlabels = the longest list
    t = ragged.candidate_tables(((2,), (), (2, 1)), 2, labels="local")
    assert t["E"] == 3 and t["E_pad"] == 4 and t["nlabels"] == 2 and t["sets"] == ((2,), (), (1, 2))
    assert t["tab"].tolist() == [0, 1, 1, 3] + [1, 1, 2, 0] and t["entries"].tolist() == [0, 2, 2, 2]
    s = ragged.candidate_tables(((2,), (), (2, 1)), 2, labels="set")
    assert s["tab"].tolist() == [0, 1, 1, 3] + [3, 2, 3, 0] and s["nlabels"] == 3 and torch.equal(s["rows"], t["rows"])
    assert ragged.candidate_tables([torch.tensor([1, 0])], 1)["sets"] == ((0, 1),)
    for bad in (((0, 0),), ((1, 2, 1), (0,)), ((3,),), ((-1,), (0,)), ((), ()), (), ((0,), (0, 1, 99))):
        with pytest.raises(ValueError):
            ragged.candidate_tables(bad, 2)
    with pytest.raises(ValueError):
        ragged.candidate_tables(cand, 0)
    with pytest.raises(ValueError):
        ragged.candidate_tables(cand, 2, labels="global")


def test_candidate_tables_large_library():
    """More than 254 sets: labels='set' does not fit a byte and says to use 'local'; 'local' works, up to 254 candidates
    a query."""
    big = _sets(300, 1)
    with pytest.raises(ValueError, match="local"):
        big.candidate_tables(((299, 3),), 2)
    t = big.candidate_tables(((299, 3), (7,)), 2, labels="local")
    assert t["nlabels"] == 2 and t["tab"].tolist() == [0, 2, 3, 1, 2, 1, 0] and t["rows"].tolist()[:3] == [[3, 1], [299, 1], [7, 1]]
    assert big.candidate_tables((range(254),), 127, labels="local")["nlabels"] == 254
    with pytest.raises(ValueError, match="254"):
        big.candidate_tables((range(255),), 5, labels="local")


# ---------------------------------------------------------------------------------------------- ABI
def test_header_ctypes_and_symbol(hip_lib):
    from diffews_amd import _lib as L
    from diffews_amd import build
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int dfw_seg_labels_cand(const uint8_t* seg_u8, const uint32_t* mx, const int32_t* tab, const int32_t* tab_host, "
            "const uint8_t* gt, uint8_t* labels, int64_t* counts, int64_t* area, int32_t B, int32_t E_cap, int32_t nlabels, "
            "int32_t H, int32_t Wd, float r_threshold, float threshold, dfw_stream_t stream);") in flat
    i32, vp, f = C.c_int32, C.c_void_p, C.c_float
    assert L.SYMBOLS["dfw_seg_labels_cand"] == (i32, [vp, vp, vp, C.POINTER(i32), vp, vp, vp, vp, i32, i32, i32, i32, i32, f, f, vp])
    assert hip_lib.dfw_seg_labels_cand is not None
    assert hip_lib.dfw_version() >= 110
    assert "seg_candidates.hip" in build.SOURCES


def _tab(words):
    return (C.c_int32 * len(words))(*[int(w) for w in words])


def test_host_validation(hip_lib):
    """Every error of the entry point comes back from the loaded library on the host, before any launch (the device
    pointers are never dereferenced there), so this is safe without a GPU."""
    h = hip_lib
    P = 4096                                                   # stands for any device address
    good = [0, 2, 2, 5] + [3, 1, 2, 1, 3] + [0]                # B = 3, E = 5, E_cap = 6, nlabels = 3
    ok = dict(seg=P, mx=P, tab=P, host=good, gt=P, labels=P, counts=P, area=P, B=3, E_cap=6, nl=3, H=8, W=12, r=0.25, t=0.0)

    def call(**kw):
        a = dict(ok, **kw)
        host = None if a["host"] is None else _tab(a["host"])
        return h.dfw_seg_labels_cand(a["seg"], a["mx"], a["tab"], host, a["gt"], a["labels"], a["counts"], a["area"], a["B"],
                                     a["E_cap"], a["nl"], a["H"], a["W"], a["r"], a["t"], None)
    many = [0, 255, 255, 255] + [1] * 255 + [0]
    bad = [
        ("null seg_u8", dict(seg=None)), ("null tab", dict(tab=None)), ("null tab_host", dict(host=None)),
        ("null labels", dict(labels=None)),
        ("B 0", dict(B=0)), ("B < 0", dict(B=-1)), ("H 0", dict(H=0)), ("W 0", dict(W=0)), ("H < 0", dict(H=-8)),
        ("E_cap 0", dict(E_cap=0)), ("E_cap < 0", dict(E_cap=-6)),
        ("nlabels 0", dict(nl=0)), ("nlabels 255", dict(nl=255)), ("nlabels < 0", dict(nl=-1)),
        ("counts without gt", dict(gt=None)),
        ("dynamic threshold without mx", dict(mx=None)),
        ("no threshold", dict(r=0.0, t=0.0)), ("negative thresholds", dict(r=-1.0, t=-0.5)),
        ("offsets start above 0", dict(host=[1, 2, 2, 5] + good[4:])),
        ("offsets start below 0", dict(host=[-1, 2, 2, 5] + good[4:])),
        ("offsets decrease", dict(host=[0, 3, 2, 5] + good[4:])),
        ("offsets end above E_cap", dict(host=[0, 2, 2, 7] + good[4:])),
        ("offsets pass E_cap in the middle", dict(host=[0, 7, 7, 7] + good[4:])),
        ("255 entries in a query", dict(host=many, E_cap=256, nl=3)),
        ("label 0 below E", dict(host=good[:4] + [3, 0, 2, 1, 3, 0])),
        ("label above nlabels", dict(host=good[:4] + [3, 1, 4, 1, 3, 0])),
        ("label < 0", dict(host=good[:4] + [3, 1, 2, 1, -3, 0])),
        ("last real label bad", dict(host=good[:4] + [3, 1, 2, 1, 9, 0])),
    ]
    for what, kw in bad:
        assert call(**kw) == DFW_EINVAL, what
    assert call(B=65536) == DFW_ERANGE
    from diffews_amd import ops
    u8 = torch.zeros(6, 3, 8, 12, dtype=torch.uint8)
    mx = torch.zeros(6, dtype=torch.int32)
    t = torch.tensor(good, dtype=torch.int32)
    for tab, th in ((t[:9], t), (t.long(), t), (t, t.long()), (t[:1], t[:1]), (t.view(2, 5), t)):
        with pytest.raises(ValueError):                        # ops: both tables are contiguous int32 [B + 1 + E_cap]
            ops.seg_labels_cand(u8, mx, tab, th, 3)
    with pytest.raises(ValueError):                            # ops: the device table lives on the device
        ops.seg_labels_cand(u8, mx, t, t, 3)


def test_public_signatures():
    """The Python surface the issue names, argument for argument."""
    from diffews_amd import evaluate, ops
    from diffews_amd.input_pipeline import QueryLoader
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise as P
    from diffews_amd.unet import SupportBankSet
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(ops.seg_labels_cand) == ["seg_u8", "mx", "tab", "tab_host", "nlabels", "gt", "r_threshold", "threshold",
                                          "want_area", "labels_out", "counts_out"]
    assert names(SupportBankSet.candidate_tables) == ["self", "candidates", "entry_batch", "labels"]
    assert inspect.signature(SupportBankSet.candidate_tables).parameters["labels"].default == "set"
    assert names(P.segment_candidates) == ["self", "bankset", "query_img", "candidates", "query_labels", "r_threshold",
                                           "threshold", "entry_batch", "labels", "captured"]
    sig = inspect.signature(P.segment_candidates).parameters
    assert sig["entry_batch"].default == 8 and sig["labels"].default == "set" and "batch_max" not in sig
    sig = inspect.signature(P.segment_stream).parameters
    assert "candidates" in sig and sig["candidates"].default is None
    assert "candidates" in inspect.signature(QueryLoader.__init__).parameters
    assert names(evaluate.evaluate_candidates)[:3] == ["pipe", "library", "items"]
