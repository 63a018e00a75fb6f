"""CPU tests of the score stage and of what sits on it: tests/scores_ref.py against a per-pixel loop, the C ABI of
dfw_seg_scores (struct mirror, sizeof, signatures, every refusal in its documented order on host memory -- validation
precedes any launch --, the workspace and block queries), the plane-table helpers against hand-written tables,
metrics.average_precision against a plain-loop reference and known answers, and objects.coco_results on a hand-made map.
All integers, and float64 quotients of the same integers on both sides: every comparison is exact."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import scores_ref as sr
from seg_args_cases import check_overlap_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ESHAPE, DFW_ERANGE, DFW_EWORKSPACE = -1, -2, -3, -4


def test_error_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    for name, v in (("DFW_EINVAL", DFW_EINVAL), ("DFW_ESHAPE", DFW_ESHAPE), ("DFW_EWORKSPACE", DFW_EWORKSPACE),
                    ("DFW_ERANGE", DFW_ERANGE)):
        assert re.search(name + r" = (-\d+)", hdr).group(1) == str(v), name


# ------------------------------------------------------------------------------------------------ the reference

def test_worked_example_of_the_header():
    ids, labels = [[1, 1, 2]], [[2, 2, 1]]
    u8 = [[[[10, 20, 9]], [[1, 2, 9]], [[0, 3, 9]]]]
    want = [[36, 2, 11, 25], [0, 0, 0, 0]]
    assert sr.brute_scores(ids, labels, u8, [-7, -1, 0], 2) == want
    assert sr.scores_image(ids, labels, np.array(u8, np.uint8), [-7, -1, 0], 2).tolist() == want


@pytest.mark.parametrize("shape", [(1, 1), (1, 13), (12, 1), (5, 7), (12, 13)])
def test_reference_equals_the_pixel_loop(shape):
    H, W = shape
    rs = np.random.RandomState(100 * H + W)
    for trial in range(6):
        P, nlabels, cap = rs.randint(1, 5), rs.randint(1, 5), rs.randint(1, 7)
        ids = rs.randint(-1, cap + 3, (H, W)).astype(np.int32)
        labels = rs.randint(0, nlabels + 2, (H, W)).astype(np.uint8)
        labels[rs.rand(H, W) < 0.05] = 255
        u8 = rs.randint(0, 256, (P, 3, H, W)).astype(np.uint8)
        if trial == 0:
            u8[:] = 255
        row = rs.randint(-1, P, nlabels + 1)
        if trial == 1:
            row[1:] = [P + 3, -5, 1 << 30, P][:nlabels]                 # what the kernel clamps: not counted
        got = sr.scores_image(ids, labels, u8, row, cap)
        assert got.dtype == np.int64 and got.tolist() == sr.brute_scores(ids.tolist(), labels.tolist(), u8.tolist(),
                                                                         row.tolist(), cap)
        empty = got[:, 1] == 0
        assert not got[empty].any() and (got[~empty, 2] <= got[~empty, 3]).all()


# ------------------------------------------------------------------------------------------------ the C ABI

def test_struct_mirror_sizeof_and_signatures(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\}\s*dfw_seg_scores_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.replace("*", " ").replace(",", " ").split()
        names += [p for p in parts if p not in ("const", "void", "int32_t", "int64_t", "size_t", "uint8_t")]
    assert names == [f[0] for f in L.SegScoresArgs._fields_]
    assert names == ["ids", "labels", "seg_u8", "planes", "planes_host", "scores", "ws", "ws_bytes", "B", "H", "W", "cap",
                     "nlabels", "P"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\n'
                   'int main(){printf("%zu", sizeof(dfw_seg_scores_args));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(L.SegScoresArgs)
    i32 = C.c_int32
    assert L.SYMBOLS["dfw_seg_scores"] == (i32, [C.POINTER(L.SegScoresArgs), C.c_void_p])
    assert L.SYMBOLS["dfw_seg_scores_workspace_bytes"] == (C.c_size_t, [i32, i32])
    assert L.SYMBOLS["dfw_seg_scores_block"] == (i32, [C.POINTER(i32)])
    assert hip_lib.dfw_version() >= 118
    assert "seg_scores.hip" in __import__("diffews_amd.build", fromlist=["SOURCES"]).SOURCES


def test_block_and_workspace_queries(hip_lib):
    from diffews_amd import ops
    p = C.c_int32()
    assert hip_lib.dfw_seg_scores_block(None) == DFW_EINVAL
    assert hip_lib.dfw_seg_scores_block(C.byref(p)) == 0
    assert p.value >= 64 and p.value % 64 == 0 and ops.seg_scores_block() == p.value
    q = hip_lib.dfw_seg_scores_workspace_bytes
    for B in (1, 2, 3, 64, 65535):
        for cap in (1, 2, 15, 16, 255, 256, 1024):
            got = q(B, cap)
            assert got >= 20 * B * cap > 0, (B, cap)                       # 8 + 3 * 4 bytes of accumulators a row
            assert q(B, cap + 1) >= got and (B == 65535 or q(B + 1, cap) >= got)
            assert ops.seg_scores_workspace(B, cap) == got
    for bad in ((0, 4), (-1, 4), (4, 0), (4, -3), (65536, 1), (1, 1 << 29), (4, 1 << 27), (65535, 6554)):
        assert q(*bad) == 0, bad                                            # B * cap * 5 above 2^31 - 1, B above 65535


def _valid(lib, B=2, H=5, W=7, cap=4, nlabels=3, P=6):
    """A fully valid call on host memory (never launched: every test below breaks one thing)."""
    from diffews_amd import _lib as L
    ws_bytes = lib.dfw_seg_scores_workspace_bytes(B, cap)
    assert ws_bytes > 0
    table = np.full((B, nlabels + 1), -1, np.int32)
    table[:, 1:] = np.arange(B * nlabels).reshape(B, nlabels) % P
    table[:, 0] = 1 << 20                                              # entry 0 is never read, whatever it holds
    keep = dict(ids=np.zeros((B, H, W), np.int32), labels=np.zeros((B, H, W + 1), np.uint8),
                seg_u8=np.zeros((P, 3, H, W + 1), np.uint8), planes=table.copy(), planes_host=table,
                scores=np.zeros((B, cap, 4), np.int64), ws=np.zeros(ws_bytes // 8 + 1, np.int64))
    a = L.SegScoresArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.ws_bytes, a.B, a.H, a.W, a.cap, a.nlabels, a.P = ws_bytes, B, H, W, cap, nlabels, P
    return a, keep


def test_every_refusal_comes_from_the_host_before_any_launch(hip_lib):
    kept = []

    def broken(**kw):
        a, keep = _valid(hip_lib)
        kept.append(keep)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.dfw_seg_scores(C.byref(a), None)

    assert hip_lib.dfw_seg_scores(None, None) == DFW_EINVAL
    for field in ("ids", "labels", "seg_u8", "planes", "planes_host", "scores", "ws"):
        assert broken(**{field: None}) == DFW_EINVAL, field
    for field in ("B", "H", "W", "cap", "P"):
        for v in (0, -1):
            assert broken(**{field: v}) == DFW_EINVAL, field
    for v in (0, -1, 255, 1000):
        assert broken(nlabels=v) == DFW_EINVAL, v
    # DFW_ERANGE: the sizes are judged before the table, the workspace and the pointers' extents
    assert broken(H=65536, W=1) == DFW_ERANGE
    assert broken(H=1, W=65536) == DFW_ERANGE
    assert broken(H=65535, W=32768) == DFW_ERANGE                    # H * W above 2^30
    assert broken(B=65536) == DFW_ERANGE
    assert broken(cap=1 << 28) == DFW_ERANGE                         # B * cap * 5 above 2^31 - 1
    assert broken(B=1, cap=1 << 29) == DFW_ERANGE
    # the host mirror of the table: an entry above P - 1 or below -1, in any row; entry 0 is not looked at
    for b, l, v in ((0, 1, 6), (1, 3, 6), (0, 2, -2), (1, 1, 1 << 30), (1, 2, -(1 << 31))):
        a, keep = _valid(hip_lib)
        keep["planes_host"][b, l] = v
        assert hip_lib.dfw_seg_scores(C.byref(a), None) == DFW_EINVAL, (b, l, v)
    assert broken(P=5) == DFW_EINVAL                                 # the table names group 5
    # DFW_EWORKSPACE: one byte short; anything larger on the same workspace
    a, keep = _valid(hip_lib)
    a.ws_bytes -= 1
    assert hip_lib.dfw_seg_scores(C.byref(a), None) == DFW_EWORKSPACE
    assert broken(ws_bytes=0) == DFW_EWORKSPACE
    assert broken(cap=5) == DFW_EWORKSPACE
    # scores or ws on top of an input, at its start and inside it; an input inside an output
    for out in ("scores", "ws"):
        for inp, last in (("ids", 4 * (2 * 5 * 7 - 1)), ("labels", 2 * 5 * 7 - 1), ("seg_u8", 6 * 3 * 5 * 7 - 1),
                          ("planes", 4 * (2 * 4 - 1))):
            for shift in (0, last):
                a, keep = _valid(hip_lib)
                setattr(a, out, getattr(a, inp) + shift)
                assert hip_lib.dfw_seg_scores(C.byref(a), None) == DFW_EINVAL, (out, inp, shift)
    a, keep = _valid(hip_lib)
    a.labels = a.scores + 8
    assert hip_lib.dfw_seg_scores(C.byref(a), None) == DFW_EINVAL
    a, keep = _valid(hip_lib)
    a.ws = a.scores + 16                                             # the two outputs on each other
    assert hip_lib.dfw_seg_scores(C.byref(a), None) == DFW_EINVAL
    # DFW_ESHAPE: words off their natural alignment; scores holds 64-bit words
    for field, shift in (("ids", 2), ("planes", 2), ("ws", 2), ("ws", 1), ("scores", 4), ("scores", 2)):
        a, keep = _valid(hip_lib)
        if field == "ws":                                            # room for the shift behind the workspace
            keep["ws"] = np.zeros(len(keep["ws"]) + 1, np.int64)
            a.ws = keep["ws"].ctypes.data
        setattr(a, field, getattr(a, field) + shift)
        assert hip_lib.dfw_seg_scores(C.byref(a), None) == DFW_ESHAPE, (field, shift)
    # the order of the house: null before size, EINVAL sizes before ERANGE, sizes before the table, the table before the
    # workspace, the workspace before overlap, overlap before alignment
    assert broken(ids=None, H=65536) == DFW_EINVAL
    assert broken(H=65536, nlabels=0) == DFW_EINVAL
    a, keep = _valid(hip_lib)
    keep["planes_host"][0, 1] = 99
    a.H, a.ws_bytes = 70000, 0
    assert hip_lib.dfw_seg_scores(C.byref(a), None) == DFW_ERANGE
    a, keep = _valid(hip_lib)
    keep["planes_host"][0, 1] = 99
    a.ws_bytes = 0
    assert hip_lib.dfw_seg_scores(C.byref(a), None) == DFW_EINVAL
    a, keep = _valid(hip_lib)
    a.scores, a.ws_bytes = a.ids, 0
    assert hip_lib.dfw_seg_scores(C.byref(a), None) == DFW_EWORKSPACE
    a, keep = _valid(hip_lib)
    a.scores = a.ids + 2
    assert hip_lib.dfw_seg_scores(C.byref(a), None) == DFW_EINVAL
    for keep in kept:                                                # nothing was written by any of these
        assert not keep["scores"].any() and not keep["ws"].any() and not keep["ids"].any()
    # the buffer rule of the object stages: every output and the workspace against every input and each other
    # (planes_host is host memory and no part of it)
    check_overlap_rule(lambda a: hip_lib.dfw_seg_scores(C.byref(a), None), lambda: _valid(hip_lib),
                       dict(ids=(4 * 2 * 5 * 7, 4), labels=(2 * 5 * 7, 1), seg_u8=(6 * 3 * 5 * 7, 1), planes=(2 * 4 * 4, 4)),
                       dict(scores=(2 * 4 * 32, 8), ws=(hip_lib.dfw_seg_scores_workspace_bytes(2, 4), 4)))
    assert hip_lib.dfw_version() >= 122


def test_ops_pass_the_allocation_scan():
    import test_launch_guard_cpu as scan
    seen = scan._allocating_functions(os.path.join(ROOT, "diffews_amd", "ops.py"))
    assert "seg_scores" not in seen and "seg_scores_workspace" not in seen
    scan.test_every_allocation_of_the_wrappers_is_reachable_and_declared()


# ------------------------------------------------------------------------------------------------ the plane helpers

def test_plane_tables_against_hand_written_ones():
    from diffews_amd.objects import planes_for_binary, planes_for_candidates, planes_for_classes
    t = planes_for_classes(3, 2)
    assert t.dtype == torch.int32 and t.tolist() == [[-1, 0, 2, 4], [-1, 1, 3, 5]]
    assert planes_for_classes(1, 1).tolist() == [[-1, 0]]
    assert planes_for_binary(3).tolist() == [[-1, 0], [-1, 1], [-1, 2]]
    # queries in order, each list in ascending set index as the route sorts it; class 3 is listed by query 0 only, class 1
    # by query 2 only, query 1 has no candidate
    cands = [(3, 0), (), [1, 2, 0]]
    assert planes_for_candidates(cands, 4).tolist() == [[-1, 0, -1, -1, 1], [-1, -1, -1, -1, -1], [-1, 2, 3, 4, -1]]
    assert planes_for_candidates(cands, 4, labels="set").tolist() == planes_for_candidates(cands, 4, "global").tolist()
    assert planes_for_candidates(cands, 3, labels="local").tolist() == [[-1, 0, 1, -1], [-1, -1, -1, -1], [-1, 2, 3, 4]]
    assert planes_for_candidates([torch.tensor([2, 0]), torch.tensor([1])], 3).tolist() == [[-1, 0, -1, 1], [-1, -1, 2, -1]]
    for bad in (lambda: planes_for_candidates(cands, 3), lambda: planes_for_candidates(cands, 2, "local"),
                lambda: planes_for_candidates([(1, 1)], 4), lambda: planes_for_candidates(cands, 4, "query"),
                lambda: planes_for_candidates([(-1,)], 4), lambda: planes_for_classes(0, 2), lambda: planes_for_binary(0)):
        with pytest.raises(ValueError):
            bad()


def test_wrappers_refuse_wrong_arguments_without_a_device(hip_lib):
    from diffews_amd import objects
    with pytest.raises(ValueError):
        objects.ScoreBuffers(1, 0, 3, device="cpu")
    with pytest.raises(ValueError):
        objects.ScoreBuffers(1, 4, 255, device="cpu")
    with pytest.raises(ValueError):
        objects.ScoreBuffers(65536, 4, 3, device="cpu")                    # seg_scores refuses the size
    o = dict(ids=torch.zeros(5, 7, dtype=torch.int32), labels=torch.zeros(5, 7, dtype=torch.uint8),
             stats=torch.zeros(4, 8, dtype=torch.int32))
    with pytest.raises(ValueError):
        objects.object_scores(o, torch.zeros(1, 3, 5, 7, dtype=torch.uint8), [[-1, 0]])   # host ids
    with pytest.raises(ValueError):
        objects.object_scores(o, torch.zeros(1, 3, 5, 7, dtype=torch.uint8), [[-1.0, 0.5]])


# ------------------------------------------------------------------------------------------------ average precision

COCO = tuple((n, 20) for n in range(10, 20))


def _same_ap(got, want):
    assert got["ap"].shape == (len(want), len(got["thresholds"]))
    for c, per in enumerate(want):
        if per is None:
            assert np.isnan(got["ap"][c]).all(), c
        else:
            assert got["ap"][c].tolist() == per, (c, got["ap"][c].tolist(), per)
    m = sr.loop_map(want)
    assert (math.isnan(m) and math.isnan(got["map"])) or got["map"] == m


def test_average_precision_equals_the_loop_reference():
    from diffews_amd.metrics import average_precision
    rs = np.random.RandomState(2024)
    for trial in range(50):
        nlabels, images = rs.randint(1, 6), rs.randint(1, 5)
        per_image = []
        for _ in range(images):
            k = rs.randint(0, 40)
            n = rs.randint(1, 50 if trial % 2 else 4, k)                   # small n: many ties in sum / n
            total = rs.randint(0, 766, k) * n if trial % 3 == 0 else np.array([rs.randint(0, 765 * v + 1) for v in n], np.int64)
            union = rs.randint(1, 200, k)
            inter = np.minimum(union, (union * rs.choice([0.3, 0.5, 0.55, 0.6, 0.75, 0.9, 0.95, 1.0], k)).astype(np.int64) + rs.randint(0, 2, k))
            partner = rs.rand(k) < 0.7
            rows = np.stack([rs.randint(0, nlabels + 2, k), total, n, np.where(partner, inter, 0), np.where(partner, union, 0)], 1)
            per_image.append(rows.astype(np.int64).reshape(-1, 5))
        npos = rs.randint(0, 30, nlabels + 1)
        npos[0] = 0
        thr = COCO if trial % 2 else ((1, 2), (2, 3), (19, 20), (1, 1))
        flat = [r for rows in per_image for r in rows.tolist()]
        want = sr.loop_ap(flat, npos.tolist(), thr)
        got = average_precision(per_image, npos, thr)
        _same_ap(got, want)
        assert got["thresholds"] == tuple(thr)
        _same_ap(average_precision([per_image[:1], per_image[1:]], npos, thr), want)   # nested lists: the same order
        if thr is COCO:
            assert np.array_equal(got["ap50"], got["ap"][:, 0], equal_nan=True)
        else:
            assert got["ap50"] is None


def test_average_precision_known_answers():
    from diffews_amd.metrics import average_precision
    D = lambda *rows: np.array(rows, np.int64).reshape(-1, 5)  # noqa: E731
    # all TP in score order -> 1.0
    r = average_precision([D((1, 700, 1, 10, 10), (1, 600, 1, 8, 8)), D((1, 500, 1, 20, 20))], [0, 3])
    assert r["ap"][1].tolist() == [1.0] * 10 and r["ap50"][1] == 1.0 and r["map"] == 1.0
    # no detection -> 0.0; a class with npos = 0 -> NaN and excluded from map
    r = average_precision([], [0, 4, 0])
    assert r["ap"][1].tolist() == [0.0] * 10 and np.isnan(r["ap"][0]).all() and np.isnan(r["ap"][2]).all() and r["map"] == 0.0
    r = average_precision(D((2, 10, 1, 9, 10)), [0, 1, 0])
    assert r["ap"][1].tolist() == [0.0] * 10 and np.isnan(r["ap"][2]).all() and r["map"] == 0.0
    assert math.isnan(average_precision(D((1, 10, 1, 9, 10)), [0, 0])["map"])
    # one FP ranked above one TP, npos = 1: precision 1/2 at every recall up to 1 -> 0.5
    r = average_precision(D((1, 500, 1, 0, 0), (1, 400, 1, 10, 10)), [0, 1], ((1, 2),))
    assert r["ap"][1].tolist() == [0.5] and r["map"] == 0.5 and r["ap50"] is None    # ap50 is the column of (10, 20)
    # the rule is strict: IoU exactly at the threshold is no TP (COCO would count it)
    r = average_precision(D((1, 500, 1, 5, 10)), [0, 1], ((1, 2), (2, 3)))
    assert r["ap"][1].tolist() == [0.0, 0.0]
    r = average_precision(D((1, 500, 1, 7, 10)), [0, 1], ((1, 2), (7, 10), (2, 3)))
    assert r["ap"][1].tolist() == [1.0, 0.0, 1.0] and r["ap50"] is None
    # a tie in score (2/1 == 4/2) is resolved by image order: the first image's detection is ranked first
    tp, fp = (1, 4, 2, 9, 10), (1, 2, 1, 0, 0)
    assert average_precision([D(tp), D(fp)], [0, 1], ((1, 2),))["ap"][1].tolist() == [1.0]
    assert average_precision([D(fp), D(tp)], [0, 1], ((1, 2),))["ap"][1].tolist() == [0.5]
    # a threshold below 1/2 is refused: the match table cannot decide it
    for bad in (((9, 20),), ((1, 2), (1, 3)), ((0, 1),), ((3, 2),)):
        with pytest.raises(ValueError):
            average_precision(D(tp), [0, 1], bad)


# ------------------------------------------------------------------------------------------------ COCO result records

def test_coco_results_on_a_hand_made_map():
    """4 x 5, two objects.  The three host tables are written by hand in the forms objects_to_host, runs_to_host and
    scores_to_host return for one image."""
    from diffews_amd.objects import coco_results, runs_to_mask
    ids = np.array([[1, 1, 0, 0, 0],
                    [1, 0, 0, 2, 2],
                    [0, 0, 0, 2, 2],
                    [0, 0, 0, 0, 2]])
    h, w = ids.shape
    o_host = [(2, 3, (0, 0, 2, 2), 0), (1, 5, (1, 3, 4, 5), 8)]          # (label, area, half-open box, first pixel)
    runs_host = [np.array([[0, 2], [4, 1]], np.int32), np.array([[13, 2], [17, 3]], np.int32)]   # column order: x * 4 + y
    for k in (1, 2):
        assert np.array_equal(runs_to_mask(runs_host[k - 1], h, w, "column"), ids == k)
    scores_host = dict(sum=np.array([1530, 7, 0], np.int64), n=np.array([3, 5, 0], np.int64),
                       min=np.array([300, 0, 0], np.int64), max=np.array([765, 3, 0], np.int64))
    got = coco_results(o_host, runs_host, scores_host, image_id=42, category_ids=[18, 44], h=h, w=w)
    assert [g["image_id"] for g in got] == [42, 42] and [g["category_id"] for g in got] == [44, 18]
    assert [g["bbox"] for g in got] == [[0, 0, 2, 2], [3, 1, 2, 3]] and [g["area"] for g in got] == [3, 5]
    assert got[0]["segmentation"] == {"size": [4, 5], "counts": [0, 2, 2, 1, 15]}
    assert got[1]["segmentation"] == {"size": [4, 5], "counts": [13, 2, 2, 3]}
    for g in got:
        assert sum(g["segmentation"]["counts"]) == h * w
    assert got[0]["score"] == 1530 / (765 * 3) and got[1]["score"] == 7 / (765 * 5)
    assert set(got[0]) == {"image_id", "category_id", "segmentation", "bbox", "area", "score"}
    # an object without a counted pixel scores 0; one without runs (a truncated table) gets the empty encoding
    got = coco_results(o_host + [(1, 1, (3, 0, 4, 1), 15)], runs_host, scores_host, 7, [18, 44], h, w)
    assert got[2]["score"] == 0.0 and got[2]["segmentation"]["counts"] == [20] and got[2]["bbox"] == [0, 3, 1, 1]
