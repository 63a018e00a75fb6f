"""CPU tests of the matching stage: the numpy reference tests/match_ref.py on the header's worked example, against a
per-pixel dictionary loop and against a brute-force IoU matrix (with the uniqueness of the partner asserted);
metrics.panoptic_quality against hand-computed values; and the C ABI of dfw_seg_match -- header, ctypes mirror, sizeof, the
workspace query and every host-side refusal (host pointers, null stream: nothing is launched).  Every comparison of
integers is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as cr
import match_ref as mr
from seg_args_cases import check_overlap_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ESHAPE, DFW_ERANGE, DFW_EWORKSPACE = -1, -2, -3, -4


# ------------------------------------------------------------------------------------------------ the reference

def test_worked_example_of_the_header():
    pids = np.array([[1, 1, 0], [2, 1, 1]], np.int32)
    gids = np.array([[1, 1, 1], [0, 2, 2]], np.int32)
    k = mr.keys(pids, gids, 2, 2)
    rk, rl, n = mr.records(k, 100)
    assert [(int(a) // 3, int(a) % 3, int(b)) for a, b in zip(rk, rl)] == [(1, 1, 2), (0, 1, 1), (2, 0, 1), (1, 2, 2)] and n == (4, 4)
    r = mr.match_image(pids, gids, 2, 2, 1, 100, 100)
    assert r["pairs"].tolist() == [[0, 1, 1], [1, 1, 2], [1, 2, 2], [2, 0, 1]]
    assert r["pair_off"].tolist() == [0, 1, 3, 4] and r["area"].tolist() == [1, 4, 1, 1, 3, 2]
    assert r["n"].tolist() == [4, 4, 4, 4]
    assert not r["match"].any() and not r["gmatch"].any()              # 2/5, and 2/4 is not ABOVE one half
    assert r["pq"].tolist() == [[0, 0, 0, 0], [0, 2, 2, 0]]
    gids2 = np.array([[1, 1, 0], [0, 1, 1]], np.int32)                 # g = 1 is p = 1 exactly
    r = mr.match_image(pids, gids2, 2, 2, 1, 100, 100)
    assert r["match"].tolist() == [[1, 4, 4], [0, 0, 0]] and r["gmatch"].tolist() == [1, 0]
    assert r["pq"][1].tolist() == [1, 1, 0, 1 << 32]
    # one more shared pixel lifts (1, 2) from 2/4 to 3/5; at a threshold of 3/5 that is, again, not above
    gids3 = np.array([[1, 2, 2], [0, 2, 2]], np.int32)
    assert mr.match_image(pids, gids3, 2, 2, 1, 100, 100)["match"][0].tolist() == [2, 3, 5]
    assert not mr.match_image(pids, gids3, 2, 2, 1, 100, 100, iou=(3, 5))["match"].any()
    # truncation: the first records, then the first pairs; every table describes what was kept
    r = mr.match_image(pids, gids, 2, 2, 1, 2, 100)                    # records (1,1)x2 and (0,1)x1
    assert r["n"].tolist() == [2, 2, 2, 4] and r["pairs"].tolist() == [[0, 1, 1], [1, 1, 2]]
    assert r["area"].tolist() == [1, 2, 0, 0, 3, 0] and r["pair_off"].tolist() == [0, 1, 2, 2]
    assert r["match"][0].tolist() == [1, 2, 3] and r["pq"][1].tolist() == [1, 0, 0, (2 << 32) // 3]
    r = mr.match_image(pids, gids, 2, 2, 1, 100, 3)
    assert r["n"].tolist() == [3, 4, 4, 4] and r["pairs"].tolist() == [[0, 1, 1], [1, 1, 2], [1, 2, 2]]
    assert r["area"].tolist() == [1, 4, 0, 0, 3, 2] and r["pair_off"].tolist() == [0, 1, 3, 3]
    # ids above cap and negative ids are background; a skipped pixel is (0, 0)
    r = mr.match_image(np.array([[3, -1, 1]], np.int32), np.array([[1, 1, 9]], np.int32), 2, 2, 1, 100, 100)
    assert r["pairs"].tolist() == [[0, 1, 2], [1, 0, 1]]
    r = mr.match_image(pids, gids, 2, 2, 1, 100, 100, skip=np.array([[0, 255, 0], [255, 0, 7]], np.uint8))
    assert r["pairs"].tolist() == [[0, 1, 1], [1, 1, 1], [1, 2, 2]] and r["area"].tolist() == [1, 3, 0, 0, 2, 2]
    assert r["match"][0].tolist() == [2, 2, 3] and r["pq"][1].tolist()[:3] == [1, 0, 1]   # object p = 2 is absent: no FP


def _maps(H, W, rs, nlabels=3):
    lab = mr.blobs(H, W, rs, nlabels)
    gt = mr.perturb(lab, rs)
    p = cr.components(lab[None], 8, 0, 256)
    g = cr.components(gt[None], 4, 0, 256)
    return p["ids"][0], p["stats"][0], g["ids"][0], g["stats"][0], gt


@pytest.mark.parametrize("shape", [(5, 7), (9, 11), (1, 37), (16, 13)])
def test_reference_equals_the_pixel_loop_and_the_iou_matrix(shape):
    H, W = shape
    rs = np.random.RandomState(100 * H + W)
    for rep in range(4):
        pids, pstats, gids, gstats, gt = _maps(H, W, rs)
        cap_p, cap_g = max(1, int(pids.max())) + 1, max(1, int(gids.max()))
        for skip in (None, gt):
            for iou in ((1, 2), (3, 4), (2, 3)):
                for with_stats in (True, False):
                    ps, gs = (pstats[:cap_p], gstats[:cap_g]) if with_stats else (None, None)
                    r = mr.match_image(pids, gids, cap_p, cap_g, 3, H * W, H * W, ps, gs, skip, iou)
                    want = mr.pixel_pairs(pids.tolist(), gids.tolist(), cap_p, cap_g, None if skip is None else skip.tolist())
                    assert {(p, g): i for p, g, i in r["pairs"].tolist()} == want
                    assert r["pairs"].tolist() == sorted(r["pairs"].tolist())
                    assert r["n"][0] == r["n"][1] == len(want) and r["n"][2] == r["n"][3]
                    for p in range(cap_p + 1):
                        rows = r["pairs"][r["pair_off"][p]:r["pair_off"][p + 1]]
                        assert (rows[:, 0] == p).all() and rows[:, 2].sum() == r["area"][p]
                        assert r["area"][p] == sum(v for (a, _), v in want.items() if a == p)
                    for g in range(cap_g + 1):
                        assert r["area"][cap_p + 1 + g] == sum(v for (_, b), v in want.items() if b == g)
                    pcls, gcls = mr.classes_of(ps, cap_p), mr.classes_of(gs, cap_g)
                    matches, counts = mr.brute_matches(pids, gids, cap_p, cap_g, pcls, gcls, 3, skip, iou)
                    got = [(p + 1, *row) for p, row in enumerate(r["match"].tolist()) if row[0]]
                    assert got == [(p, g, i, u) for p, g, i, u in matches], (shape, rep, iou)
                    assert [(int(p), g + 1) for g, p in enumerate(r["gmatch"]) if p] == sorted((p, g) for p, g, _, _ in matches)
                    assert r["pq"][:, :3].tolist() == counts and not r["pq"][0].any()
                    for c in range(1, 4):
                        assert r["pq"][c, 3] == sum((i << 32) // u for p, g, i, u in matches if pcls[p - 1] == c)


def test_panoptic_quality_against_hand_computed_values():
    import torch
    from diffews_amd.metrics import panoptic_quality
    one = 1 << 32
    # class 1: two TPs of IoU 3/4 and 1/1, one FP, one FN; class 2: no object at all; class 3: three FPs
    pq = torch.tensor([[0, 0, 0, 0], [2, 1, 1, (3 * one) // 4 + one], [0, 0, 0, 0], [0, 3, 0, 0]], dtype=torch.int64)
    r = panoptic_quality(pq)
    assert r["sq"].dtype == torch.float64 and r["pq"].shape == (4,)
    assert r["sq"].tolist() == [0.0, 0.875, 0.0, 0.0]
    assert r["rq"].tolist() == [0.0, 2 / 3, 0.0, 0.0]
    assert r["pq"].tolist() == [0.0, 0.875 * (2 / 3), 0.0, 0.0]
    assert r["mean_sq"] == 0.4375 and r["mean_rq"] == 1 / 3 and r["mean_pq"] == 0.875 * (2 / 3) / 2    # classes 1 and 3
    # a batch is summed first; a list of per-image tables of different batch shapes likewise
    two = torch.stack([pq, pq])
    assert panoptic_quality(two)["pq"].tolist() == r["pq"].tolist()
    assert panoptic_quality([pq, two])["sq"].tolist() == r["sq"].tolist()
    empty = panoptic_quality(torch.zeros(1, 3, 4, dtype=torch.int64))
    assert empty["mean_pq"] == 0.0 and not empty["pq"].any()
    only_fn = panoptic_quality(torch.tensor([[0, 0, 0, 0], [0, 0, 2, 0]]))
    assert only_fn["rq"].tolist() == [0.0, 0.0] and only_fn["mean_rq"] == 0.0
    with pytest.raises(ValueError):
        panoptic_quality(torch.zeros(3, 5, dtype=torch.int64))
    with pytest.raises(ValueError):
        panoptic_quality(torch.zeros(1, 4, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ the C ABI

FIELDS = ["pids", "gids", "pstats", "gstats", "skip", "pairs", "pair_off", "area", "match", "gmatch", "pq", "n", "ws", "ws_bytes",
          "B", "H", "W", "capP", "capG", "nlabels", "max_records", "max_pairs", "num", "den"]


def test_struct_mirror_and_sizeof(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\}\s*dfw_seg_match_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.replace("*", " ").replace(",", " ").split()
        names += [p for p in parts if p not in ("const", "void", "int32_t", "int64_t", "size_t", "uint8_t")]
    assert names == [f[0] for f in L.SegMatchArgs._fields_] == FIELDS
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\n'
                   'int main(){printf("%zu", sizeof(dfw_seg_match_args));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(L.SegMatchArgs)
    i32 = C.c_int32
    assert L.SYMBOLS["dfw_seg_match"] == (i32, [C.POINTER(L.SegMatchArgs), C.c_void_p])
    assert L.SYMBOLS["dfw_seg_match_workspace_bytes"] == (C.c_size_t, [i32] * 7)
    assert L.SYMBOLS["dfw_seg_match_block"] == (i32, [C.POINTER(i32), C.POINTER(i32)])
    assert hip_lib.dfw_version() >= 116
    assert "seg_match.hip" in __import__("diffews_amd.build", fromlist=["SOURCES"]).SOURCES


def _block(lib):
    p, r = C.c_int32(), C.c_int32()
    assert lib.dfw_seg_match_block(C.byref(p), C.byref(r)) == 0
    return p.value, r.value


def test_workspace_query_is_monotone(hip_lib):
    q = hip_lib.dfw_seg_match_workspace_bytes
    P, R = _block(hip_lib)
    assert P >= 1 and R >= 1 and hip_lib.dfw_seg_match_block(None, None) == DFW_EINVAL
    p, r = C.c_int32(), C.c_int32()
    assert hip_lib.dfw_seg_match_block(C.byref(p), None) == DFW_EINVAL and hip_lib.dfw_seg_match_block(None, C.byref(r)) == DFW_EINVAL
    for B in (1, 3):
        for H, W in ((1, 1), (2, 37), (64, 65), (65, 64)):
            for cp, cg in ((1, 1), (15, 15), (255, 256), (4095, 4095), (32767, 65535)):
                for M in (1, R - 1, R, R + 1, 3 * R + 5):
                    for MP in (1, 255, 256, 1000):
                        got = q(B, H, W, cp, cg, M, MP)
                        # the records before and after the sort, the block sums, both pair arrays
                        assert got >= 4 * B * (5 * M + -(-(H * W) // P) + 2 * MP) > 0, (B, H, W, cp, cg, M, MP)
                        for d in range(7):
                            more = [B, H, W, cp, cg, M, MP]
                            more[d] += 1
                            top = cp == 32767 and d in (3, 4)          # one more object and the key leaves the int
                            assert (q(*more) == 0) if top else (q(*more) >= got), (d, more)
    assert q(2, 32768, 32768, 1024, 1024, 1 << 20, 1 << 18) >= (2 * 5 << 20) * 4          # no 32-bit arithmetic on the way
    for bad in ((0, 5, 5, 4, 4, 4, 4), (1, 0, 5, 4, 4, 4, 4), (1, 5, -1, 4, 4, 4, 4), (1, 5, 5, 0, 4, 4, 4), (1, 5, 5, 4, 0, 4, 4),
                (1, 5, 5, 4, 4, 0, 4), (1, 5, 5, 4, 4, 4, 0), (1, 65536, 1, 4, 4, 4, 4), (1, 5, 5, 65535, 65535, 4, 4),
                (65536, 5, 5, 4, 4, 4, 4), (1, 5, 5, 4, 4, 1 << 30, 1 << 30)):
        assert q(*bad) == 0, bad


def _valid(lib, B=2, H=5, W=7, capP=4, capG=3, nlabels=2, max_records=6, max_pairs=5, stats=True, skip=True):
    """A fully valid call on host memory (never launched: every test below breaks one thing)."""
    from diffews_amd import _lib as L
    ws_bytes = lib.dfw_seg_match_workspace_bytes(B, H, W, capP, capG, max_records, max_pairs)
    assert ws_bytes > 0
    keep = dict(pids=np.zeros((B, H, W), np.int32), gids=np.zeros((B, H, W), np.int32),
                pstats=np.zeros((B, capP, 8), np.int32), gstats=np.zeros((B, capG, 8), np.int32),
                skip=np.zeros((B, H, W + 1), np.uint8), pairs=np.zeros((B, max_pairs, 3), np.int32),
                pair_off=np.zeros((B, capP + 2), np.int32), area=np.zeros((B, capP + capG + 2), np.int32),
                match=np.zeros((B, capP, 3), np.int32), gmatch=np.zeros((B, capG), np.int32),
                pq=np.zeros((B, nlabels + 1, 4), np.int64), n=np.zeros((B, 4), np.int32), ws=np.zeros(ws_bytes // 8 + 1, np.int64))
    a = L.SegMatchArgs()
    for k, v in keep.items():
        if (k in ("pstats", "gstats") and not stats) or (k == "skip" and not skip):
            continue
        setattr(a, k, v.ctypes.data)
    a.ws_bytes, a.B, a.H, a.W, a.capP, a.capG, a.nlabels = ws_bytes, B, H, W, capP, capG, nlabels
    a.max_records, a.max_pairs, a.num, a.den = max_records, max_pairs, 1, 2
    return a, keep


OUTPUTS = ("pairs", "pair_off", "area", "match", "gmatch", "pq", "n")
INPUTS = ("pids", "gids", "pstats", "gstats", "skip")


def test_every_refusal_comes_from_the_host_before_any_launch(hip_lib):
    kept = []

    def broken(valid=None, **kw):
        a, keep = _valid(hip_lib, **(valid or {}))
        kept.append(keep)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.dfw_seg_match(C.byref(a), None)

    assert hip_lib.dfw_seg_match(None, None) == DFW_EINVAL
    for field in ("pids", "gids", "ws") + OUTPUTS:
        assert broken(**{field: None}) == DFW_EINVAL, field
    for field in ("B", "H", "W", "capP", "capG", "max_records", "max_pairs"):
        for v in (0, -1):
            assert broken(**{field: v}) == DFW_EINVAL, field
    # the threshold: 1 <= num <= den <= 65535 and 2 * num >= den
    for num, den in ((0, 1), (1, 0), (-1, -2), (1, 3), (49, 100), (2, 1), (32768, 65536), (40000, 70000), (0, 0)):
        assert broken(num=num, den=den) == DFW_EINVAL, (num, den)
    for nlabels in (0, -1, 255, 1000):
        assert broken(nlabels=nlabels) == DFW_EINVAL, nlabels
        assert broken(valid=dict(stats=False), nlabels=nlabels) == DFW_EINVAL, nlabels
    # an output on top of an input, at its start and inside it; an input inside an output
    sizes = dict(pids=4 * 2 * 5 * 7, gids=4 * 2 * 5 * 7, pstats=4 * 2 * 4 * 8, gstats=4 * 2 * 3 * 8, skip=2 * 5 * 7)
    for out in OUTPUTS:
        for inp in INPUTS:
            for shift in (0, 8, sizes[inp] - 1):
                a, keep = _valid(hip_lib)
                setattr(a, out, getattr(a, inp) + shift)
                assert hip_lib.dfw_seg_match(C.byref(a), None) == DFW_EINVAL, (out, inp, shift)
    a, keep = _valid(hip_lib)
    a.gids = a.pairs + 8
    assert hip_lib.dfw_seg_match(C.byref(a), None) == DFW_EINVAL
    # DFW_ERANGE: the sizes are checked before the workspace, which could not be that large here
    assert broken(H=65536, W=1) == DFW_ERANGE
    assert broken(H=1, W=65536) == DFW_ERANGE
    assert broken(H=65535, W=32768) == DFW_ERANGE                    # H * W above 2^30
    assert broken(B=65536) == DFW_ERANGE
    assert broken(capP=32768, capG=65535) == DFW_ERANGE              # the highest key would be 2^31 + 65535
    assert broken(capP=65535, capG=65535) == DFW_ERANGE
    assert broken(capP=0x7fffffff, capG=1) == DFW_ERANGE
    assert broken(max_pairs=1 << 29) == DFW_ERANGE                   # B * max_pairs * 3 words
    assert broken(max_records=1 << 30) == DFW_ERANGE                 # B * max_records = 2^31
    assert broken(B=3, capP=1 << 28, capG=1) == DFW_ERANGE           # B * capP * 3 words of match
    # the highest key that is an int passes the sizes: the workspace here is merely too small for nothing else changed
    assert broken(capP=32767, capG=65535, ws_bytes=0) == DFW_EWORKSPACE
    # DFW_EWORKSPACE: one byte short; anything larger on the same workspace
    a, keep = _valid(hip_lib)
    a.ws_bytes -= 1
    assert hip_lib.dfw_seg_match(C.byref(a), None) == DFW_EWORKSPACE
    assert broken(ws_bytes=0) == DFW_EWORKSPACE
    assert broken(H=500) == DFW_EWORKSPACE
    assert broken(B=3) == DFW_EWORKSPACE
    assert broken(max_records=7) == DFW_EWORKSPACE
    assert broken(max_pairs=6) == DFW_EWORKSPACE
    # DFW_ESHAPE: words off their natural alignment, pq off 8 bytes
    for field in ("pids", "gids", "pstats", "gstats", "ws") + OUTPUTS:
        a, keep = _valid(hip_lib)
        setattr(a, field, getattr(a, field) + 2)
        assert hip_lib.dfw_seg_match(C.byref(a), None) == DFW_ESHAPE, field
    a, keep = _valid(hip_lib)
    a.pq += 4
    assert hip_lib.dfw_seg_match(C.byref(a), None) == DFW_ESHAPE
    # the order of the house: a null pointer wins over a size that is out of range, that over the workspace, that over overlap
    assert broken(pids=None, H=65536) == DFW_EINVAL
    a, keep = _valid(hip_lib)
    a.H, a.ws_bytes = 70000, 0
    assert hip_lib.dfw_seg_match(C.byref(a), None) == DFW_ERANGE
    a, keep = _valid(hip_lib)
    a.n, a.ws_bytes = a.pids, 0
    assert hip_lib.dfw_seg_match(C.byref(a), None) == DFW_EWORKSPACE
    assert all(not v.any() for keep in kept for v in keep.values())  # nothing was written by any of these
    # the buffer rule of the object stages: every output and the workspace against every input and each other
    check_overlap_rule(lambda a: hip_lib.dfw_seg_match(C.byref(a), None), lambda: _valid(hip_lib),
                       {k: (v, 1 if k == "skip" else 4) for k, v in sizes.items()},
                       dict(pairs=(2 * 5 * 12, 4), pair_off=(2 * 6 * 4, 4), area=(2 * 9 * 4, 4), match=(2 * 4 * 12, 4),
                            gmatch=(2 * 3 * 4, 4), pq=(2 * 3 * 32, 8), n=(2 * 16, 4),
                            ws=(hip_lib.dfw_seg_match_workspace_bytes(2, 5, 7, 4, 3, 6, 5), 4)))
    assert hip_lib.dfw_version() >= 122


def test_ops_pass_the_allocation_scan():
    """ops.seg_match / seg_match_workspace allocate nothing: test_launch_guard_cpu's scan of ops.py neither sees them nor
    fails."""
    import test_launch_guard_cpu as scan
    seen = scan._allocating_functions(os.path.join(ROOT, "diffews_amd", "ops.py"))
    assert "seg_match" not in seen and "seg_match_workspace" not in seen
    scan.test_every_allocation_of_the_wrappers_is_reachable_and_declared()


def test_wrappers_refuse_wrong_arguments_without_a_device(hip_lib):
    import torch
    from diffews_amd import objects, ops
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise
    assert ops.seg_match_workspace(1, 5, 7, 4, 4, 0, 4) == 0
    ids = torch.zeros(5, 7, dtype=torch.int32)
    with pytest.raises(ValueError):
        objects.match_objects((ids, None, 4), (ids, None, 4), nlabels=1)         # host tensors
    with pytest.raises(ValueError):
        objects.match_objects((ids, None), (ids, None, 4), nlabels=1)            # ids without stats need a cap
    with pytest.raises(ValueError):
        objects.match_objects(ids, (ids, None, 4), nlabels=1)                    # not a result, not a tuple
    with pytest.raises(ValueError):
        objects.match_objects(([ids], None, 4), (ids, None, 4), nlabels=1)       # a list against one map
    with pytest.raises(ValueError):
        objects.match_objects(([ids, ids], None, 4), ([ids], None, 4), nlabels=1)
    with pytest.raises(ValueError):
        objects.MatchBuffers(1, 5, 7, 0, 4, 1, device="cpu")
    with pytest.raises(ValueError):
        objects.MatchBuffers(1, 5, 7, 4, 4, 0, device="cpu")
    with pytest.raises(ValueError):
        objects.MatchBuffers(1, 5, 7, 65535, 65535, 1, device="cpu")             # the key would not fit
    b = objects.MatchBuffers(2, 5, 7, 4, 3, 2, device="cpu")                      # defaults: choices, not measurements
    assert b.max_records == 35 and b.max_pairs == 35 and b.pairs.shape == (2, 35, 3) and b.pq.shape == (2, 3, 4)
    assert b.pair_off.shape == (2, 6) and b.area.shape == (2, 9) and b.match.shape == (2, 4, 3) and b.gmatch.shape == (2, 3)
    assert b.ws.numel() == ops.seg_match_workspace(2, 5, 7, 4, 3, 35, 35)
    big = ops.seg_match_workspace(1, 4096, 4096, 1024, 1024, 1 << 20, 1 << 18)
    assert 0 < big < 40 << 20
    two = torch.zeros(2, 5, 7, dtype=torch.int32)
    for field, wrong in (("pids", two.float()), ("pids", ids), ("gids", two[:, :4]), ("gids", two.long()),
                         ("pairs", b.pairs[:, :, :2].contiguous()), ("pair_off", b.pair_off[:, :5].contiguous()),
                         ("area", b.area.long()), ("pq", b.pq.int()), ("match", b.match[0]), ("gmatch", b.gmatch[:1]),
                         ("n", b.n[:, :2].contiguous()), ("ws", b.ws.int()), ("skip", two), ("pstats", b.match),
                         ("gstats", torch.zeros(2, 4, 8, dtype=torch.int32)), (None, None)):
        kw = dict(pids=two, gids=two, pairs=b.pairs, pair_off=b.pair_off, area=b.area, match=b.match, gmatch=b.gmatch, pq=b.pq,
                  n=b.n, ws=b.ws, max_records=35)
        if field:
            kw[field] = wrong
        # every wrong argument is named; the valid call is refused only for lying on the host
        with pytest.raises(ValueError, match="match must be" if field == "match" else field or "device tensors"):
            ops.seg_match(**kw)
    assert callable(MarigoldPipelineRGBLatentNoise.match_objects)
