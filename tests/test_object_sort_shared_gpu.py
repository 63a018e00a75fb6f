"""GPU test of the run compaction and radix sort the run-length and the matching stage share (csrc/seg_sort.h): on one id
map both stages must find the same records.  H * W = 3 * pixels + 5 positions with an odd W and ids 1 + (7 q mod 300): every
position starts a run, so there are 3 * records + 5 of them -- more than three sort chunks, the last one partial -- and
both stages sort on two key bytes (cap 300 on the run-length side; key = 2 p on the matching side, whose ground truth is
empty).  Each output is also compared with its numpy reference, so two equal wrong answers do not pass.  All integers:
every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import match_ref as mr
import rle_ref as rr

pytestmark = pytest.mark.gpu

CAP = 300


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def block(hip_lib):
    p, r, p2, r2 = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    assert hip_lib.dfw_seg_rle_block(C.byref(p), C.byref(r)) == 0 and hip_lib.dfw_seg_match_block(C.byref(p2), C.byref(r2)) == 0
    assert (p.value, r.value) == (p2.value, r2.value)
    return p.value, r.value


@pytest.fixture(scope="module")
def ids(block):
    P, R = block
    HW = 3 * P + 5
    assert P == R and HW % 2 == 1
    W = next(w for w in range(3, HW + 1, 2) if HW % w == 0)              # odd, and HW itself at the latest
    return (1 + 7 * np.arange(HW) % CAP).astype(np.int32).reshape(1, HW // W, W)


@pytest.mark.parametrize("truncated", [False, True], ids=["all-kept", "cut-in-the-second-chunk"])
def test_both_stages_find_the_same_records(ops, block, ids, truncated):
    P, R = block
    _, H, W = ids.shape
    M = R + 3 if truncated else H * W
    i32 = dict(dtype=torch.int32, device="cuda")
    dev = torch.from_numpy(ids).cuda()
    runs, run_off, nruns = torch.empty(1, M, 2, **i32), torch.empty(1, CAP + 1, **i32), torch.empty(1, 2, **i32)
    ops.seg_rle(dev, runs, run_off, nruns, torch.empty(ops.seg_rle_workspace(1, H, W, CAP, M, "row"), dtype=torch.uint8, device="cuda"),
                CAP, "row")
    MP = CAP + 1
    pairs, pair_off, area = torch.empty(1, MP, 3, **i32), torch.empty(1, CAP + 2, **i32), torch.empty(1, CAP + 3, **i32)
    match, gmatch, n = torch.empty(1, CAP, 3, **i32), torch.empty(1, 1, **i32), torch.empty(1, 4, **i32)
    pq = torch.empty(1, 2, 4, dtype=torch.int64, device="cuda")
    nbytes = ops.seg_match_workspace(1, H, W, CAP, 1, M, MP)
    assert nbytes > 0
    ops.seg_match(dev, torch.zeros_like(dev), pairs, pair_off, area, match, gmatch, pq, n,
                  torch.empty(nbytes, dtype=torch.uint8, device="cuda"), M)
    torch.cuda.synchronize()
    runs, run_off, nruns, pairs, area, n = (t.cpu().numpy()[0] for t in (runs, run_off, nruns, pairs, area, n))

    # the two stages against each other
    kept = min(H * W, M)
    assert nruns.tolist() == [kept, H * W] and np.array_equal(n[2:4], nruns)
    area_p, area_g = area[:CAP + 1], area[CAP + 1:]
    per_object = np.array([0] + [rr.object_rows(runs, run_off, k)[:, 1].sum() for k in range(1, CAP + 1)])
    assert per_object.sum() == kept and np.array_equal(area_p, per_object)
    present = np.flatnonzero(area_p)
    assert n[0] == n[1] == len(present)
    assert np.array_equal(pairs[:len(present)], np.stack([present, 0 * present, area_p[present]], 1))
    assert area_g[0] == kept and not area_g[1:].any()                    # cell 0 is the background column; no object has area

    # each stage against its reference
    want = rr.rle(ids, CAP, M, "row")
    assert np.array_equal(nruns, want["nruns"][0]) and np.array_equal(run_off, want["run_off"][0])
    assert np.array_equal(runs[:kept], want["runs"][0])
    want = mr.match(ids, np.zeros_like(ids), CAP, 1, 1, M, MP)
    got = dict(n=n, pair_off=pair_off.cpu().numpy()[0], area=area, match=match.cpu().numpy()[0], gmatch=gmatch.cpu().numpy()[0],
               pq=pq.cpu().numpy()[0])
    for k, v in got.items():
        assert np.array_equal(v, want[k][0]), k
    assert np.array_equal(pairs[:n[0]], want["pairs"][0])
