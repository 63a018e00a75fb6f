"""The buffer rule of the object stages (csrc/seg_args.h) does not refuse a legitimate arena: for seg_components, seg_rle
and seg_match every output and the workspace are carved back to back out of ONE allocation, each padded only to its
required alignment, so that neighbours touch end to start -- and the results are bit-equal to the references these
stages' own GPU tests use (components_ref, rle_ref, match_ref).  B = 2, H = 5, W = 7, cap = 4, max_runs = max_records =
max_pairs = 35; two classes, diagonal touches, objects on the last column, and more objects than cap in the second image."""
import numpy as np
import pytest
import torch

import components_ref as cr
import match_ref as mr
import rle_ref as rr

pytestmark = pytest.mark.gpu

B, H, W, CAP, NLAB, ROWS, MIN_AREA = 2, 5, 7, 4, 2, 35, 2
GUARD, SENT = 64, 0xA5

LABELS = np.array([[[1, 1, 0, 0, 2, 0, 0],
                    [1, 0, 0, 2, 0, 0, 1],
                    [0, 1, 0, 0, 0, 0, 1],
                    [0, 0, 2, 2, 0, 0, 1],
                    [0, 0, 0, 0, 0, 0, 0]],
                   [[2, 0, 1, 0, 2, 0, 1],
                    [0, 0, 1, 0, 0, 0, 1],
                    [1, 0, 0, 0, 2, 2, 0],
                    [0, 1, 0, 0, 0, 0, 2],
                    [0, 0, 0, 1, 1, 0, 2]]], np.uint8)
GT = LABELS.copy()
GT[0, 0, 1], GT[0, 4, 0], GT[0, 3, 6], GT[1, 2, 5], GT[1, 4, 2] = 0, 255, 0, 0, 1


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


class Arena:
    """Tensors carved back to back out of one uint8 allocation filled with 0xA5, between two guards: each starts at the
    first multiple of its alignment behind its predecessor's end."""

    def __init__(self, fields):
        at, self.where = GUARD, {}
        for name, (shape, dtype, align) in fields.items():
            at += -at % align
            nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
            self.where[name] = (at, nbytes, shape, dtype)
            at += nbytes
        self.raw = torch.full((at + GUARD,), SENT, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.t = {name: self.raw[o:o + n].view(dtype).view(shape) for name, (o, n, shape, dtype) in self.where.items()}

    def check(self):
        """No byte between the buffers, in front of the first or behind the last was written."""
        used = torch.zeros_like(self.raw, dtype=torch.bool)
        for o, n, _, _ in self.where.values():
            assert not used[o:o + n].any()
            used[o:o + n] = True
        assert (self.raw[~used] == SENT).all()
        spans = sorted((o, o + n) for o, n, _, _ in self.where.values())
        assert any(a[1] == b[0] for a, b in zip(spans, spans[1:]))       # neighbours do touch


def _components(ops, labels, gt):
    i32, u8 = torch.int32, torch.uint8
    ar = Arena(dict(ids=((B, H, W), i32, 4), n=((B, 2), i32, 4), filtered=((B, H, W), u8, 1), stats=((B, CAP, 8), i32, 4),
                    counts=((B, 2, NLAB + 1), torch.int64, 8), ws=((ops.seg_components_workspace(B, H, W),), u8, 4)))
    t = ar.t
    ops.seg_components(torch.from_numpy(labels).cuda(), t["ids"], t["n"], t["ws"], filtered=t["filtered"], stats=t["stats"],
                       gt=torch.from_numpy(gt).cuda(), counts=t["counts"], connectivity=8, min_area=MIN_AREA, nlabels=NLAB)
    torch.cuda.synchronize()
    ar.check()
    want = cr.components(labels, 8, MIN_AREA, CAP, gt=gt, nlabels=NLAB)
    for k in ("ids", "n", "filtered", "stats", "counts"):
        got = t[k].cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    return ar, want


def test_components_runs_and_matches_in_one_allocation_each(ops):
    i32 = torch.int32
    pred, pw = _components(ops, LABELS, GT)
    truth, gw = _components(ops, GT, GT)
    assert pw["n"][1, 0] > CAP and pw["n"][0, 0] == CAP and (pw["n"][:, 1] > pw["n"][:, 0]).any()   # above cap; filtered

    for order in ("column", "row"):
        ar = Arena(dict(runs=((B, ROWS, 2), i32, 4), run_off=((B, CAP + 1), i32, 4), nruns=((B, 2), i32, 4),
                        ws=((ops.seg_rle_workspace(B, H, W, CAP, ROWS, order),), torch.uint8, 4)))
        t = ar.t
        ops.seg_rle(pred.t["ids"], t["runs"], t["run_off"], t["nruns"], t["ws"], CAP, order)
        torch.cuda.synchronize()
        ar.check()
        want = rr.rle(pw["ids"], CAP, ROWS, order)
        assert np.array_equal(t["nruns"].cpu().numpy(), want["nruns"]) and np.array_equal(t["run_off"].cpu().numpy(), want["run_off"])
        runs = t["runs"].cpu().numpy()
        for b, w in enumerate(want["runs"]):
            assert len(w) > 0 and np.array_equal(runs[b, :len(w)], w), (order, b)
            assert (runs[b, len(w):].view(np.uint8) == SENT).all()       # rows behind kept are left as they were

    ar = Arena(dict(pairs=((B, ROWS, 3), i32, 4), pair_off=((B, CAP + 2), i32, 4), area=((B, 2 * CAP + 2), i32, 4),
                    match=((B, CAP, 3), i32, 4), gmatch=((B, CAP), i32, 4), pq=((B, NLAB + 1, 4), torch.int64, 8),
                    n=((B, 4), i32, 4), ws=((ops.seg_match_workspace(B, H, W, CAP, CAP, ROWS, ROWS),), torch.uint8, 4)))
    t = ar.t
    ops.seg_match(pred.t["ids"], truth.t["ids"], t["pairs"], t["pair_off"], t["area"], t["match"], t["gmatch"], t["pq"], t["n"],
                  t["ws"], ROWS, pstats=pred.t["stats"], gstats=truth.t["stats"], skip=torch.from_numpy(GT).cuda())
    torch.cuda.synchronize()
    ar.check()
    want = mr.match(pw["ids"], gw["ids"], CAP, CAP, NLAB, ROWS, ROWS, pstats=pw["stats"], gstats=gw["stats"], skip=GT)
    assert want["pq"][:, 1:, 0].sum() > 0                                 # something did match
    for k in ("n", "pair_off", "area", "match", "gmatch", "pq"):
        got = t[k].cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    pairs = t["pairs"].cpu().numpy()
    for b, w in enumerate(want["pairs"]):
        assert np.array_equal(pairs[b, :len(w)], w), b
