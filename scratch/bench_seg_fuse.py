"""Times the segmentation output-side entry points of whichever library DFW_LIB names (default: the in-tree one), at the
shapes of scratch/bench_nway.py, bench_candidates.py, bench_native.py, bench_nway_native.py, bench_candidates_native.py.
One JSON line per case: per-call ms (median / min / p10 / p90 over windows of CALLS calls between device events) and a
sha256 of every output, so two libraries' results can be compared bit for bit.  TS_ONLY="case;case" restricts the run to
those cases (exact names), e.g. under `rocprofv3 --kernel-trace --stats`.

    [DFW_LIB=<library of another build>] python scratch/bench_seg_fuse.py TAG OUT.jsonl
"""
import hashlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffews_amd import _lib, ops  # noqa: E402
from diffews_amd.input_pipeline import NativeTargets  # noqa: E402
import bench_native as bn  # noqa: E402
import bench_nway_native as bnn  # noqa: E402

WARM, WINDOWS, CALLS = 20, 30, 20
S = 512


def digest(r):
    h = hashlib.sha256()

    def feed(v):
        if v is None:
            h.update(b"none")
        elif isinstance(v, torch.Tensor):
            h.update(v.detach().cpu().contiguous().numpy().tobytes())
        elif isinstance(v, dict):
            for k in sorted(v):
                if k != "sizes":
                    feed(v[k])
        elif isinstance(v, (list, tuple)):
            for x in v:
                feed(x)
    feed(r)
    return h.hexdigest()[:16]


ONLY = [s for s in os.environ.get("TS_ONLY", "").split(";") if s]   # exact case names; empty: all


def run(name, fn, out):
    if ONLY and name not in ONLY:
        return
    r = fn()
    torch.cuda.synchronize()
    d = digest(r)
    del r
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(WINDOWS):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        e.record()
        e.synchronize()
        ts.append(a.elapsed_time(e) / CALLS)
    ts.sort()
    row = dict(case=name, median_ms=round(statistics.median(ts), 5), min_ms=round(ts[0], 5),
               p10_ms=round(ts[len(ts) // 10], 5), p90_ms=round(ts[(9 * len(ts)) // 10], 5), digest=d)
    out.write(json.dumps(row) + "\n")
    out.flush()
    print(json.dumps(row), flush=True)


def main():
    tag, path = sys.argv[1], sys.argv[2]
    assert torch.cuda.is_available()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    out = open(path, "a")
    out.write(json.dumps(dict(tag=tag, lib=_lib.LIB_PATH)) + "\n")
    g = torch.Generator().manual_seed(1)
    # seg_postprocess with gt (seg_zero + seg_u8 + seg_count)
    x = (torch.rand(4, 3, S, S, generator=g) * 2.4 - 1.2).cuda()
    gtb = torch.randint(0, 2, (4, S, S), generator=g).to(torch.uint8)
    gtb[torch.rand(4, S, S, generator=g) < 0.05] = 255
    gtb = gtb.cuda()
    run("seg_postprocess b4 gt", lambda: ops.seg_postprocess(x, gtb), out)
    # seg_labels: bench_nway's (N, b)
    for N, b in [(5, 2), (3, 1)]:
        seg = bn.smooth_masks(N * b, S, 10 + N).view(N, b, 3, S, S).cuda()
        mx = seg.view(N * b, -1).max(dim=1).values.to(torch.int32).contiguous()
        gt = torch.randint(0, N + 1, (b, S, S), generator=g).to(torch.uint8).cuda()
        run(f"seg_labels N{N} b{b} gt", lambda: ops.seg_labels(seg, mx, gt), out)
        run(f"seg_labels N{N} b{b} gt batch_max", lambda: ops.seg_labels(seg, mx, gt, batch_max=True), out)
    # seg_labels_cand: bench_candidates' b 4, k (3, 1, 2, 2) of 8
    ks = [3, 1, 2, 2]
    E = sum(ks)
    off = [0]
    for k in ks:
        off.append(off[-1] + k)
    rs = np.random.RandomState(3)
    lab = [int(v) for k in ks for v in sorted(rs.choice(8, k, replace=False) + 1)]
    tab_host = torch.tensor(off + lab, dtype=torch.int32)
    tab = tab_host.cuda()
    seg = bn.smooth_masks(E, S, 21).cuda()
    mx = seg.view(E, -1).max(dim=1).values.to(torch.int32).contiguous()
    gt = torch.randint(0, 9, (4, S, S), generator=g).to(torch.uint8).cuda()
    run("seg_labels_cand b4 k3122 gt area", lambda: ops.seg_labels_cand(seg, mx, tab, tab_host, 8, gt, want_area=True), out)
    run("seg_labels_cand b4 k3122", lambda: ops.seg_labels_cand(seg, mx, tab, tab_host, 8), out)
    # seg_native: bench_native's batch
    seg = bn.smooth_masks(4, S, 3).cuda()
    gts = [rs.choice([0, 7, 7, 9, 255], size=s, p=[.4, .25, .25, .05, .05]).astype(np.uint8) for s in bn.SIZES]
    t = NativeTargets((S, S), bn.SIZES, gt=gts, class_value=7, ignore_value=255)
    run("seg_native b4 gt", lambda: ops.seg_native(seg, t), out)
    # seg_labels_native: bench_nway_native's N
    b = len(bnn.SIZES)
    for N in bnn.CLASSES:
        seg = bnn.smooth_masks(N * b, S, 3 + N).view(N, b, 3, S, S).cuda()
        gts = [rs.randint(0, N + 1, size=s).astype(np.uint8) for s in bnn.SIZES]
        for gg in gts:
            gg[rs.rand(*gg.shape) < 0.05] = 255
        t = NativeTargets((S, S), bnn.SIZES, gt=gts, ignore_value=255)
        run(f"seg_labels_native N{N} b4 gt", lambda: ops.seg_labels_native(seg, t), out)
        if N == 5:
            ids = [11, 300, 11, 7, 1000][:N]
            g32 = [rs.choice([0, 7, 11, 300, 1000, 255], size=s).astype(np.int32) for s in bnn.SIZES]
            t32 = NativeTargets((S, S), bnn.SIZES, gt=g32, ignore_value=255)
            run(f"seg_labels_native N{N} b4 gt int32 class_ids", lambda: ops.seg_labels_native(seg, t32, class_ids=ids), out)
    # seg_labels_cand_native: bench_candidates_native's k
    for k in [2, 5, 20]:
        E = b * k
        seg = bnn.smooth_masks(E, S, 3 + k).cuda()
        gts = [rs.randint(0, k + 1, size=s).astype(np.uint8) for s in bnn.SIZES]
        for gg in gts:
            gg[rs.rand(*gg.shape) < 0.05] = 255
        off, lab = [q * k for q in range(b + 1)], [1 + p for _ in range(b) for p in range(k)]
        tab_host = torch.tensor(off + lab, dtype=torch.int32)
        tab = tab_host.cuda()
        t = NativeTargets((S, S), bnn.SIZES, gt=gts, ignore_value=255)
        run(f"seg_labels_cand_native k{k} b4 gt", lambda: ops.seg_labels_cand_native(seg, t, tab, tab_host, k), out)
        if k == 5:
            eids = [int(v) for v in rs.choice([3, 9, 400], size=E)]
            run(f"seg_labels_cand_native k{k} b4 gt entry_ids area",
                lambda: ops.seg_labels_cand_native(seg, t, tab, tab_host, k, entry_ids=eids, want_area=True), out)
    out.close()


if __name__ == "__main__":
    main()
