"""Candidate classes per query at native size: the device stage (ops.seg_labels_cand_native) against the host route on the
same box.

b = 4 queries at 512 x 512 -> 427x640, 480x640, 427x640, 480x640 (h x w), k in {2, 5, 20} candidates per query (E = 4 k
entries, labels = 1 + position), uint8 label ground truth with 255 = ignore:
  device: ops.seg_labels_cand_native on a device-resident seg_u8 [E, 3, S, S] with the targets and the table staged
          beforehand (the four launches plus the allocation of the packed outputs and scratch), timed with device events;
  host:   seg_u8 D2H (E * 3 * S * S bytes), PIL resize per entry, then the label rule and counts per query in vectorised
          numpy (the same fp32 expressions, entries ascending, strictly larger takes over), 16 threads, host clock.
Labels and counts of the two are asserted equal before anything is timed.  Medians over --reps, the two sides
interleaved; one JSON line per k, and with --md the table of profiles/candidates_native_timing.md on stdout.

    python scratch/bench_candidates_native.py [--reps 20] [--md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_nway_native import SIZES, smooth_masks  # noqa: E402

CANDIDATES = [2, 5, 20]
F = np.float32


def host_route(seg_cpu, off, lab, nlabels, gts, r_threshold=0.25):
    """(labels [uint8 [h, w]], counts int64 [B, 2, nlabels+1]) from host bytes: PIL per entry, numpy per query."""
    import native_ref as nr
    labels, counts = [], np.zeros((len(SIZES), 2, nlabels + 1), np.int64)
    for q, (h, w) in enumerate(SIZES):
        best = np.full((h, w), -1.0, F)
        out = np.zeros((h, w), np.uint8)
        for e in range(off[q], off[q + 1]):
            r = nr.resize_u8(seg_cpu[e], h, w).numpy()
            thr = F(int(r.max())) / F(255.0) * F(r_threshold)
            u = r.astype(F) / F(255.0)
            sc = ((u[0] + u[1]) + u[2]) / F(3.0)
            take = (sc > thr) & (sc > best)
            best = np.where(take, sc, best)
            out = np.where(take, np.uint8(lab[e]), out)
        g = gts[q]
        keep = g <= nlabels
        p, t = out[keep].astype(np.int64), g[keep].astype(np.int64)
        pred, gth = np.bincount(p, minlength=nlabels + 1), np.bincount(t, minlength=nlabels + 1)
        inter = np.bincount(p[p == t], minlength=nlabels + 1)
        counts[q, 0], counts[q, 1] = inter, pred + gth - inter
        labels.append(out)
    return labels, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from diffews_amd import ops
    from diffews_amd.input_pipeline import NativeTargets
    torch.set_num_threads(16)
    S, b = 512, len(SIZES)
    rows = []
    for k in CANDIDATES:
        E = b * k
        seg = smooth_masks(E, S, 3 + k)
        rs = np.random.RandomState(4 + k)
        gts = [rs.randint(0, k + 1, size=s).astype(np.uint8) for s in SIZES]
        for g in gts:
            g[rs.rand(*g.shape) < 0.05] = 255
        off, lab = [q * k for q in range(b + 1)], [1 + p for _ in range(b) for p in range(k)]
        tab_host = torch.tensor(off + lab, dtype=torch.int32)
        segd, tab = seg.cuda(), tab_host.cuda()
        t = NativeTargets((S, S), SIZES, gt=gts, ignore_value=255)

        def device_stage():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = ops.seg_labels_cand_native(segd, t, tab, tab_host, k)
            e.record()
            e.synchronize()
            return a.elapsed_time(e), r

        def host():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = host_route(segd.cpu(), off, lab, k, gts)
            return (time.perf_counter() - t0) * 1e3, r
        rd, (hl, hc) = device_stage()[1], host()[1]
        assert torch.equal(rd["counts"].cpu(), torch.from_numpy(hc)), "counts differ between the device stage and the host route"
        assert all(torch.equal(x.cpu(), torch.from_numpy(y)) for x, y in zip(rd["labels"], hl)), "labels differ"
        for _ in range(args.warmup):
            device_stage(), host()
        td, th = [], []
        for _ in range(args.reps):
            td.append(device_stage()[0])
            th.append(host()[0])
        med = lambda v: round(statistics.median(v), 4)
        row = dict(candidates=k, E=E, b=b, res=S, sizes=SIZES, reps=args.reps, device_stage_ms=med(td),
                   device_stage_min_ms=round(min(td), 4), host_route_ms=med(th), host_threads=torch.get_num_threads(),
                   equal_to_host=True, d2h_mb=round(seg.numel() / 1e6, 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.md:
        print("| candidates per query | E | device stage, median ms (min) | host route, median ms | D2H the host route needs, MB | equal to host |")
        print("|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['candidates']} | {r['E']} | {r['device_stage_ms']} ({r['device_stage_min_ms']}) | {r['host_route_ms']} | "
                  f"{r['d2h_mb']} | {r['equal_to_host']} |")


if __name__ == "__main__":
    main()
