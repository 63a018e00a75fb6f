"""Run-length encoding of labelled objects on the device (ops.seg_rle) against what a caller does without it: copy the
int32 id map to the host and run-length encode it in numpy, once per object.

One shape, 4096 x 4096 with B = 1, on the contents of scratch/bench_components.py -- empty, one component over the whole
image, random blobs of three classes (a smooth random field, thresholded) -- in both orders, 1024 objects encoded, the
default max_runs of objects.RunBuffers.  The checkerboard (8.4 M objects of one pixel) is left out of the default set:
with the default max_runs it exercises nothing but the truncation; --checkerboard adds it.

  device: ops.seg_components once (not timed), then one ops.seg_rle call into a resident objects.RunBuffers, device events
          around it; and objects.runs_to_host on the result, host clock (its two copies and the split per object);
  host:   D2H of the ids, then per object 1..min(n, 1024) the runs of (ids == k) over the flattened map with np.diff, host
          clock from after a device synchronise.  The per-object loop is bounded by --host-objects (default 32) and the
          time scaled to all objects, because thousands of passes over 16.8 M pixels take minutes.
Medians over --reps (default 20); the host side is timed --host-reps times.  One JSON line per row, and with --md the
table of profiles/object_runs_timing.md on stdout.

    python scratch/bench_object_runs.py [--reps 20] [--host-reps 1] [--host-objects 32] [--checkerboard] [--md]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPE = (1, 4096, 4096)
CAP = 1024


def host_runs(flat, k):
    on = np.concatenate([[False], flat == k, [False]])
    edge = np.flatnonzero(on[1:] != on[:-1])
    return np.stack([edge[::2], edge[1::2] - edge[::2]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-objects", type=int, default=32)
    ap.add_argument("--checkerboard", action="store_true")
    ap.add_argument("--md", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from bench_components import contents
    from diffews_amd import ops
    from diffews_amd.objects import ComponentBuffers, RunBuffers, runs_to_host
    torch.set_num_threads(16)
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    B, H, W = SHAPE
    cb = ComponentBuffers(B, H, W, CAP)
    rows = []
    for name, conn, lab in contents(B, H, W):
        if name.startswith("checkerboard") and not args.checkerboard:
            continue
        ops.seg_components(lab, cb.ids, cb.n, cb.ws, stats=cb.stats, connectivity=conn)
        n = int(cb.n[0, 0])
        for order in ("column", "row"):
            rb = RunBuffers(B, H, W, CAP, order=order)
            rr = dict(runs=rb.runs, run_off=rb.run_off, nruns=rb.nruns, order=order, shape=(H, W))

            def device():
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ops.seg_rle(cb.ids, rb.runs, rb.run_off, rb.nruns, rb.ws, CAP, order)
                e.record()
                e.synchronize()
                return a.elapsed_time(e)

            def to_host():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = runs_to_host(rr)
                return (time.perf_counter() - t0) * 1e3, out

            def host():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = cb.ids.cpu().numpy()[0]
                t1 = time.perf_counter()
                flat = (h if order == "row" else np.ascontiguousarray(h.T)).reshape(-1)
                t2 = time.perf_counter()
                ks = list(range(1, min(n, CAP) + 1))[:args.host_objects]
                got = [host_runs(flat, k) for k in ks]
                per = (time.perf_counter() - t2) / max(1, len(ks))
                return (t1 - t0) * 1e3, ((t2 - t0) + per * min(n, CAP)) * 1e3, got
            device()                                                        # warm-up: code objects, first touch of the buffers
            to_host()
            td = [device() for _ in range(args.reps)]
            tc, d2h, th, got = [], [], [], []
            for _ in range(max(1, args.host_reps)):
                t, (per_image, truncated) = to_host()
                tc.append(t)
                c, t, got = host()
                d2h.append(c)
                th.append(t)
            same = all(np.array_equal(g, p) for g, p in zip(got, per_image[0]))
            kept, found = rb.nruns[0].tolist()
            row = dict(shape=[B, H, W], content=name, order=order, objects=n, encoded=min(n, CAP), runs_found=found, runs_kept=kept,
                       truncated=truncated, reps=args.reps, device_ms=med(td), runs_to_host_ms=med(tc), d2h_ids_ms=med(d2h),
                       host_route_ms=med(th), host_objects_timed=min(min(n, CAP), args.host_objects), same_runs=same,
                       d2h_mb=round(cb.ids.numel() * 4 / 1e6, 1), runs_mb=round(kept * 8 / 1e6, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.md:
        print("| content | order | objects encoded | runs | device `seg_rle`, median ms | `runs_to_host`, ms | D2H of the ids, ms | "
              "D2H + numpy RLE per object, ms (scaled from the objects timed) |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['content']} | {r['order']} | {r['encoded']} | {r['runs_kept']}{' of ' + str(r['runs_found']) if r['truncated'] else ''} "
                  f"| {r['device_ms']} | {r['runs_to_host_ms']} | {r['d2h_ids_ms']} | {r['host_route_ms']} ({r['host_objects_timed']}) |")


if __name__ == "__main__":
    main()
