"""Per-object confidence on the device (ops.seg_scores) against what a caller does without it: copy the int32 id map, the
label map and the uint8 mask planes to the host and reduce them with np.bincount and np.minimum.at / np.maximum.at.

One shape, 4096 x 4096 with B = 1, N = 3 class-major planes of random bytes, ids from ops.seg_components (not timed) on the
contents of scratch/bench_components.py: empty, one component over the whole image (every workgroup adds to ONE row: the
contention case), random blobs of three classes (about 6700 objects, the first --cap scored) and the 4-connected
checkerboard (a run per pixel; only the first --cap of its 8.4 M one-pixel objects are scored).  --cap objects (default 1024).

  device: one ops.seg_scores call into a resident objects.ScoreBuffers, device events around it; and
          objects.scores_to_host on the result, host clock (its one copy);
  host:   D2H of ids, labels and planes, the plane sum gathered by label, np.bincount with weights and
          np.minimum.at / np.maximum.at over the counted pixels, host clock from after a device synchronise.
The tables of the two routes are compared and must be equal.  Medians over --reps (default 20); the host side is timed
--host-reps times (default 1).  One JSON line per row, and with --md the table of profiles/object_scores_timing.md on
stdout.

    python scratch/bench_object_scores.py [--reps 20] [--host-reps 1] [--cap 1024] [--md]
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
NLAB = 3


def host_route(ids, labels, u8, table, cap):
    """The reduction on the host, after the copies: int64 [cap, 4]."""
    ids, labels = ids.reshape(-1), labels.reshape(-1).astype(np.int64)
    P = u8.shape[0]
    row = np.concatenate([table, np.full(256 - len(table), -1, table.dtype)])
    row[0] = -1
    g = row[labels]
    q = np.flatnonzero((ids >= 1) & (ids <= cap) & (g >= 0) & (g < P))
    out = np.zeros((cap, 4), np.int64)
    if len(q) == 0:
        return out
    flat = u8.reshape(P, 3, -1)
    gq = g[q]
    v = flat[gq, 0, q].astype(np.int64) + flat[gq, 1, q] + flat[gq, 2, q]
    k = ids[q] - 1
    out[:, 0] = np.bincount(k, weights=v, minlength=cap).astype(np.int64)
    out[:, 1] = np.bincount(k, minlength=cap)
    lo, hi = np.full(cap, 766, np.int64), np.zeros(cap, np.int64)
    np.minimum.at(lo, k, v)
    np.maximum.at(hi, k, v)
    out[:, 2], out[:, 3] = np.where(out[:, 1] > 0, lo, 0), hi
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--md", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from bench_components import contents
    from diffews_amd import ops
    from diffews_amd.objects import ComponentBuffers, ScoreBuffers, planes_for_classes, scores_to_host
    torch.set_num_threads(16)
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    B, H, W = SHAPE
    cap = args.cap
    cb, sb = ComponentBuffers(B, H, W, cap), ScoreBuffers(B, cap, NLAB)
    table = planes_for_classes(NLAB, B)
    sb.stage(table)
    u8 = torch.randint(0, 256, (NLAB, B, 3, H, W), dtype=torch.uint8, device="cuda",
                       generator=torch.Generator(device="cuda").manual_seed(11))
    rows = []
    for name, conn, lab in contents(B, H, W):
        ops.seg_components(lab, cb.ids, cb.n, cb.ws, filtered=cb.labels, stats=cb.stats, connectivity=conn)

        def call():
            ops.seg_scores(cb.ids, cb.labels, u8.view(-1, 3, H, W), sb.planes, sb.planes_host, sb.scores, sb.ws)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        td, tc = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            td.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            host = scores_to_host(dict(scores=sb.scores))
            tc.append((time.perf_counter() - t0) * 1e3)
        th, d2h = [], []
        for _ in range(args.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids, labels, planes = cb.ids.cpu().numpy(), cb.labels.cpu().numpy(), u8.cpu().numpy()
            d2h.append((time.perf_counter() - t0) * 1e3)
            want = host_route(ids[0], labels[0], planes.reshape(-1, 3, H, W), table[0].numpy(), cap)
            th.append((time.perf_counter() - t0) * 1e3)
        got = np.stack([host[k][0] for k in ("sum", "n", "min", "max")], 1)
        assert np.array_equal(got, want), name                                    # the two routes agree on every row
        rows.append(dict(content=name, shape=[B, H, W], cap=cap, objects=int(cb.n[0, 0]), scored=int((want[:, 1] > 0).sum()),
                         counted_pixels=int(want[:, 1].sum()), reps=args.reps, device_ms=med(td), scores_to_host_ms=med(tc),
                         d2h_ms=med(d2h), host_route_ms=med(th), host_reps=args.host_reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.md:
        print("| content | objects | rows scored | counted pixels | device `seg_scores`, median ms | `scores_to_host`, ms | "
              "D2H of ids, labels, planes, ms | D2H + numpy reduction, ms |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['content']} | {r['objects']} | {r['scored']} | {r['counted_pixels']} | {r['device_ms']} | "
                  f"{r['scores_to_host_ms']} | {r['d2h_ms']} | {r['host_route_ms']} |")


if __name__ == "__main__":
    main()
