"""Boundary bands on the device (ops.seg_boundary, ops.seg_boundary_counts) against what a caller does without them: copy
the map to the host and run d iterations of a 3 x 3 erosion per value.

One shape, 4096 x 4096 with B = 1, d = dmax = 116 (2 % of the diagonal), on the contents of scratch/bench_components.py:
empty, one component, random blobs of three classes (about 6700 objects) and the 4-connected checkerboard -- each as the
uint8 label map and as the int32 id map ops.seg_components makes of it.

  device: one ops.seg_boundary call (two launches, dist and band) into a resident objects.BoundaryBuffers, device events
          around it; ops.seg_boundary_counts alone (the label map against a ground truth shifted by three pixels, both dist
          maps resident); and ops.seg_components on the same label map, for scale;
  host:   D2H of the map, then for the LABEL map, per value, --host-iters iterations of scipy.ndimage.binary_erosion
          (border_value=0; numpy shifts where scipy does not import) -- timed once and SCALED to d iterations, which the
          output says; the eroded mask of --host-iters iterations is compared with the device's dist > --host-iters.
          For the id map only the copy is timed: per-value erosion of thousands of ids is not a route anyone would run.
Medians over --reps (default 20).  One JSON line per row, and with --md the table of profiles/object_boundaries_timing.md
on stdout.

    python scratch/bench_object_boundaries.py [--reps 20] [--host-iters 4] [--md]
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


def erode_shifts(mask):
    H, W = mask.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = mask
    out = np.ones((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + H, dx:dx + W]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=4)
    ap.add_argument("--md", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from bench_components import contents
    from diffews_amd import metrics, ops
    from diffews_amd.objects import BoundaryBuffers, ComponentBuffers
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    torch.set_num_threads(16)
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    B, H, W = SHAPE
    d = metrics.boundary_width(H, W)
    k = args.host_iters
    cb = ComponentBuffers(B, H, W, 1024)
    bufs = {torch.uint8: BoundaryBuffers(B, H, W, d, torch.uint8), torch.int32: BoundaryBuffers(B, H, W, d, torch.int32)}
    gb = BoundaryBuffers(B, H, W, d, torch.uint8)
    counts = torch.empty(B, 2, NLAB + 1, dtype=torch.int64, device="cuda")

    def timed(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        t = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        return med(t)

    rows = []
    for name, conn, lab in contents(B, H, W):
        t_comp = timed(lambda: ops.seg_components(lab, cb.ids, cb.n, cb.ws, filtered=cb.labels, stats=cb.stats, connectivity=conn))
        gt = torch.roll(lab, (3, 3), (1, 2)).contiguous()
        ops.seg_boundary(gt, gb.dist, gb.ws, d, band=gb.band, d=d)
        for m in (lab, cb.ids):
            bb = bufs[m.dtype]
            t_dev = timed(lambda: ops.seg_boundary(m, bb.dist, bb.ws, d, band=bb.band, d=d))
            row = dict(content=name, map=str(m.dtype).replace("torch.", ""), shape=[B, H, W], d=d, reps=args.reps,
                       objects=int(cb.n[0, 0]), band_pixels=int(((bb.dist >= 1) & (bb.dist <= d)).sum()),
                       deeper_pixels=int((bb.dist == d + 1).sum()), seg_boundary_ms=t_dev, seg_components_ms=t_comp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = m.cpu().numpy()
            row["d2h_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            if m.dtype == torch.uint8:
                row["seg_boundary_counts_ms"] = timed(lambda: ops.seg_boundary_counts(lab, bb.dist, gt, gb.dist, counts, d))
                dist = bb.dist.cpu().numpy()[0]
                t0 = time.perf_counter()
                values = [v for v in np.unique(host) if v != 0]
                eroded = {}
                for v in values:
                    mask = host[0] == v
                    if ndi is not None:
                        eroded[v] = ndi.binary_erosion(mask, np.ones((3, 3), bool), iterations=k, border_value=0)
                    else:
                        for _ in range(k):
                            mask = erode_shifts(mask)
                        eroded[v] = mask
                t_host = (time.perf_counter() - t0) * 1e3
                for v in values:
                    assert np.array_equal(eroded[v], (host[0] == v) & (dist > k)), (name, int(v))   # the two routes agree
                row.update(values=len(values), host_iters=k, host_erosion_ms=round(t_host, 3),
                           host_route_scaled_ms=round(row["d2h_ms"] + t_host * d / k, 1), erosion="scipy" if ndi is not None else "numpy")
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.md:
        print("| content | map | objects | band pixels | deeper than d | `seg_boundary`, median ms | `seg_boundary_counts`, ms | "
              "`seg_components`, ms | D2H of the map, ms | erosion, values × iterations timed, ms | host route scaled to d iterations, ms |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['content']} | {r['map']} | {r['objects']} | {r['band_pixels']} | {r['deeper_pixels']} | {r['seg_boundary_ms']} | "
                  f"{r.get('seg_boundary_counts_ms', '—')} | {r['seg_components_ms']} | {r['d2h_ms']} | "
                  + (f"{r['values']} × {r['host_iters']}: {r['host_erosion_ms']} ({r['erosion']}) | {r['host_route_scaled_ms']} |"
                     if "values" in r else "not timed | not timed |"))


if __name__ == "__main__":
    main()
