"""Outlines of labelled objects on the device (ops.seg_contours) against what a caller does without it: copy the int32 id
map to the host and trace it there, object by object.

One shape, 4096 x 4096 with B = 1, ids from ops.seg_components (not timed, 1024 stats rows, so objects 1..1024 are
outlined) on the contents of scratch/bench_components.py -- empty, one component over the whole image, random blobs of
three classes -- and the random blobs once more with max_edges at half their edge count: a map that overflows.  The
complete cases run with objects.ContourBuffers' default max_edges (2^21 here: 21 doubling rounds, 62 launches).

  device: one ops.seg_contours call into a resident objects.ContourBuffers, device events around it;
          objects.contours_to_host on the result, host clock (its two copies and the split per object);
  host:   D2H of the ids, then a tracer.  cv2.findContours or skimage.measure.find_contours are used when one of them is
          installed; otherwise the reference tracer of tests/contours_ref.py on the bounding box of each of the first
          --host-objects objects (default 16), scaled to all objects outlined and marked "scaled" -- a Python tracer, the
          order of magnitude of a first host implementation and no more.
Medians over --reps (default 20); the host side is timed once.  One JSON line per row, and with --md the table of
profiles/object_contours_timing.md on stdout.

    python scratch/bench_object_contours.py [--reps 20] [--host-objects 16] [--md]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = (1, 4096, 4096)
CAP = 1024


def host_tracer():
    """(name, f(ids [H, W], stats rows, objects, limit) -> (seconds, objects traced))."""
    try:
        import cv2

        def trace(ids, stats, n, limit):
            t0 = time.perf_counter()
            for k in range(1, n + 1):
                cv2.findContours((ids == k).astype(np.uint8), cv2.RETR_CCOMP, cv2.CHAIN_APPROX_SIMPLE)
            return time.perf_counter() - t0, n
        return "cv2.findContours", trace
    except ImportError:
        pass
    try:
        from skimage import measure

        def trace(ids, stats, n, limit):
            t0 = time.perf_counter()
            for k in range(1, n + 1):
                measure.find_contours(ids == k, 0.5)
            return time.perf_counter() - t0, n
        return "skimage.measure.find_contours", trace
    except ImportError:
        pass
    import contours_ref as ct

    def trace(ids, stats, n, limit):
        ks = list(range(1, n + 1))[:limit]
        t0 = time.perf_counter()
        for k in ks:
            _, _, y0, x0, y1, x1 = stats[k - 1][:6]
            ct.trace((ids[y0:y1, x0:x1] == k).astype(np.int32), 1, 8)
        return (time.perf_counter() - t0) * (n / max(1, len(ks))), len(ks)
    return "tests/contours_ref.py, scaled", trace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-objects", type=int, default=16)
    ap.add_argument("--md", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from bench_components import contents
    from diffews_amd import ops
    from diffews_amd.objects import ComponentBuffers, ContourBuffers, contours_to_host
    torch.set_num_threads(16)
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    B, H, W = SHAPE
    cb = ComponentBuffers(B, H, W, CAP)
    tracer_name, tracer = host_tracer()
    full = ContourBuffers(B, H, W, CAP)
    cases = [(name, conn, lab, None) for name, conn, lab in contents(B, H, W) if not name.startswith("checkerboard")]
    cases.append(("random blobs, max_edges too small", cases[-1][1], cases[-1][2], "half"))
    rows = []
    for name, conn, lab, cut in cases:
        ops.seg_components(lab, cb.ids, cb.n, cb.ws, stats=cb.stats, connectivity=conn)
        n = min(int(cb.n[0, 0]), CAP)
        buf = full
        if cut:
            ops.seg_contours(cb.ids, full.verts, full.rings, full.ring_off, full.n, full.ws, CAP, conn)
            buf = ContourBuffers(B, H, W, CAP, max_edges=int(full.n[0, 0]) // 2 // 4 * 4)
        c = dict(verts=buf.verts, rings=buf.rings, ring_off=buf.ring_off, n=buf.n, shape=(H, W), connectivity=conn)

        def device():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.seg_contours(cb.ids, buf.verts, buf.rings, buf.ring_off, buf.n, buf.ws, CAP, conn)
            e.record()
            e.synchronize()
            return a.elapsed_time(e)

        def to_host():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = contours_to_host(c)
            return (time.perf_counter() - t0) * 1e3, out
        device()                                                            # warm-up: code objects, first touch of the buffers
        to_host()
        td = [device() for _ in range(args.reps)]
        tc, (per_image, incomplete) = to_host()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = cb.ids.cpu().numpy()[0]
        d2h = (time.perf_counter() - t0) * 1e3
        stats = cb.stats[0].cpu().numpy().tolist()
        th, traced = tracer(h, stats, n, args.host_objects)
        found, corners, rings, complete = buf.n[0].tolist()
        row = dict(shape=[B, H, W], content=name, objects=n, max_edges=buf.max_edges, edges_found=found, corners=corners,
                   rings=rings, complete=bool(complete), reps=args.reps, device_ms=med(td), contours_to_host_ms=round(tc, 3),
                   d2h_ids_ms=round(d2h, 3), host_route_ms=round(d2h + th * 1e3, 3), host_tracer=tracer_name,
                   host_objects_timed=traced, d2h_mb=round(cb.ids.numel() * 4 / 1e6, 1), verts_mb=round(corners * 8 / 1e6, 3),
                   ws_mb=round(buf.ws.numel() / 1e6, 1))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.md:
        print(f"| content | objects outlined | max_edges | edges found | rings | corners | device `seg_contours`, median ms | "
              f"`contours_to_host`, ms | D2H of the ids, ms | D2H + host tracer ({tracer_name}), ms (objects timed) |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['content']} | {r['objects']} | {r['max_edges']} | {r['edges_found']} | {r['rings']} | {r['corners']} | "
                  f"{r['device_ms']} | {r['contours_to_host_ms']} | {r['d2h_ids_ms']} | {r['host_route_ms']} ({r['host_objects_timed']}) |")


if __name__ == "__main__":
    main()
