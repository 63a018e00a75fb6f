"""Simplified rings on the device (ops.seg_contours with the simp_ buffers and tol4) against the same call without the
stage, and against what a caller does without it: copy every corner to the host and run a tolerance simplification there,
ring by ring.

One shape, 4096 x 4096 with B = 1, ids from ops.seg_components (not timed, 1024 stats rows) on the contents of
scratch/bench_components.py -- empty, one component over the whole image, random blobs of three classes -- and one map
with a long diagonal staircase edge: the lower left triangle of 4000 x 4000, one ring of 8002 corners served by a single
workgroup, the stage's expected weak spot.  Tolerances 0.5, 1 and 2 pixels.

  device: one ops.seg_contours call into a resident objects.ContourBuffers(simplify=True), device events around it, with
          and without the stage; objects.contours_to_host on both forms of the result, host clock;
  host:   D2H of the tables and the corners (what contours_to_host copies), then tests/simplify_ref.py's level-synchronous
          form on the rings of the first --host-rings rings (default 64), scaled by the corners to all rings and marked
          "scaled" when that is fewer than all -- interpreted Python, the order of magnitude of a first host implementation
          and no more.  shapely's simplify is timed as well when shapely is installed.
Medians over --reps (default 20); the host side is timed once.  One JSON line per row, and with --md the table of
profiles/object_simplify_timing.md on stdout.

    python scratch/bench_object_simplify.py [--reps 20] [--host-rings 64] [--md]
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
TOLERANCES = (0.5, 1.0, 2.0)


def staircase(B, H, W, n=4000):
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    return ((xx <= yy) & (yy < n) & (xx < n)).to(torch.uint8).expand(B, H, W).contiguous()


def host_simplify(rings, verts, tol4, limit):
    """(seconds scaled to all rings, rings timed, shapely seconds or None) on the host copies of one image."""
    import simplify_ref as sr
    take = rings[:limit]
    t0 = time.perf_counter()
    for _, first, count, _ in take.tolist():
        sr.simplify_rounds(verts[first:first + count], tol4)
    dt = time.perf_counter() - t0
    done, total = int(take[:, 2].sum()) if len(take) else 0, int(rings[:, 2].sum()) if len(rings) else 0
    scaled = dt * (total / done) if done else 0.0
    shp = None
    try:
        from shapely.geometry import LinearRing
        t0 = time.perf_counter()
        for _, first, count, _ in rings.tolist():
            LinearRing(verts[first:first + count]).simplify(tol4 / 4.0, preserve_topology=False)
        shp = time.perf_counter() - t0
    except ImportError:
        pass
    return scaled, len(take), shp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-rings", type=int, default=64)
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
    buf = ContourBuffers(B, H, W, CAP, simplify=True)
    cases = [(name, conn, lab) for name, conn, lab in contents(B, H, W) if not name.startswith("checkerboard")]
    cases.append(("staircase edge of 4000 pixels", 8, staircase(B, H, W)))
    rows = []
    for name, conn, lab in cases:
        ops.seg_components(lab, cb.ids, cb.n, cb.ws, stats=cb.stats, connectivity=conn)
        full = dict(verts=buf.verts, rings=buf.rings, ring_off=buf.ring_off, n=buf.n, shape=(H, W), connectivity=conn)
        simp = dict(full, verts=buf.simp_verts, rings=buf.simp_rings, n=buf.simp_n)

        def device(tol4):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if tol4 is None:
                ops.seg_contours(cb.ids, buf.verts, buf.rings, buf.ring_off, buf.n, buf.ws, CAP, conn)
            else:
                ops.seg_contours(cb.ids, buf.verts, buf.rings, buf.ring_off, buf.n, buf.ws, CAP, conn, buf.simp_verts, buf.simp_rings,
                                 buf.simp_n, tol4)
            e.record()
            e.synchronize()
            return a.elapsed_time(e)

        def to_host(c):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            contours_to_host(c)
            return (time.perf_counter() - t0) * 1e3
        device(None)
        off = med([device(None) for _ in range(args.reps)])
        for tol in TOLERANCES:
            tol4 = int(tol * 4)
            device(tol4)                                                    # warm-up: code objects, first touch of the buffers
            to_host(full), to_host(simp)
            on = med([device(tol4) for _ in range(args.reps)])
            t_full, t_simp = to_host(full), to_host(simp)
            found, corners, nrings, complete = buf.n[0].tolist()
            _, kept, _, _ = buf.simp_n[0].tolist()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hr, hv = buf.rings[0, :nrings].cpu().numpy(), buf.verts[0, :corners].cpu().numpy()
            d2h = (time.perf_counter() - t0) * 1e3
            th, timed, shp = host_simplify(hr, hv, tol4, args.host_rings)
            row = dict(shape=[B, H, W], content=name, tolerance=tol, max_edges=buf.max_edges, edges_found=found, rings=nrings,
                       corners_in=corners, corners_kept=kept, complete=bool(complete), reps=args.reps, device_off_ms=off, device_on_ms=on,
                       stage_ms=round(on - off, 3), to_host_full_ms=round(t_full, 3), to_host_simplified_ms=round(t_simp, 3),
                       d2h_corners_ms=round(d2h, 3), host_route_ms=round(d2h + th * 1e3, 3), host_rings_timed=timed,
                       host_scaled=timed < nrings, shapely_ms=None if shp is None else round(shp * 1e3, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.md:
        print("| content | tolerance, px | rings | corners in | corners kept | call without the stage, median ms | with it, median ms | "
              "`contours_to_host`, full, ms | simplified, ms | D2H of the corners, ms | D2H + tests/simplify_ref.py, ms (rings timed) |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['content']} | {r['tolerance']} | {r['rings']} | {r['corners_in']} | {r['corners_kept']} | {r['device_off_ms']} | "
                  f"{r['device_on_ms']} | {r['to_host_full_ms']} | {r['to_host_simplified_ms']} | {r['d2h_corners_ms']} | "
                  f"{r['host_route_ms']} ({r['host_rings_timed']}{', scaled' if r['host_scaled'] else ''}) |")


if __name__ == "__main__":
    main()
