"""Euclidean distance maps and inscribed circles on the device (ops.seg_boundary with metric="euclidean", with and without
peaks) against the chessboard call of the same library in the same process, and against what a caller does without them:
copy the map to the host and run scipy.ndimage.distance_transform_edt per value.

One shape, 4096 x 4096 with B = 1, d = dmax = 116 (2 % of the diagonal), on the contents of scratch/bench_components.py:
empty, the 4-connected checkerboard, random blobs of three classes and one component (the worst case of the column walk:
14.9 M pixels walk all 115 rows both ways).

  device: the int32 id map ops.seg_components makes of the label map, into resident objects.BoundaryBuffers, device events
          around each call, every call warmed three times (cache-warm), median of --reps:
            chessboard          ops.seg_boundary(ids, dist, ws, d, band=, d=)                          two launches
            euclidean           ... metric="euclidean"                                                 two launches
            euclidean + peaks   ... metric="euclidean", peaks=int64 [B, cap], cap = 8192               three launches
          and the same three on the uint8 label map (without peaks, which want ids);
  host:   D2H of the uint8 label map, then per value distance_transform_edt of (map == v) padded by one false pixel, once;
          its square, capped, is compared with the device's dist2 of the label map.
--chessboard-only times the chessboard call alone, for a comparison of two library builds: one process per build
(DFW_LIB=<library>), alternated by the caller.  One JSON line per row, and with --md the table of
profiles/object_thickness_timing.md on stdout.

    [DFW_LIB=<library of another build>] python scratch/bench_object_thickness.py [--reps 20] [--md] [--chessboard-only] [--no-host]
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
CAP = 8192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--md", action="store_true")
    ap.add_argument("--chessboard-only", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from bench_components import contents
    from diffews_amd import metrics, ops
    from diffews_amd.objects import BoundaryBuffers, ComponentBuffers
    torch.set_num_threads(16)
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    B, H, W = SHAPE
    d = metrics.boundary_width(H, W)
    cb = ComponentBuffers(B, H, W, 1024)
    chess = {torch.uint8: BoundaryBuffers(B, H, W, d, torch.uint8), torch.int32: BoundaryBuffers(B, H, W, d, torch.int32)}

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

    if args.chessboard_only:
        for name, conn, lab in contents(B, H, W):
            ops.seg_components(lab, cb.ids, cb.n, cb.ws, filtered=cb.labels, stats=cb.stats, connectivity=conn)
            for m in (lab, cb.ids):
                bb = chess[m.dtype]
                t = timed(lambda: ops.seg_boundary(m, bb.dist, bb.ws, d, band=bb.band, d=d))
                print(json.dumps(dict(content=name, map=str(m.dtype).replace("torch.", ""), chessboard_ms=t, reps=args.reps,
                                      lib=os.environ.get("DFW_LIB", "in-tree"))), flush=True)
        return

    eu = {torch.uint8: BoundaryBuffers(B, H, W, d, torch.uint8, metric="euclidean"),
          torch.int32: BoundaryBuffers(B, H, W, d, torch.int32, metric="euclidean", max_components=CAP)}
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    rows = []
    for name, conn, lab in contents(B, H, W):
        ops.seg_components(lab, cb.ids, cb.n, cb.ws, filtered=cb.labels, stats=cb.stats, connectivity=conn)
        for m in (lab, cb.ids):
            bc, be = chess[m.dtype], eu[m.dtype]
            row = dict(content=name, map=str(m.dtype).replace("torch.", ""), shape=[B, H, W], d=d, reps=args.reps, objects=int(cb.n[0, 0]))
            row["chessboard_ms"] = timed(lambda: ops.seg_boundary(m, bc.dist, bc.ws, d, band=bc.band, d=d))
            row["euclidean_ms"] = timed(lambda: ops.seg_boundary(m, be.dist, be.ws, d, band=be.band, d=d, metric="euclidean"))
            if m.dtype == torch.int32:
                row["euclidean_peaks_ms"] = timed(lambda: ops.seg_boundary(m, be.dist, be.ws, d, band=be.band, d=d, metric="euclidean",
                                                                          peaks=be.peaks))
                row["peak_rows"] = int((be.peaks != 0).sum())
            d2 = be.dist.view(torch.int16).to(torch.int32) & 0xFFFF
            row["band_pixels"], row["capped_pixels"] = int(((d2 >= 1) & (d2 <= d * d)).sum()), int((d2 == (d + 1) ** 2).sum())
            if m.dtype == torch.uint8 and not args.no_host:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = m.cpu().numpy()
                row["d2h_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                if ndi is not None:
                    t0 = time.perf_counter()
                    values = [v for v in np.unique(host) if v != 0]
                    want = np.zeros((H, W), np.int64)
                    for v in values:
                        mask = np.pad(host[0] == v, 1, constant_values=False)
                        e = ndi.distance_transform_edt(mask)[1:-1, 1:-1]
                        want[host[0] == v] = np.rint(e[host[0] == v] ** 2).astype(np.int64)
                    row.update(values=len(values), host_edt_ms=round((time.perf_counter() - t0) * 1e3, 1))
                    row["host_route_ms"] = round(row["d2h_ms"] + row["host_edt_ms"], 1)
                    assert np.array_equal(np.minimum(want, (d + 1) ** 2), d2.cpu().numpy()[0]), name    # the two routes agree
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.md:
        print("| content | map | objects | band pixels | capped pixels | chessboard, median ms | Euclidean, ms | Euclidean with peaks, ms "
              "| non-zero peak rows | D2H of the map, ms | `distance_transform_edt` per value, values: ms | host route, ms |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['content']} | {r['map']} | {r['objects']} | {r['band_pixels']} | {r['capped_pixels']} | {r['chessboard_ms']} | "
                  f"{r['euclidean_ms']} | {r.get('euclidean_peaks_ms', '—')} | {r.get('peak_rows', '—')} | {r.get('d2h_ms', 'not timed')} | "
                  + (f"{r['values']}: {r['host_edt_ms']} | {r['host_route_ms']} |" if "values" in r else "not timed | not timed |"))


if __name__ == "__main__":
    main()
