"""Splitting touching objects on the device: the nearest seed inside the object (ops_split.seg_nearest), components of
equal (byte, key) pairs (ops_split.seg_components_keyed) and the composition objects.split_objects, in the manner of
scratch/bench_object_thickness.py.

One shape, 4096 x 4096 with B = 1, on the contents of scratch/bench_components.py: empty, the 4-connected checkerboard,
random blobs of three classes and one component.  Every timed call is warmed three times on the same resident buffers
(cache-warm), timed with device events around the call and a synchronise per repeat, median of --reps.

  seg_nearest         the id map ops.seg_components makes of the labels, seeds = the ids of the cores at RADIUS, for reach
                      8 (split_objects' default at that radius) and 116, passes 1 and 3: the time of one pass is the
                      one-pass call, a later pass (3 passes - 1 pass) / 2
  euclidean           ops.seg_boundary(ids, metric="euclidean") with dmax = the same reach and no band: it walks the same
                      distances, so the ratio of one pass to it is recorded (and not asserted anywhere)
  keyed / keyless     ops_split.seg_components_keyed(labels, keys = nearest) against ops.seg_components(labels), same buffers
  split_objects       objects.split_objects(o, RADIUS) as a whole into resident objects.SplitBuffers, defaults otherwise
--untouched times the calls this stage left alone -- the chessboard and the Euclidean ops.seg_boundary and the keyless
ops.seg_components -- for a comparison of two library builds: one process per build (DFW_LIB=<library>), alternated by the
caller.  One JSON line per row, and with --md the tables of profiles/object_split_timing.md on stdout.

    [DFW_LIB=<library of another build>] python scratch/bench_object_split.py [--reps 20] [--md] [--untouched] [--digits 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPE = (1, 4096, 4096)
CAP = 8192
RADIUS = 3
REACHES = (8, 116)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--md", action="store_true")
    ap.add_argument("--untouched", action="store_true")
    ap.add_argument("--digits", type=int, default=3, help="decimals of the medians, ms")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from bench_components import contents
    from diffews_amd import _lib, metrics
    if args.untouched and os.environ.get("DFW_LIB"):
        _lib.SYMBOLS.pop("dfw_seg_nearest_workspace_bytes", None)   # a build from before it: nothing here asks for it
    from diffews_amd import ops, ops_split
    from diffews_amd.objects import BoundaryBuffers, ComponentBuffers, SplitBuffers, label_objects, object_cores, split_objects
    torch.set_num_threads(16)
    med = lambda v: round(statistics.median(v), args.digits)  # noqa: E731
    B, H, W = SHAPE
    d = metrics.boundary_width(H, W)
    cb = ComponentBuffers(B, H, W, CAP)

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

    if args.untouched:
        chess, eu = BoundaryBuffers(B, H, W, d, torch.int32), BoundaryBuffers(B, H, W, d, torch.int32, metric="euclidean")
        for name, conn, lab in contents(B, H, W):
            comp = lambda: ops.seg_components(lab, cb.ids, cb.n, cb.ws, filtered=cb.labels, stats=cb.stats, connectivity=conn)  # noqa: E731
            row = dict(content=name, reps=args.reps, lib=os.environ.get("DFW_LIB", "in-tree"), components_ms=timed(comp))
            row["chessboard_ms"] = timed(lambda: ops.seg_boundary(cb.ids, chess.dist, chess.ws, d, band=chess.band, d=d))
            row["euclidean_ms"] = timed(lambda: ops.seg_boundary(cb.ids, eu.dist, eu.ws, d, band=eu.band, d=d, metric="euclidean"))
            print(json.dumps(row), flush=True)
        return

    sb = SplitBuffers(B, H, W, CAP)
    eu = BoundaryBuffers(B, H, W, max(REACHES), torch.int32, metric="euclidean")
    rows = []
    for name, conn, lab in contents(B, H, W):
        o = label_objects(lab, connectivity=conn, max_components=CAP, buffers=cb)
        cores = object_cores(o, RADIUS, connectivity=conn, max_components=CAP)
        seeds = cores["ids"]
        row = dict(content=name, shape=[B, H, W], radius=RADIUS, reps=args.reps, objects=int(o["n"][0, 0]), cores=int(cores["n"][0, 0]))
        for R in REACHES:
            one = timed(lambda: ops_split.seg_nearest(o["ids"], seeds, sb.nearest, sb.dist, sb.ws, R, 1))
            row[f"assigned_r{R}_p1"] = int((sb.nearest != 0).sum())
            three = timed(lambda: ops_split.seg_nearest(o["ids"], seeds, sb.nearest, sb.dist, sb.ws, R, 3))
            row[f"assigned_r{R}_p3"] = int((sb.nearest != 0).sum())
            e = timed(lambda: ops.seg_boundary(o["ids"], eu.dist, eu.ws, R, metric="euclidean"))
            row.update({f"nearest_r{R}_p1_ms": one, f"nearest_r{R}_p3_ms": three, f"later_pass_r{R}_ms": round((three - one) / 2, 3),
                        f"euclidean_r{R}_ms": e, f"ratio_r{R}": round(one / e, 2)})
        ops_split.seg_nearest(o["ids"], seeds, sb.nearest, sb.dist, sb.ws, REACHES[0], 3)
        out = sb.out
        row["keyless_ms"] = timed(lambda: ops.seg_components(lab, out.ids, out.n, out.ws, filtered=out.labels, stats=out.stats,
                                                             connectivity=conn))
        row["keyed_ms"] = timed(lambda: ops_split.seg_components_keyed(lab, sb.nearest, out.ids, out.n, out.ws, filtered=out.labels,
                                                                       stats=out.stats, connectivity=conn))
        row["instances"] = int(out.n[0, 0])
        row["split_objects_ms"] = timed(lambda: split_objects(o, RADIUS, buffers=sb, connectivity=conn))
        row["foreground"] = int((lab != 0).sum())
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.md:
        for R in REACHES:
            print(f"\nreach {R}\n")
            print("| content | objects | cores | foreground pixels | assigned, 1 pass | assigned, 3 passes | seg_nearest 1 pass, median ms | "
                  "3 passes, ms | a later pass, ms | Euclidean call, dmax = reach, ms | one pass / Euclidean |")
            print("|---|---|---|---|---|---|---|---|---|---|---|")
            for r in rows:
                print(f"| {r['content']} | {r['objects']} | {r['cores']} | {r['foreground']} | {r[f'assigned_r{R}_p1']} | {r[f'assigned_r{R}_p3']} | "
                      f"{r[f'nearest_r{R}_p1_ms']} | {r[f'nearest_r{R}_p3_ms']} | {r[f'later_pass_r{R}_ms']} | {r[f'euclidean_r{R}_ms']} | {r[f'ratio_r{R}']} |")
        print("\n| content | keyless seg_components, median ms | keyed, ms | instances | split_objects as a whole, ms |")
        print("|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['content']} | {r['keyless_ms']} | {r['keyed_ms']} | {r['instances']} | {r['split_objects_ms']} |")


if __name__ == "__main__":
    main()
