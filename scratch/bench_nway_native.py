"""N-way labels and counts at native size: the device stage (ops.seg_labels_native) against the host route on the same box.

b = 4 queries at 512 x 512 -> 427x640, 480x640, 427x640, 480x640 (h x w), N in {2, 5, 20} classes, uint8 label ground truth:
  device: ops.seg_labels_native on a device-resident seg_u8 [N, b, 3, S, S] with the targets staged beforehand (the four
          launches plus the allocation of the packed outputs), timed with device events;
  host:   seg_u8 D2H (N * b * 3 * S * S bytes), PIL resize per class and image, the torch label rule and counts per image
          (tests/nway_native_ref.py), 16 threads, host clock.
Medians over --reps, the two sides interleaved; one JSON line per N, and with --md the table of
profiles/nway_native_timing.md on stdout.

    python scratch/bench_nway_native.py [--reps 20] [--md]
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

SIZES = [(427, 640), (480, 640), (427, 640), (480, 640)]
CLASSES = [2, 5, 20]


def smooth_masks(n, S, seed):
    """Mask-like uint8 [n, 3, S, S]: blurred blobs, the three channels nearly equal, as a decoded mask is."""
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.interpolate(torch.rand(n, 1, S // 32, S // 32, generator=g), size=(S, S), mode="bicubic")
    x = (x.clamp(0, 1).repeat(1, 3, 1, 1) * 255 + torch.rand(n, 3, S, S, generator=g) * 4).clamp(0, 255)
    return x.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    import nway_native_ref as nn
    from diffews_amd import ops
    from diffews_amd.input_pipeline import NativeTargets
    torch.set_num_threads(16)
    S, b = 512, len(SIZES)
    rows = []
    for N in CLASSES:
        seg = smooth_masks(N * b, S, 3 + N).view(N, b, 3, S, S)
        rs = np.random.RandomState(4 + N)
        gts = [rs.randint(0, N + 1, size=s).astype(np.uint8) for s in SIZES]
        for g in gts:
            g[rs.rand(*g.shape) < 0.05] = 255
        segd = seg.cuda()
        t = NativeTargets((S, S), SIZES, gt=gts, ignore_value=255)

        def device_stage():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = ops.seg_labels_native(segd, t)
            e.record()
            e.synchronize()
            return a.elapsed_time(e), r

        def host_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = nn.nway_native_ref(segd.cpu(), SIZES, gts, None, 255)
            return (time.perf_counter() - t0) * 1e3, r
        for _ in range(args.warmup):
            device_stage(), host_route()
        td, th = [], []
        for _ in range(args.reps):
            td.append(device_stage()[0])
            th.append(host_route()[0])
        rd, rh = device_stage()[1], host_route()[1]
        same = torch.equal(rd["counts"].cpu(), rh["counts"]) and all(torch.equal(x.cpu(), y) for x, y in zip(rd["labels"], rh["labels"]))
        med = lambda v: round(statistics.median(v), 4)
        row = dict(N=N, b=b, res=S, sizes=SIZES, reps=args.reps, device_stage_ms=med(td), device_stage_min_ms=round(min(td), 4),
                   host_route_ms=med(th), host_threads=torch.get_num_threads(), equal_to_host=bool(same),
                   d2h_mb=round(seg.numel() / 1e6, 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.md:
        print("| N | device stage, median ms (min) | host route, median ms | D2H the host route needs, MB | equal to host |")
        print("|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['N']} | {r['device_stage_ms']} ({r['device_stage_min_ms']}) | {r['host_route_ms']} | {r['d2h_mb']} | "
                  f"{r['equal_to_host']} |")


if __name__ == "__main__":
    main()
