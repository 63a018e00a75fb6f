"""Native-size masks and scores: the device stage (ops.seg_native) against the host route on the same box.

4 queries at 512 x 512 -> 480x640, 427x640, 375x500, 640x480 (h x w), uint8 class-id ground truth:
  device: ops.seg_native on a device-resident seg_u8 with the targets staged beforehand (resize, threshold, counts; the
          four launches), timed with device events; and once more including NativeTargets' staging (weights from the
          cache, one H2D copy), timed on the host clock around a synchronize;
  host:   seg_u8 D2H, PIL resize per image, torch threshold and metric per image (the launcher's expressions), 16 threads.
Medians over --reps, the two sides interleaved; one JSON line.

    python scratch/bench_native.py [--reps 30]
    python scratch/bench_native.py --bench-steps 20 [--parent DIR]   # also: bench.py --gpus 1 here (and in a built checkout
                                                                   # of the parent commit), each in a fresh process
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [(480, 640), (427, 640), (375, 500), (640, 480)]


def smooth_masks(b, S, seed):
    """Mask-like uint8 [b, 3, S, S]: blurred blobs, the three channels nearly equal, as a decoded mask is."""
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.interpolate(torch.rand(b, 1, S // 32, S // 32, generator=g), size=(S, S), mode="bicubic")
    x = (x.clamp(0, 1).repeat(1, 3, 1, 1) * 255 + torch.rand(b, 3, S, S, generator=g) * 4).clamp(0, 255)
    return x.to(torch.uint8)


def bench_line(cwd, steps, warmup):
    # the headline step only: the CPU baseline, roofline and secondary configs do not bear on this comparison
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--no-cpu-baseline", "--no-roofline", "--no-secondary"], cwd=cwd, stdout=subprocess.PIPE, text=True, check=True).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=0)
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    if args.bench_steps:        # before this process touches the GPU: each bench.py is a fresh child
        for name, cwd in (("this", ROOT), ("parent", args.parent)):
            if cwd:
                print(json.dumps({"bench": name, **bench_line(cwd, args.bench_steps, 5)}), flush=True)
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    import native_ref as nr
    from diffews_amd import ops
    from diffews_amd.input_pipeline import NativeTargets
    torch.set_num_threads(16)
    S, b = 512, len(SIZES)
    seg = smooth_masks(b, S, 3)
    rs = np.random.RandomState(4)
    gts = [rs.choice([0, 7, 7, 9, 255], size=s, p=[.4, .25, .25, .05, .05]).astype(np.uint8) for s in SIZES]
    segd = seg.cuda()
    t = NativeTargets((S, S), SIZES, gt=gts, class_value=7, ignore_value=255)

    def device_stage():
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = ops.seg_native(segd, t)
        e.record()
        e.synchronize()
        return a.elapsed_time(e), r

    def device_with_staging():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tt = NativeTargets((S, S), SIZES, gt=gts, class_value=7, ignore_value=255)
        r = ops.seg_native(segd, tt)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def host_route():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = nr.native_ref(segd.cpu(), SIZES, gts, 7, 255)
        return (time.perf_counter() - t0) * 1e3, r
    for _ in range(args.warmup):
        device_stage(), device_with_staging(), host_route()
    td, ts, th = [], [], []
    for _ in range(args.reps):
        td.append(device_stage()[0])
        ts.append(device_with_staging()[0])
        th.append(host_route()[0])
    rd, rh = device_stage()[1], host_route()[1]
    same = torch.equal(rd["counts"].cpu(), rh["counts"]) and all(torch.equal(x.cpu(), y) for x, y in zip(rd["pred"], rh["pred"]))
    med = lambda v: round(statistics.median(v), 4)
    out_bytes = sum(4 * h * w for h, w in SIZES)
    print(json.dumps(dict(sizes=SIZES, res=S, reps=args.reps, device_stage_ms=med(td), device_stage_min_ms=round(min(td), 4),
                          device_with_staging_ms=med(ts), host_route_ms=med(th), host_threads=torch.get_num_threads(),
                          equal_to_host=bool(same), out_mb=round(out_bytes / 1e6, 2))), flush=True)


if __name__ == "__main__":
    main()
