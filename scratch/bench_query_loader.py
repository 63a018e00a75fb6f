"""Query stream input: the batched input transform (DeviceImageTransform.batch, dfw_inputs_to_tensor) against the two
routes it replaces, and pipeline.segment_stream end to end.

Part 1, per case -- b = 4 and b = 16 queries of 427x640 / 480x640 (h x w) in turn -> 512 x 512, and 100 supports of the
same sizes with their class-id maps (-> +-1 masks) -- three variants, each from decoded uint8 arrays on the host to
finished device tensors, host clock around a synchronize:
  host:     PIL resize + torch ToTensor / Normalize per image (F.interpolate(nearest) per map), stack, one H2D copy;
  per_item: this tree's unchanged per-image route, tf.image() / tf.mask() per item (one pinned buffer, one H2D copy, two
            launches per image, one per map), stack;
  batched:  tf.batch(): one pinned buffer, one H2D copy, three launches.
Warm-up rounds, then --reps rounds with the three variants interleaved; medians.  The three results are compared
(torch.equal) once.

Part 2 (--stream N): images/s of segment_stream over N queries (batch 4) against a 1-shot bank, sd21 widths with synthetic
weights, captured step, against the per-image loop: tf.image() per query, a hand-built NativeTargets per batch,
segment_queries.  Each side runs --stream-reps times, interleaved; medians.

    python scratch/bench_query_loader.py [--reps 20] [--stream 48] [--md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(427, 640), (480, 640)]
S = 512


def decoded(n, seed, masks):
    rs = np.random.RandomState(seed)
    ims = [rs.randint(0, 256, SIZES[i % 2] + (3,)).astype(np.uint8) for i in range(n)]
    mks = [rs.choice([0, 7, 7, 9, 255], size=SIZES[i % 2]).astype(np.uint8) for i in range(n)] if masks else []
    return ims, mks


def host_route(ims, mks, cv):
    from PIL import Image
    out = []
    for im in ims:
        res = np.asarray(Image.fromarray(im, "RGB").resize((S, S), Image.BILINEAR))
        t = torch.from_numpy(res.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        out.append((t - 0.5) / 0.5)
    img = torch.stack(out).pin_memory().cuda(non_blocking=True)
    pm1 = None
    if mks:
        ms = [F.interpolate((torch.from_numpy(m) == cv).float()[None, None], (S, S), mode="nearest")[0] for m in mks]
        pm1 = (torch.stack(ms).repeat(1, 3, 1, 1) * 2 - 1).pin_memory().cuda(non_blocking=True)
    return img, pm1


def per_item_route(tf, ims, mks, cv):
    img = torch.stack([tf.image(im) for im in ims])
    pm1 = torch.stack([tf.mask(m, cv - 1)[0] for m in mks]) if mks else None
    return img, pm1


def batched_route(tf, ims, mks, cv):
    r = tf.batch(ims, mks, cv, want_pm1=True, want_bin=False)
    return r["images"], r["pm1"]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def part1(args):
    from diffews_amd.input_pipeline import DeviceImageTransform
    tf = DeviceImageTransform(S)
    rows = []
    for name, n, masks in (("4 queries", 4, False), ("16 queries", 16, False), ("100 supports + masks", 100, True)):
        ims, mks = decoded(n, n, masks)
        routes = dict(host=lambda: host_route(ims, mks, 7), per_item=lambda: per_item_route(tf, ims, mks, 7),
                      batched=lambda: batched_route(tf, ims, mks, 7))
        for _ in range(args.warmup):
            for fn in routes.values():
                timed(fn)
        ms = {k: [] for k in routes}
        for _ in range(args.reps):
            for k, fn in routes.items():          # interleaved: the three see the same neighbours on the box
                ms[k].append(timed(fn)[0])
        res = {k: fn() for k, fn in routes.items()}
        torch.cuda.synchronize()
        same = all(torch.equal(res["host"][j], res[k][j]) for k in ("per_item", "batched") for j in (0, 1)
                   if res["host"][j] is not None)
        launches = dict(per_item=2 * n + len(mks), batched=2 + (1 if mks else 0))
        rows.append(dict(case=name, reps=args.reps, equal=bool(same), launches=launches,
                         **{f"{k}_ms": round(statistics.median(v), 3) for k, v in ms.items()},
                         **{f"{k}_min_ms": round(min(v), 3) for k, v in ms.items()}))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def part2(args):
    sys.path.insert(0, ROOT)
    import bench
    from diffews_amd.input_pipeline import DeviceImageTransform, NativeTargets
    pipe, _ = bench.build_pipeline(torch.bfloat16)
    tf = DeviceImageTransform(S)
    n, b = args.stream, 4
    ims, gts = decoded(n, 99, True)
    qs = [dict(query_img=im, gt=g) for im, g in zip(ims, gts)]
    sim, smk = decoded(1, 5, True)
    r = tf.batch(sim, smk, 7, want_pm1=True, want_bin=False)
    bank = pipe.prepare_support(r["images"], r["pm1"])

    def stream():
        tot = torch.zeros(4, dtype=torch.int64, device="cuda")
        for index, r in pipe.segment_stream(bank, qs, batch=b, size=S, ignore_value=255, captured=True):
            tot += r["native"]["counts"].sum(0)
        return tot

    def loop():
        tot = torch.zeros(4, dtype=torch.int64, device="cuda")
        for i in range(0, n, b):
            part = qs[i:i + b]
            qry = torch.stack([tf.image(q["query_img"]) for q in part])
            t = NativeTargets((S, S), [q["gt"].shape for q in part], gt=[q["gt"] for q in part], class_value=1, ignore_value=255)
            r = pipe.segment_queries(bank, qry, None, captured=True, native=t)
            tot += r["native"]["counts"].sum(0)
        return tot
    a, b_ = timed(stream)[1], timed(loop)[1]          # warm-up: capture, allocator pools, weight cache
    same = torch.equal(a, b_)
    ts, tl = [], []
    for _ in range(args.stream_reps):
        ts.append(timed(stream)[0])
        tl.append(timed(loop)[0])
    row = dict(queries=n, batch=4, reps=args.stream_reps, equal_counts=bool(same),
               stream_img_s=round(n / (statistics.median(ts) / 1e3), 2), loop_img_s=round(n / (statistics.median(tl) / 1e3), 2),
               stream_ms=round(statistics.median(ts), 2), loop_ms=round(statistics.median(tl), 2))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stream", type=int, default=48, help="queries of the end-to-end part (0: skip it)")
    ap.add_argument("--stream-reps", type=int, default=5)
    ap.add_argument("--md", action="store_true", help="also print the two tables as markdown")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.set_num_threads(16)
    rows = part1(args)
    row = part2(args) if args.stream else None
    if args.md:
        print("| case | host PIL + torch + H2D, ms | per-item calls, ms (launches) | batched call, ms (launches) | equal |")
        print("|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['case']} | {r['host_ms']} | {r['per_item_ms']} ({r['launches']['per_item']}) | "
                  f"{r['batched_ms']} ({r['launches']['batched']}) | {r['equal']} |")
        if row:
            print("\n| queries | segment_stream, images/s | per-image loop, images/s | equal counts |")
            print("|---|---|---|---|")
            print(f"| {row['queries']} | {row['stream_img_s']} | {row['loop_img_s']} | {row['equal_counts']} |")


if __name__ == "__main__":
    main()
