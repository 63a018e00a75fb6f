"""Matching of predicted to ground-truth objects on the device (ops.seg_match) against what a caller does without it: copy
both int32 id maps to the host and count the (p, g) pairs with np.unique over H * W keys.

One shape, 4096 x 4096 with B = 1, ids from ops.seg_components (8 neighbours, not timed) on the contents of
scratch/bench_components.py: empty, one component over the whole image, random blobs of three classes matched against
themselves, and the same blobs against a perturbed ground truth (shifted by 3 pixels down and 2 right; skip = that map with
2 % of its pixels set to the ignore value 255 -- the objects themselves come from the map without them, so that the ignored
pixels do not become 335 k one-pixel objects).  --cap objects a side (default 8192: the blobs hold about
6700, and 8193^2 keys mean four digit passes), the default max_records / max_pairs of objects.MatchBuffers.

  device: one ops.seg_match call into a resident objects.MatchBuffers, device events around it; and
          objects.matches_to_host on the result, host clock (its two copies);
  host:   D2H of both id maps (and of skip), key = p * (cap + 1) + g with skipped pixels and ids above cap as 0, then
          np.unique(key, return_counts=True) without the key 0, host clock from after a device synchronise.
The pairs of the two routes are compared and must be equal.  Medians over --reps (default 20); the host side is timed
--host-reps times (default 1: one pass sorts 16.8 M keys).  One JSON line per row, and with --md the table of
profiles/object_match_timing.md on stdout.

    python scratch/bench_object_match.py [--reps 20] [--host-reps 1] [--cap 8192] [--md]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--md", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from bench_components import contents
    from diffews_amd import ops
    from diffews_amd.objects import ComponentBuffers, MatchBuffers, matches_to_host
    torch.set_num_threads(16)
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    B, H, W = SHAPE
    cap = args.cap
    pb, gb = ComponentBuffers(B, H, W, cap), ComponentBuffers(B, H, W, cap)
    mb = MatchBuffers(B, H, W, cap, cap, NLAB)
    cases = []
    for name, conn, lab in contents(B, H, W)[:3]:
        cases.append((name, lab, lab, None))
        if name == "random blobs":
            gt = torch.roll(lab, (3, 2), (1, 2)).contiguous()
            skip = gt.clone()
            skip[torch.rand(B, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) < 0.02] = 255
            cases.append(("random blobs, perturbed ground truth, skip", lab, gt, skip))
    rows = []
    for name, lab, gt, skip in cases:
        ops.seg_components(lab, pb.ids, pb.n, pb.ws, stats=pb.stats, connectivity=8)
        ops.seg_components(gt, gb.ids, gb.n, gb.ws, stats=gb.stats, connectivity=8)

        def call():
            ops.seg_match(pb.ids, gb.ids, mb.pairs, mb.pair_off, mb.area, mb.match, mb.gmatch, mb.pq, mb.n, mb.ws,
                          mb.max_records, pstats=pb.stats, gstats=gb.stats, skip=skip)
        m = {k: getattr(mb, k) for k in ("pairs", "pair_off", "area", "match", "gmatch", "pq", "n")}
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
            host, truncated = matches_to_host(m)
            tc.append((time.perf_counter() - t0) * 1e3)
        th, d2h = [], []
        for _ in range(args.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p, g = pb.ids.cpu().numpy().reshape(-1), gb.ids.cpu().numpy().reshape(-1)
            s = None if skip is None else skip.cpu().numpy().reshape(-1)
            d2h.append((time.perf_counter() - t0) * 1e3)
            key = np.where(p <= cap, p, 0).astype(np.int64) * (cap + 1) + np.where(g <= cap, g, 0)
            if s is not None:
                key[s == 255] = 0
            uk, cnt = np.unique(key, return_counts=True)
            uk, cnt = uk[uk > 0], cnt[uk > 0]
            th.append((time.perf_counter() - t0) * 1e3)
        want = np.stack([uk // (cap + 1), uk % (cap + 1), cnt], 1)
        n = host["n"][0].tolist()
        assert not truncated and n[0] == n[1] == len(want), (name, n, len(want))
        assert np.array_equal(host["pairs"][0], want), name                       # the two routes agree on every pair
        pq = host["pq"][0]
        rows.append(dict(content=name, shape=[B, H, W], cap=cap, objects=[int(pb.n[0, 0]), int(gb.n[0, 0])], records=n[2],
                         pairs=n[0], tp_fp_fn=pq[:, :3].sum(0).tolist(), reps=args.reps, device_ms=med(td),
                         matches_to_host_ms=med(tc), d2h_ms=med(d2h), host_route_ms=med(th), host_reps=args.host_reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.md:
        print("| content | objects (pred, gt) | records | pairs | TP, FP, FN | device `seg_match`, median ms | `matches_to_host`, ms | "
              "D2H of the maps, ms | D2H + `np.unique`, ms |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['content']} | {r['objects'][0]}, {r['objects'][1]} | {r['records']} | {r['pairs']} | "
                  f"{r['tp_fp_fn'][0]}, {r['tp_fp_fn'][1]}, {r['tp_fp_fn'][2]} | {r['device_ms']} | {r['matches_to_host_ms']} | "
                  f"{r['d2h_ms']} | {r['host_route_ms']} |")


if __name__ == "__main__":
    main()
