"""Tiled segmentation: what merging on the device saves, and what segment_tiled costs beyond its routed calls.

SD-2.1 UNet + SD VAE, bf16, seeded synthetic weights, tile 512 x 512, overlap 64, batch 4, captured; a 2048 x 2048 image
(5 x 5 windows) and a 4096 x 4096 image (9 x 9), against a 1-shot bank (N = 1) and a 3-class set (N = 3).

Table 1 -- the merge stage, on the windows' seg_u8 [N, T, 3, 512, 512] left on the device by one segment_tiled-style pass:
  device: ops.tiles_merge + ops.seg_labels (with ground truth), device events;
  host:   D2H of all windows' seg_u8, the numpy merge of tests/tiles_ref.py, seg_labels' rule in torch
          (tests/nway_ref.py), 16 threads, host clock around work that begins after a device synchronise.
Table 2 -- the whole call: pipe.segment_tiled (host clock, synchronised) against the bare sum of its routed calls, i.e. the
  same number of segment_queries / segment_classes replays on a resident batch with nothing around them.
Medians over --reps, the two sides of each table interleaved; one JSON line per row, and with --md the tables of
profiles/tiled_timing.md on stdout.  The host route of the 4096 x 4096, N = 3 row moves 191 MB and takes seconds per
repeat: --host-reps bounds it.

    python scratch/bench_tiled.py [--reps 5] [--host-reps 2] [--md]
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

S, OVERLAP, BATCH = 512, 64, 4
IMAGES = [(2048, 2048), (4096, 4096)]


def build_pipe():
    from diffews_amd import config, weights
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise
    from diffews_amd.scheduler import DDIMSchedulerCustomized
    from diffews_amd.unet import MyUNet2DConditionModel
    from diffews_amd.vae import AutoencoderKL
    kw = lambda c: {k: v for k, v in c.items() if not k.startswith("_")}
    dt = torch.bfloat16
    ucfg, vcfg = config.get("sd21_unet"), config.get("sd_vae")
    unet = MyUNet2DConditionModel(ucfg, weights.synthetic_unet_state_dict(ucfg), torch_dtype=dt)
    vae = AutoencoderKL(vcfg, weights.synthetic_vae_state_dict(vcfg), torch_dtype=dt)
    return MarigoldPipelineRGBLatentNoise(unet, vae, DDIMSchedulerCustomized(**kw(config.get("scheduler"))),
                                          text_embeds=weights.synthetic_text_embed(ucfg).cuda())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--md", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    import nway_ref
    import tiles_ref as tr
    from diffews_amd import ops
    from diffews_amd.episodes import make_episode_batch
    torch.set_num_threads(16)
    pipe = build_pipe()
    med = lambda v: round(statistics.median(v), 3)
    supports = []
    st = make_episode_batch(1, 1, S, seed=71, device="cuda")
    supports.append((1, pipe.prepare_support(st["support_imgs"], st["support_masks"])))
    st3 = make_episode_batch(3, 1, S, seed=72, device="cuda")
    supports.append((3, pipe.prepare_support_classes(st3["support_imgs"].view(3, 1, 3, S, S),
                                                     st3["support_masks"].view(3, 1, 3, S, S))))
    rows = []
    for hw in IMAGES:
        rs = np.random.RandomState(hw[0])
        img = rs.randint(0, 256, hw + (3,)).astype(np.uint8)
        for N, support in supports:
            gt = rs.randint(0, N + 1, hw).astype(np.uint8)
            nway = N > 1
            call = lambda: pipe.segment_tiled(support, img, gt, overlap=OVERLAP, batch=BATCH, captured=True)
            r = call()                                                     # warm-up: capture, allocator pools
            plan = r["plan"]
            T, nb = plan.T, -(-plan.T // BATCH)
            q = torch.rand(BATCH, 3, S, S, device="cuda") * 2 - 1
            routed = (lambda: pipe.segment_classes(support, q, captured=True)) if nway else \
                     (lambda: pipe.segment_queries(support, q, captured=True))
            routed()
            # the windows' seg_u8 as the call leaves them, for table 1 (values do not matter to the time; mask-like bytes)
            win = (torch.rand(N, T, 3, S, S, device="cuda") * 255).to(torch.uint8)
            gtd = torch.from_numpy(gt).cuda()[None]

            def device_stage():
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                seg, mx = ops.tiles_merge(plan, win)
                lab, cnt = ops.seg_labels(seg.view(N, 1, 3, *hw), mx, gtd)
                e.record()
                e.synchronize()
                return a.elapsed_time(e), (seg, lab, cnt)

            def host_route():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                seg, _ = tr.merge(win.cpu().numpy(), hw, plan.ys, plan.xs, plan.ramp)
                lab, cnt = nway_ref.seg_labels(torch.from_numpy(seg)[:, None], torch.from_numpy(gt)[None])
                return (time.perf_counter() - t0) * 1e3, (seg, lab, cnt)

            def whole():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            def bare():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(nb):
                    routed()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            device_stage()
            td, th, tw, tb, h = [], [], [], [], None
            for i in range(args.reps):
                td.append(device_stage()[0])
                if i < max(1, args.host_reps):
                    ms, h = host_route()
                    th.append(ms)
                tw.append(whole())
                tb.append(bare())
            d = device_stage()[1]
            same = bool(np.array_equal(d[0].cpu().numpy(), h[0]) and torch.equal(d[1].cpu(), h[1]) and torch.equal(d[2].cpu(), h[2]))
            row = dict(image=list(hw), N=N, windows=T, batches=nb, reps=args.reps, host_reps=len(th),
                       device_merge_labels_ms=med(td), host_route_ms=med(th), d2h_mb=round(win.numel() / 1e6, 1),
                       equal_to_host=same, segment_tiled_ms=med(tw), routed_calls_ms=med(tb),
                       around_the_calls_ms=round(med(tw) - med(tb), 3), window_buffer_mb=round(plan.window_bytes(N) / 1e6, 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del win
    if args.md:
        print("| image | N | windows | device merge + labels, median ms | host route, median ms | D2H the host route needs, MB | equal to host |")
        print("|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['image'][0]}×{r['image'][1]} | {r['N']} | {r['windows']} | {r['device_merge_labels_ms']} | "
                  f"{r['host_route_ms']} | {r['d2h_mb']} | {r['equal_to_host']} |")
        print()
        print("| image | N | batches of 4 | segment_tiled, median ms | its routed calls alone, median ms | around the calls, ms |")
        print("|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['image'][0]}×{r['image'][1]} | {r['N']} | {r['batches']} | {r['segment_tiled_ms']} | "
                  f"{r['routed_calls_ms']} | {r['around_the_calls_ms']} |")


if __name__ == "__main__":
    main()
