"""Shared support bank: segment_queries (bank prepared once) against run_episodes (supports replicated per query).

One process, SD-2.1 UNet + SD VAE, 512 x 512, captured mode: after warm-up the two captured steps are replayed
alternately, each replay timed with device events; the medians, their ratio and prepare_support's own time are printed as
one JSON line per (b, s).  --episodes-only: run_episodes at configs[1] alone (the A/B of two library builds through
DFW_LIB=<path>, one process per build, interleaved by the caller).

    python scratch/bench_support_bank.py [--reps 24] [--dtype bf16] [--episodes-only]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_pipeline(dtype):
    from diffews_amd import config, weights
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise
    from diffews_amd.scheduler import DDIMSchedulerCustomized
    from diffews_amd.unet import MyUNet2DConditionModel
    from diffews_amd.vae import AutoencoderKL
    ucfg, vcfg = config.get("sd21_unet"), config.get("sd_vae")
    usd = weights.synthetic_unet_state_dict(ucfg, round_to=torch.float16)
    vsd = weights.synthetic_vae_state_dict(vcfg, round_to=torch.float16)
    te = weights.synthetic_text_embed(ucfg).to(torch.float16).float()
    sched = DDIMSchedulerCustomized(**{k: v for k, v in config.get("scheduler").items() if not k.startswith("_")})
    return MarigoldPipelineRGBLatentNoise(MyUNet2DConditionModel(ucfg, usd, torch_dtype=dtype),
                                          AutoencoderKL(vcfg, vsd, torch_dtype=dtype), sched, text_embeds=te.cuda())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(ts):
    ts = sorted(ts)
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(ts[0], 3), max_ms=round(ts[-1], 3), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--episodes-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from diffews_amd import _lib
    from diffews_amd.episodes import make_episode_batch
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    pipe = build_pipeline(dtype)
    shapes = [(4, 1)] if args.episodes_only else [(4, 1), (2, 5)]
    for b, s in shapes:
        st = make_episode_batch(1, s, 512, seed=70 + s, device="cuda")
        qb = make_episode_batch(b, 1, 512, seed=80 + b, device="cuda")
        sup, msk, qry, gt = st["support_imgs"], st["support_masks"], qb["query_img"], qb["query_mask"]
        rep = lambda t: t.repeat(b, 1, 1, 1).contiguous()
        sup_r, msk_r = rep(sup), rep(msk)
        episodes = lambda: pipe.run_episodes(sup_r, qry, msk_r, gt, captured=True)
        row = dict(b=b, s=s, res=512, dtype=args.dtype, lib=_lib.LIB_PATH, reps=args.reps)
        if args.episodes_only:
            for _ in range(args.warmup):
                episodes()
            torch.cuda.synchronize()
            row["run_episodes"] = summary([timed(episodes) for _ in range(args.reps)])
            print(json.dumps(row), flush=True)
            continue
        prep = [timed(lambda: pipe.prepare_support(sup, msk)) for _ in range(args.warmup + 5)][args.warmup:]
        bank = pipe.prepare_support(sup, msk)
        queries = lambda: pipe.segment_queries(bank, qry, gt, captured=True)
        for _ in range(args.warmup):
            episodes()
            queries()
        torch.cuda.synchronize()
        te, tq = [], []
        for _ in range(args.reps):              # the two variants interleaved
            te.append(timed(episodes))
            tq.append(timed(queries))
        z_e, z_q = episodes()["z0"].clone(), queries()["z0"].clone()
        row["run_episodes"], row["segment_queries"] = summary(te), summary(tq)
        row["prepare_support_eager"] = summary(prep)
        row["ratio_queries_over_episodes"] = round(row["segment_queries"]["median_ms"] / row["run_episodes"]["median_ms"], 4)
        row["z0_rel_l2_queries_vs_episodes"] = float((z_q - z_e).norm() / z_e.norm())
        row["bank_mb"] = round(bank.nbytes() / 1e6, 1)
        print(json.dumps(row), flush=True)
        pipe._graphs = {}
        del bank
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
