"""N-way segmentation: segment_classes (one class-major pass over a stack of class banks) against N sequential
segment_queries calls on the same stack's .bank(c).

One process, SD-2.1 UNet + SD VAE, 512 x 512, captured mode: after warm-up the N-way step and the N per-class steps are
replayed alternately, each side timed with device events; the medians, their ratio and prepare_support_classes' own time
are printed as one JSON line per (N, s, b).  The per-class side leaves N binary masks on the device and no label map; the
N-way side includes the label fusion.

    python scratch/bench_nway.py [--reps 24] [--dtype bf16] [--max-batch 16]

The regression check of the existing step (the bank divisor in the attention kernel) is scratch/bench_support_bank.py
--episodes-only, run from a checkout of the parent commit with DFW_LIB=<library of either build>, alternated.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_support_bank import build_pipeline, summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--max-batch", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from diffews_amd import _lib
    from diffews_amd.episodes import make_episode_batch
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    pipe = build_pipeline(dtype)
    pipe.MAX_QUERY_GRAPHS = 8           # the N per-class graphs and the N-way graph live side by side here
    for N, s, b in [(5, 1, 2), (3, 5, 1)]:
        sets = [make_episode_batch(1, s, 512, seed=70 + 10 * c + s, device="cuda") for c in range(N)]
        sup = torch.stack([st["support_imgs"] for st in sets])
        msk = torch.stack([st["support_masks"] for st in sets])
        qb = make_episode_batch(b, 1, 512, seed=80 + b, device="cuda")
        qry = qb["query_img"]
        g = torch.Generator().manual_seed(N)
        labels = torch.randint(0, N + 1, (b, 512, 512), generator=g).to(torch.uint8).cuda()
        binary = [(labels == c + 1).to(torch.uint8) for c in range(N)]
        prep = [timed(lambda: pipe.prepare_support_classes(sup, msk)) for _ in range(args.warmup + 5)][args.warmup:]
        bankset = pipe.prepare_support_classes(sup, msk)
        nway = lambda: pipe.segment_classes(bankset, qry, labels, max_batch=args.max_batch, captured=True)

        def per_class():
            return [pipe.segment_queries(bankset.bank(c), qry, binary[c], captured=True) for c in range(N)]
        for _ in range(args.warmup):
            nway()
            per_class()
        torch.cuda.synchronize()
        tn, tp = [], []
        for _ in range(args.reps):              # the two variants interleaved
            tn.append(timed(nway))
            tp.append(timed(per_class))
        z_n = nway()["z0"].clone()
        z_p = torch.stack([r["z0"].clone() for r in per_class()])
        row = dict(N=N, s=s, b=b, res=512, dtype=args.dtype, lib=_lib.LIB_PATH, reps=args.reps, max_batch=args.max_batch,
                   chunks=-(-N // max(1, args.max_batch // b)))
        row["segment_classes"], row["n_segment_queries"] = summary(tn), summary(tp)
        row["prepare_support_classes_eager"] = summary(prep)
        row["ratio_nway_over_sequential"] = round(row["segment_classes"]["median_ms"] / row["n_segment_queries"]["median_ms"], 4)
        row["z0_rel_l2_nway_vs_sequential"] = float((z_n - z_p).norm() / z_p.norm())
        row["bank_mb"] = round(bankset.nbytes() / 1e6, 1)
        print(json.dumps(row), flush=True)
        pipe._graphs = {}
        del bankset
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
