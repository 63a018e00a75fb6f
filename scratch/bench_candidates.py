"""Candidate classes per query: a captured segment_candidates on a library of N = 8 classes, b = 4 queries with
k = (3, 1, 2, 2) candidates each (E = 8 entries, one pass of entry_batch 8), the candidates changing with every replay,
against the two routes a caller had before it --
  (a) segment_classes over all 8 classes (N x b UNet and decoder entries for E that are wanted);
  (b) sum(k) captured segment_routed calls of batch 1 (the query's VAE encode repeated per candidate, one launch train
      per entry) plus b ops.seg_labels launches that fuse each query's masks (class-major [k_i, 1, 3, H, W]).

One process, SD-2.1 UNet + SD VAE, 512 x 512, captured mode: after warm-up the three routes are replayed alternately, each
replay timed with device events; the medians and their ratios are printed as one JSON line.

    python scratch/bench_candidates.py [--reps 24] [--dtype bf16] [--max-batch 12] [--entry-batch 8]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_nway_ragged import classes  # noqa: E402
from bench_support_bank import build_pipeline, summary, timed  # noqa: E402

SHOTS = (1, 5, 2, 1, 3, 1, 2, 1)
CANDIDATES = [((2, 0, 7), (1,), (4, 3), (5, 6)), ((1, 3, 5), (0,), (7, 2), (4, 6)), ((6, 4, 0), (7,), (1, 2), (3, 5)),
              ((0, 1, 2), (3,), (4, 5), (6, 7))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--max-batch", type=int, default=12, help="segment_classes' max_batch (see bench_nway_ragged.py)")
    ap.add_argument("--entry-batch", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from diffews_amd import _lib, ops
    from diffews_amd.episodes import make_episode_batch
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    pipe = build_pipeline(dtype)
    pipe.MAX_QUERY_GRAPHS = 8
    b = 4
    qry = make_episode_batch(b, 1, 512, seed=84, device="cuda")["query_img"]
    sup, msk = classes(SHOTS, seed=90)
    st = pipe.prepare_support_classes(sup, msk)
    assert st.ragged and st.shots == SHOTS
    ones = [qry[i:i + 1].contiguous() for i in range(b)]
    step = [0]

    def next_candidates():
        step[0] += 1
        return CANDIDATES[step[0] % len(CANDIDATES)]

    cand = lambda: pipe.segment_candidates(st, qry, next_candidates(), entry_batch=args.entry_batch, captured=True)
    all_classes = lambda: pipe.segment_classes(st, qry, max_batch=args.max_batch, captured=True)

    def per_candidate():
        for i, cs in enumerate(next_candidates()):
            u8, mx = [], []
            for c in sorted(cs):
                r = pipe.segment_routed(st, ones[i], [c], captured=True)
                u8.append(r["seg_u8"].clone())              # the next replay overwrites the graph's output
                mx.append(u8[-1].amax().to(torch.int32).view(1))
            ops.seg_labels(torch.stack(u8), torch.cat(mx))

    for _ in range(args.warmup):
        cand()
        all_classes()
        per_candidate()
    torch.cuda.synchronize()
    graphs = len(pipe._graphs)
    tc, ta, tb = [], [], []
    for _ in range(args.reps):              # the three routes interleaved
        tc.append(timed(cand))
        ta.append(timed(all_classes))
        tb.append(timed(per_candidate))
    assert len(pipe._graphs) == graphs       # nothing was captured or dropped while timing
    r = dict(b=b, res=512, dtype=args.dtype, nsets=len(SHOTS), shots=list(SHOTS), k=[len(c) for c in CANDIDATES[0]],
             entry_batch=args.entry_batch, max_batch=args.max_batch, lib=_lib.LIB_PATH, reps=args.reps, graphs=graphs,
             segment_candidates=summary(tc), segment_classes_all=summary(ta), routed_b1_plus_seg_labels=summary(tb))
    r["ratio_candidates_over_all_classes"] = round(r["segment_candidates"]["median_ms"] / r["segment_classes_all"]["median_ms"], 4)
    r["ratio_candidates_over_per_candidate"] = round(r["segment_candidates"]["median_ms"]
                                                     / r["routed_b1_plus_seg_labels"]["median_ms"], 4)
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
