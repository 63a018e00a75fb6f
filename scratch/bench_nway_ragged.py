"""Ragged class banks: segment_classes on a ragged SupportBankSet against the only equivalent route without it, N
sequential captured segment_queries calls on .bank(c) (N launch trains, N query encodes, N graphs, no labels).

One process, SD-2.1 UNet + SD VAE, 512 x 512, b = 4, captured mode: after warm-up the two routes are replayed alternately,
each replay timed with device events; the medians and their ratio are printed as one JSON line per shot tuple.
--uniform-only: segment_classes on a UNIFORM set (3 classes x 2 shots) alone -- the A/B of two library builds through
DFW_LIB=<path>, one process per build, interleaved by the caller; a library from before the ragged entry points is
accepted (their ctypes bindings are dropped for that process).

    python scratch/bench_nway_ragged.py [--reps 16] [--dtype bf16] [--max-batch 12] [--uniform-only]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_support_bank import build_pipeline, summary, timed  # noqa: E402

SHOTS = [(1, 5, 2), (1, 1, 1, 5, 3)]


def classes(shots, seed):
    from diffews_amd.episodes import make_episode_batch
    sets = [make_episode_batch(1, s, 512, seed=seed + 7 * c, device="cuda") for c, s in enumerate(shots)]
    return [e["support_imgs"] for e in sets], [e["support_masks"] for e in sets]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--uniform-only", action="store_true")
    ap.add_argument("--max-batch", type=int, default=12,
                    help="segment_classes' max_batch: 12 images (3 classes of 4 queries) per UNet / decoder chunk; at 512 x 512 "
                         "the VAE decoder's 16-image batch passes the 2 GiB buffer-descriptor range")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from diffews_amd import _lib
    from diffews_amd.episodes import make_episode_batch
    if args.uniform_only:
        h = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SYMBOLS if "ragged" in n and not hasattr(h, n)]:
            del _lib.SYMBOLS[name]
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    pipe = build_pipeline(dtype)
    b = 4
    qry = make_episode_batch(b, 1, 512, seed=84, device="cuda")["query_img"]
    row = dict(b=b, res=512, dtype=args.dtype, max_batch=args.max_batch, lib=_lib.LIB_PATH, reps=args.reps)
    if args.uniform_only:
        sup, msk = classes((2, 2, 2), seed=90)
        st = pipe.prepare_support_classes(torch.stack(sup), torch.stack(msk))
        run = lambda: pipe.segment_classes(st, qry, max_batch=args.max_batch, captured=True)
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        row.update(shots=[2, 2, 2], segment_classes_uniform=summary([timed(run) for _ in range(args.reps)]))
        print(json.dumps(row), flush=True)
        return
    pipe.MAX_QUERY_GRAPHS = 8          # one graph per class bank of the sequential route, and the set's
    for shots in SHOTS:
        sup, msk = classes(shots, seed=90)
        st = pipe.prepare_support_classes(sup, msk)
        assert st.ragged and st.shots == shots
        banks = [st.bank(c) for c in range(st.nsets)]
        one_pass = lambda: pipe.segment_classes(st, qry, max_batch=args.max_batch, captured=True)

        def sequential():
            for bk in banks:
                pipe.segment_queries(bk, qry, captured=True)
        for _ in range(args.warmup):
            one_pass()
            sequential()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.reps):              # the two routes interleaved
            ta.append(timed(one_pass))
            tb.append(timed(sequential))
        z = one_pass()["z0"].clone()
        err = max(float((z[c] - pipe.segment_queries(bk, qry, captured=True)["z0"]).norm() / z[c].norm())
                  for c, bk in enumerate(banks))
        r = dict(row, shots=list(shots), segment_classes_ragged=summary(ta), sequential_segment_queries=summary(tb))
        r["ratio_ragged_over_sequential"] = round(r["segment_classes_ragged"]["median_ms"]
                                                  / r["sequential_segment_queries"]["median_ms"], 4)
        r["z0_rel_l2_worst_class"] = err
        r["stack_mb"] = round(st.nbytes() / 1e6, 1)
        print(json.dumps(r), flush=True)
        pipe._graphs = {}
        del st, banks
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
