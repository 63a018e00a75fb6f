"""Routed queries: segment_routed on a ragged SupportBankSet, the route changing with every replay, against the two routes
that existed before it -- (a) b sequential captured segment_queries calls of batch 1 on .bank(route[i]) (one graph per
class, b launch trains) and (b) segment_classes over all N classes (N times the UNet and decoder work per query).

One process, SD-2.1 UNet + SD VAE, 512 x 512, b = 4, library shots (1, 5, 2, 1, 3), captured mode: after warm-up the three
routes are replayed alternately, each replay timed with device events and each with the next route of a fixed cycle; the
medians and their ratios are printed as one JSON line.
--uniform-only: segment_classes on a UNIFORM set (3 classes x 2 shots) alone -- the A/B of two library builds through
DFW_LIB=<path>, one process per build, interleaved by the caller; a library from before the routed entry points is
accepted (their ctypes bindings are dropped for that process).

    python scratch/bench_routed.py [--reps 24] [--dtype bf16] [--max-batch 12] [--uniform-only]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_nway_ragged import classes  # noqa: E402
from bench_support_bank import build_pipeline, summary, timed  # noqa: E402

SHOTS = (1, 5, 2, 1, 3)
ROUTES = [(2, 0, 4, 1), (1, 1, 3, 0), (4, 2, 2, 1), (0, 3, 1, 4), (3, 4, 0, 2), (1, 0, 1, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--uniform-only", action="store_true")
    ap.add_argument("--max-batch", type=int, default=12, help="segment_classes' max_batch (see bench_nway_ragged.py)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from diffews_amd import _lib
    from diffews_amd.episodes import make_episode_batch
    if args.uniform_only:
        h = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SYMBOLS if "routed" in n and not hasattr(h, n)]:
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
    pipe.MAX_QUERY_GRAPHS = 8          # one graph per class bank of the sequential route, the routed one and the set's
    sup, msk = classes(SHOTS, seed=90)
    st = pipe.prepare_support_classes(sup, msk)
    assert st.ragged and st.shots == SHOTS
    ones = [qry[i:i + 1].contiguous() for i in range(b)]
    step = [0]

    def next_route():
        step[0] += 1
        return ROUTES[step[0] % len(ROUTES)]

    routed = lambda: pipe.segment_routed(st, qry, next_route(), captured=True)

    def sequential():
        for i, c in enumerate(next_route()):
            pipe.segment_queries(st.bank(c), ones[i], captured=True)

    all_classes = lambda: pipe.segment_classes(st, qry, max_batch=args.max_batch, captured=True)
    for c in range(st.nsets):          # every class bank's batch-1 graph exists before anything is timed
        pipe.segment_queries(st.bank(c), ones[0], captured=True)
    for _ in range(args.warmup):
        routed()
        sequential()
        all_classes()
    torch.cuda.synchronize()
    graphs = len(pipe._graphs)
    ta, tb, tc = [], [], []
    for _ in range(args.reps):              # the three routes interleaved
        ta.append(timed(routed))
        tb.append(timed(sequential))
        tc.append(timed(all_classes))
    assert len(pipe._graphs) == graphs       # nothing was captured or dropped while timing
    route = ROUTES[0]
    z = pipe.segment_routed(st, qry, route, captured=True)["z0"].clone()
    err = max(float((z[i:i + 1] - pipe.segment_queries(st.bank(c), ones[i], captured=True)["z0"]).norm() / z[i:i + 1].norm())
              for i, c in enumerate(route))
    r = dict(row, shots=list(SHOTS), routes=len(ROUTES), graphs=graphs, segment_routed=summary(ta),
             sequential_segment_queries_b1=summary(tb), segment_classes_all=summary(tc))
    r["ratio_routed_over_sequential"] = round(r["segment_routed"]["median_ms"] / r["sequential_segment_queries_b1"]["median_ms"], 4)
    r["ratio_routed_over_all_classes"] = round(r["segment_routed"]["median_ms"] / r["segment_classes_all"]["median_ms"], 4)
    r["z0_rel_l2_worst_entry"] = err
    r["stack_mb"] = round(st.nbytes() / 1e6, 1)
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
