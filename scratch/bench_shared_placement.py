"""Shared-bank attention launch per UNet level (b queries against one s-shot bank), for the A/B of two library builds
(DFW_LIB=<path>, one process per build, alternated by the caller) -- e.g. the workgroup placement of
scratch/fsa_shared_placement.patch.txt against the plain mapping.  Each point: median over --reps groups of 10 launches
(device events), and a bit-compare with the unshared launch on the bank repeated per query."""
import argparse, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffews_amd import ops, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()
assert torch.cuda.is_available(), "this benchmark needs the GPU"
dt = torch.bfloat16
g = torch.Generator(device="cuda").manual_seed(0)
for b, s in ((4, 1), (2, 5)):
    for heads, N in ((5, 4096), (10, 1024), (20, 256)):
        C = heads * 64
        qkv = torch.randn(b, N, 3 * C, generator=g, device="cuda").to(dt)
        kv = torch.randn(s, N, 2 * C, generator=g, device="cuda").to(dt)
        q, k, v, kb, vb = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], kv[..., :C], kv[..., C:]
        f = lambda: ops.fsa_attention(q, k, v, heads, kb, vb, nshot=s, q_prescaled=True, bank_shared=True)
        same = torch.equal(f(), ops.fsa_attention(q, k, v, heads, kb.repeat(b, 1, 1), vb.repeat(b, 1, 1), nshot=s, q_prescaled=True))
        for _ in range(10):
            f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                f()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 100.0)     # us per launch
        ts.sort()
        print(json.dumps(dict(lib=_lib.LIB_PATH, b=b, s=s, heads=heads, N=N, median_us=round(statistics.median(ts), 1),
                              min_us=round(ts[0], 1), max_us=round(ts[-1], 1), equals_repeated_bank=same)), flush=True)
