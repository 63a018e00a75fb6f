"""Host time per call of the op wrappers' argument checks: linear, conv3x3, groupnorm, fsa_attention and gemm_tn on device
tensors with the library replaced by a stand-in that does nothing and returns 0, so what is timed is the wrapper's own
Python -- the checks, the argument record, the allocations -- and no kernel.  Two versions of ops.py / ops_bwd.py run in one
process, alternately and twice each (parent, new, parent, new): the package's own, and the pair in --parent DIR (default:
`git show HEAD:diffews_amd/ops.py` and ops_bwd.py, the committed parent of a working tree), each executed into fresh
modules.  It tells the wrappers' host cost apart from everything else if bench.py's eager_ms_per_step moves.

Per op and run: the median over --reps of the mean time of --calls calls, in microseconds.  One JSON line per op, and with
--md the table of profiles/op_args_timing.md.  --host: host tensors and no stream (any machine; the device rule of the new
version is switched off, which takes its last, cheapest check out of the measurement).

    python scratch/bench_op_args.py [--parent DIR] [--reps 7] [--calls 2000] [--md] [--host]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Nothing:
    """The stand-in library: every entry point takes anything and returns 0 (a query: no workspace; a launch: success)."""

    def __getattr__(self, name):
        return lambda *a: 0


def load(source):
    """{"ops", "ops_bwd"} executed from source(name) into fresh modules of the package; ops_bwd imports from this ops."""
    import diffews_amd.ops          # noqa: F401  (the package's own, restored below)
    saved, mods = sys.modules["diffews_amd.ops"], {}
    try:
        for name in ("ops", "ops_bwd"):
            m = types.ModuleType("diffews_amd." + name)
            m.__package__ = "diffews_amd"
            exec(compile(source(name), name + ".py", "exec"), m.__dict__)
            mods[name] = m
            sys.modules["diffews_amd.ops"] = mods["ops"]
    finally:
        sys.modules["diffews_amd.ops"] = saved
    return mods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="directory with the parent's ops.py and ops_bwd.py")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--md", action="store_true")
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    from diffews_amd import _lib as L
    dev = "cpu" if args.host else "cuda"
    assert args.host or torch.cuda.is_available(), "device tensors need the GPU (or pass --host)"

    def parent(name):
        if args.parent:
            return open(os.path.join(args.parent, name + ".py")).read()
        return subprocess.run(["git", "show", f"HEAD:diffews_amd/{name}.py"], cwd=ROOT, check=True, capture_output=True, text=True).stdout

    versions = {"parent": load(parent), "new": load(lambda name: open(os.path.join(ROOT, "diffews_amd", name + ".py")).read())}
    L.lib = _Nothing
    for mods in versions.values():
        for m in mods.values():
            if args.host:
                m._stream = lambda: None
        if args.host and hasattr(mods["ops"], "_Args"):
            mods["ops"]._Args.device = lambda self: None
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)  # noqa: E731
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)  # noqa: E731
    x, w, bias, res = bf(4096, 320), bf(320, 320), f32(320), bf(4096, 320)
    cx, cw = bf(4, 32, 32, 320), bf(320, 9 * 320)
    gamma, beta = f32(320), f32(320)
    qkv, bank, lse = bf(4, 1024, 3 * 320), bf(4, 1024, 2 * 320), f32(4, 5, 1024)
    q, k, v, kb, vb = qkv[..., :320], qkv[..., 320:640], qkv[..., 640:], bank[..., :320], bank[..., 320:]
    out, wgrad = bf(4, 1024, 320), f32(1, 320, 1, 320)
    calls = {
        "linear": lambda m: m["ops"].linear(x, w, bias=bias, residual=res),
        "conv3x3": lambda m: m["ops"].conv3x3(cx, cw, 320, bias=bias, residual=cx),
        "groupnorm": lambda m: m["ops"].groupnorm(cx, gamma, beta, 32, 1e-5, silu=True),
        "fsa_attention": lambda m: m["ops"].fsa_attention(q, k, v, 5, kb, vb, nshot=1, out=out, lse=lse, q_prescaled=True),
        "gemm_tn": lambda m: m["ops_bwd"].gemm_tn(res, x, out=wgrad, accumulate=True),
    }
    rows = []
    for name, call in calls.items():
        runs = []
        for version in ("parent", "new", "parent", "new"):
            mods = versions[version]
            for _ in range(200):
                call(mods)
            per = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    call(mods)
                per.append((time.perf_counter() - t0) / args.calls * 1e6)
            runs.append(round(statistics.median(per), 2))
        p1, n1, p2, n2 = runs
        rows.append(dict(op=name, tensors=dev, parent_us=[p1, p2], new_us=[n1, n2], new_minus_parent_us=round((n1 + n2 - p1 - p2) / 2, 2),
                         parent_spread_us=round(abs(p1 - p2), 2), reps=args.reps, calls=args.calls))
        print(json.dumps(rows[-1]), flush=True)
    if args.md:
        print("| wrapper | parent 1 | parent 2 | new 1 | new 2 | new − parent | parent's spread |")
        print("|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| `{r['op']}` | {r['parent_us'][0]} | {r['parent_us'][1]} | {r['new_us'][0]} | {r['new_us'][1]} | "
                  f"{r['new_minus_parent_us']:+} | {r['parent_spread_us']} |")


if __name__ == "__main__":
    main()
