"""Per-window candidate classes in tiled segmentation: the sparse route against the dense one.

Table 1 -- the merge + label stage alone, on random bytes resident on the device, tile 512 x 512, overlap 64 (ramp 64), with
  ground truth: ops.tiles_labels_cand on the listed (window, class) entries [E, 3, 512, 512] against ops.tiles_merge +
  ops.seg_labels on the dense window buffer [N, T, 3, 512, 512] that holds the same entries and zeros elsewhere (equal
  labels / counts / maxima are checked), device events.  Fill = the share of the N * T pairs that is listed, the same
  share in every window; at fill 1.0 both read the same bytes and the sparse kernel is expected to cost more per pair.
Table 2 -- the whole call on the SD-2.1 UNet + SD VAE (bf16, seeded synthetic weights, captured): pipe.segment_tiled with
  `candidates` against the dense pipe.segment_tiled on the same image and library, host clock around a synchronise, and
  the UNet entries each runs.  Both sides decode 8 masks per pass (dense: max_batch 8 = 2 classes x 4 windows; sparse:
  entry_batch 8): 16 at 512 x 512 reach the VAE decoder's 2 GiB buffer-descriptor range.
Medians over --reps, the two sides interleaved; one JSON line per row, and with --md the tables of
profiles/tiled_candidates_timing.md on stdout.

    python scratch/bench_tiled_candidates.py [--reps 5] [--md] [--stage-image 4096] [--stage-n 20]
                                             [--call-image 1536] [--call-n 4] [--fills 0.1,0.25,0.5,1.0] [--no-call]
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

S, OVERLAP, BATCH, ENTRY_BATCH, MAX_BATCH = 512, 64, 4, 8, 8


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


def lists_at(fill, T, N, rs):
    """Every window lists round(fill * N) classes, drawn per window (fill 1.0: all of them)."""
    k = max(0, min(N, int(round(fill * N))))
    return [sorted(rs.choice(N, k, replace=False).tolist()) for _ in range(T)]


def dev_ms(f, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def host_ms(f, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stage_rows(args, fills):
    from diffews_amd import ops
    from diffews_amd.input_pipeline import TilePlan
    L_, N = args.stage_image, args.stage_n
    p = TilePlan((L_, L_), (S, S), OVERLAP)
    rs = np.random.RandomState(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    gt = torch.randint(0, N + 1, (L_, L_), dtype=torch.uint8, device="cuda", generator=g)
    rows = []
    for fill in fills:
        lists = lists_at(fill, p.T, N, rs)
        ct = p.candidate_table(lists, N)
        E = ct["E"]
        ent = torch.randint(0, 256, (max(E, 1), 3, S, S), dtype=torch.uint8, device="cuda", generator=g)
        win = torch.zeros(N, p.T, 3, S, S, dtype=torch.uint8, device="cuda")
        e = 0
        for t, cs in enumerate(lists):
            for c in cs:
                win[c, t] = ent[e]
                e += 1
        tab = ct["tab"].cuda()
        ent_arg = ent[:E] if E else None

        def sparse():
            return ops.tiles_labels_cand(p, ent_arg, tab, ct["tab"], N, gt)

        def dense():
            merged, mx = ops.tiles_merge(p, win)
            lab, cnt = ops.seg_labels(merged.view(N, 1, 3, L_, L_), mx, gt[None])
            return lab[0], cnt[0], mx
        a, b = sparse(), dense()
        equal = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]))
        del a, b
        ts, td = [], []
        for _ in range(args.reps):                       # interleaved
            ts += dev_ms(sparse, 1)
            td += dev_ms(dense, 1)
        rows.append(dict(table="stage", image=L_, N=N, windows=p.T, fill=fill, entries=E, pairs=N * p.T,
                         sparse_ms=statistics.median(ts), dense_ms=statistics.median(td), equal=equal,
                         sparse_bytes_mb=E * 3 * S * S / 1e6, dense_bytes_mb=(N * p.T * 3 * S * S + N * 3 * L_ * L_) / 1e6))
        print(json.dumps(rows[-1]), flush=True)
        del win, ent
    return rows


def call_rows(args, fills):
    from diffews_amd.input_pipeline import TilePlan
    pipe = build_pipe()
    L_, N = args.call_image, args.call_n
    g = torch.Generator().manual_seed(1)
    sups = [(torch.rand(1, 3, S, S, generator=g) * 2 - 1).cuda() for _ in range(N)]
    msks = [torch.where(torch.rand(1, 1, S, S, generator=g) < 0.3, 1.0, -1.0).expand(1, 3, S, S).contiguous().cuda()
            for _ in range(N)]
    library = pipe.prepare_support_classes(sups, msks)
    rs = np.random.RandomState(2)
    img = rs.randint(0, 256, (L_, L_, 3)).astype(np.uint8)
    p = TilePlan((L_, L_), (S, S), OVERLAP)

    def dense():
        return pipe.segment_tiled(library, img, batch=BATCH, max_batch=MAX_BATCH, captured=True)
    dense()                                              # capture
    rows = []
    for fill in fills:
        lists = lists_at(fill, p.T, N, rs)
        E = sum(len(l) for l in lists)

        def sparse():
            return pipe.segment_tiled(library, img, batch=BATCH, captured=True, candidates=lists, entry_batch=ENTRY_BATCH)
        sparse()                                         # capture
        ts, td = [], []
        for _ in range(args.reps):
            ts += host_ms(sparse, 1)
            td += host_ms(dense, 1)
        rows.append(dict(table="call", image=L_, N=N, windows=p.T, fill=fill, entries=E, pairs=N * p.T,
                         sparse_ms=statistics.median(ts), dense_ms=statistics.median(td)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", action="store_true")
    ap.add_argument("--stage-image", type=int, default=4096)
    ap.add_argument("--stage-n", type=int, default=20)
    ap.add_argument("--call-image", type=int, default=1536)
    ap.add_argument("--call-n", type=int, default=4)
    ap.add_argument("--fills", default="0.1,0.25,0.5,1.0")
    ap.add_argument("--no-call", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    fills = [float(v) for v in args.fills.split(",")]
    with torch.no_grad():
        stage = stage_rows(args, fills)
        call = [] if args.no_call else call_rows(args, fills)
    if args.md:
        print("\n| image | N | windows | fill | entries | sparse: labels_cand, median ms | dense: merge + labels, median ms | "
              "sparse reads, MB | dense reads + writes, MB | equal |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for r in stage:
            print(f"| {r['image']}² | {r['N']} | {r['windows']} | {r['fill']:.2f} | {r['entries']} of {r['pairs']} | "
                  f"{r['sparse_ms']:.3f} | {r['dense_ms']:.3f} | {r['sparse_bytes_mb']:.0f} | {r['dense_bytes_mb']:.0f} | "
                  f"{'yes' if r['equal'] else 'NO'} |")
        if call:
            print("\n| image | N | windows | fill | UNet entries, sparse | UNet entries, dense | segment_tiled(candidates=), "
                  "median ms | dense segment_tiled, median ms |")
            print("|---|---|---|---|---|---|---|---|")
            for r in call:
                print(f"| {r['image']}² | {r['N']} | {r['windows']} | {r['fill']:.2f} | {r['entries']} | {r['pairs']} | "
                      f"{r['sparse_ms']:.1f} | {r['dense_ms']:.1f} |")


if __name__ == "__main__":
    main()
