"""Filling the holes of labelled objects on the device (ops.seg_holes) against seg_components on the same map and against
bringing both maps to the host.

One 4096 x 4096 map, B = 1, four contents: empty, one component over the whole image, the random blobs of
bench_components.py punched with pinholes (single pixels and 3 x 3 squares), and one ring object around one large hole.
8 neighbours, no area limit, 1024 stats rows, with a ground truth (counts on).

  components: one ops.seg_components call into a resident objects.ComponentBuffers, device events around it;
  holes:      one ops.seg_holes call on its filtered labels and ids into a resident objects.HoleBuffers, device events;
  host:       D2H of the labels and the ids (84 MB), then -- where scipy is importable -- scipy.ndimage.label of the
              background under the dual connectivity and the rule of the definition in numpy, host clock from after a device
              synchronise; its ids and labels are compared with the device's.  Without scipy the D2H alone.
Medians over --reps (default 20); the host side is bounded by --host-reps.  One JSON line per row, and with --md the table of
profiles/object_holes_timing.md on stdout.

    python scratch/bench_object_holes.py [--reps 20] [--host-reps 3] [--md]
    [DFW_LIB=<library of another build>] python scratch/bench_object_holes.py --components-only [--reps 20]

--components-only times seg_components alone on the four maps: run once per library build, alternated, it is the A/B of
that call across two builds of csrc/seg_components.hip.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W = 1, 4096, 4096
NLAB = 3
CAP = 1024


def contents():
    g = torch.Generator(device="cuda").manual_seed(H)
    field = F.interpolate(torch.rand(B, 2, H // 32, W // 32, device="cuda", generator=g), size=(H, W), mode="bicubic")
    blobs = ((field[:, 0] > 0.55) * (1 + (field[:, 1] * NLAB).clamp(0, NLAB - 1e-3).long())).to(torch.uint8)
    single = torch.rand(B, H, W, device="cuda", generator=g) < 0.002
    seeds = (torch.rand(B, 1, H, W, device="cuda", generator=g) < 0.0005).float()
    square = F.max_pool2d(seeds, 3, 1, 1)[:, 0] > 0
    blobs = torch.where(single | square, torch.zeros_like(blobs), blobs)
    ring = torch.zeros(B, H, W, dtype=torch.uint8, device="cuda")
    ring[:, 64:H - 64, 64:W - 64] = 2
    ring[:, 128:H - 128, 128:W - 128] = 0
    return [("empty", torch.zeros(B, H, W, dtype=torch.uint8, device="cuda")),
            ("one component", torch.ones(B, H, W, dtype=torch.uint8, device="cuda")),
            ("random blobs with pinholes", blobs.contiguous()),
            ("one ring around one hole", ring)]


def host_fill(ndi, lab, ids, conn):
    """The definition on the host: scipy labels the background, numpy applies the rule.  -> (ids_out, labels_out, holes)."""
    structure = ndi.generate_binary_structure(2, 2 if conn == 4 else 1)            # the dual connectivity
    reg, k = ndi.label(lab == 0, structure)
    open_ = np.zeros(k + 1, bool)
    for edge in (reg[0], reg[-1], reg[:, 0], reg[:, -1]):
        open_[edge] = True
    open_[0] = True
    _, first = np.unique(reg.ravel(), return_index=True)                     # the first pixel of region r, r ascending
    first = first[-k:] if k else first[:0]
    first = np.concatenate([[1], first])
    owner = np.where(open_, 0, ids.ravel()[first - 1])
    olab = lab.ravel()[first - 1]
    bad = open_ | (owner < 1)
    hh, ww = lab.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 4 else [])
    for dy, dx in steps:
        a = reg[max(0, -dy):hh - max(0, dy), max(0, -dx):ww - max(0, dx)]
        ni = ids[max(0, dy):hh - max(0, -dy), max(0, dx):ww - max(0, -dx)]
        nl = lab[max(0, dy):hh - max(0, -dy), max(0, dx):ww - max(0, -dx)]
        m = (a > 0) & (nl != 0)
        m[m] = ni[m] != owner[a[m]]
        bad[a[m]] = True
    fill = ~bad
    f = fill[reg]
    return np.where(f, owner[reg], ids).astype(np.int32), np.where(f, olab[reg], lab).astype(np.uint8), (int(fill.sum()), int((~open_).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--md", action="store_true")
    ap.add_argument("--components-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from diffews_amd import ops
    from diffews_amd.objects import ComponentBuffers, HoleBuffers
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    torch.set_num_threads(16)
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    cb = ComponentBuffers(B, H, W, CAP)
    counts = cb.counts(NLAB)
    gt = torch.randint(0, NLAB + 1, (B, H, W), dtype=torch.uint8, device="cuda")
    hb = None if args.components_only else HoleBuffers(B, H, W, CAP)
    rows = []

    def timed(call):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        e.record()
        e.synchronize()
        return a.elapsed_time(e)

    for name, lab in contents():
        def components():
            ops.seg_components(lab, cb.ids, cb.n, cb.ws, filtered=cb.labels, stats=cb.stats, gt=gt, counts=counts, connectivity=8,
                               min_area=0, nlabels=NLAB)

        def holes():
            ops.seg_holes(cb.labels, cb.ids, hb.ids, hb.labels, hb.holes, hb.ws, stats=cb.stats, stats_out=hb.stats, gt=gt,
                          counts=hb.counts(NLAB), connectivity=8, max_area=None, nlabels=NLAB)

        def host():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hl, hi = cb.labels.cpu().numpy(), cb.ids.cpu().numpy()
            t1 = time.perf_counter()
            out = host_fill(ndi, hl[0], hi[0], 8) if ndi is not None else None
            return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3, out
        timed(components)                                                   # warm-up: code objects, first touch of the buffers
        tc = [timed(components) for _ in range(args.reps)]
        row = dict(shape=[B, H, W], content=name, reps=args.reps, objects=int(cb.n[:, 1].sum()), components_ms=med(tc),
                   components_min_ms=round(min(tc), 3), components_max_ms=round(max(tc), 3),
                   lib=os.environ.get("DFW_LIB", "in-tree"))
        if not args.components_only:
            timed(holes)
            th = [timed(holes) for _ in range(args.reps)]
            td, tr, out = [], [], None
            for _ in range(max(1, args.host_reps)):
                d, r, out = host()
                td.append(d)
                tr.append(r)
            filled, enclosed = hb.holes[0].tolist()
            same = None
            if out is not None:
                same = bool(np.array_equal(out[0], hb.ids[0].cpu().numpy()) and np.array_equal(out[1], hb.labels[0].cpu().numpy())
                            and out[2] == (filled, enclosed))
            row.update(holes_ms=med(th), filled=filled, enclosed=enclosed, d2h_ms=med(td), host_reps=len(tr),
                       host_route_ms=med(tr) if ndi is not None else None, scipy=ndi is not None, host_equals_device=same,
                       d2h_mb=round(5 * lab.numel() / 1e6, 1))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.md and not args.components_only:
        print("| content | objects | regions filled / enclosed | seg_components, median ms | seg_holes, median ms | D2H of both maps, median ms "
              "| D2H + scipy label + numpy rule, median ms | host == device |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            host = "no scipy" if r["host_route_ms"] is None else r["host_route_ms"]
            print(f"| {r['content']} | {r['objects']} | {r['filled']} / {r['enclosed']} | {r['components_ms']} | {r['holes_ms']} | "
                  f"{r['d2h_ms']} | {host} | {r['host_equals_device']} |")


if __name__ == "__main__":
    main()
