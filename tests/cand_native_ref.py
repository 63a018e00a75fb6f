"""CPU reference of candidate classes per query at native size (ops.seg_labels_cand_native): the existing references
composed, none of the package's code.

Per entry e of query q: native_ref.resize_u8 -- Pillow's own `Image.fromarray(hwc).resize((w_q, h_q))` -- and the maximum
of the RESIZED bytes.  Per query: cand_ref.seg_labels_cand's walk (entries ascending, only a strictly larger score takes
over, thr_e = (mx[e] / 255) * r_threshold or the fixed threshold) over the query's entries on the resized bytes, with its
per-pixel counts and area.  Ground truth at native size: a pixel equal to ignore_value (>= 0) is dropped; then
  no table    nway_native_ref.target_map: the id is the label, ids outside 0..nlabels are dropped
  class_ids   nway_native_ref.target_map: 1 + the lowest c with class_ids[c] == id, every other id background
  entry_ids   lab[e] of the earliest entry e OF THE QUERY with entry_ids[e] == id, every other id background
Dropped pixels travel as 255, which cand_ref drops for every nlabels <= 254.
"""
import numpy as np
import torch

import cand_ref
import native_ref as nr
import nway_native_ref as nnr


def resized(seg_u8, off, sizes):
    """uint8 [E_cap, 3, Hs, Ws] -> res[e] uint8 tensor [3, h_q, w_q] for the E = off[-1] real entries, through Pillow."""
    seg_u8 = torch.as_tensor(seg_u8).cpu()
    out = []
    for q, (h, w) in enumerate(sizes):
        out += [nr.resize_u8(seg_u8[e], h, w) for e in range(off[q], off[q + 1])]
    return out


def maxima(res, E_cap):
    """int32 [E_cap]: maximum byte of every resized entry; padding rows stay 0 (what the zeroing launch leaves)."""
    mx = np.zeros(E_cap, np.int32)
    for e, r in enumerate(res):
        mx[e] = int(r.max())
    return mx


def entry_target_map(gt, ids, labs, ignore_value=-1):
    """Integer ground truth [h, w] -> uint8 labels, dropped pixels 255: lab of the EARLIEST entry of the query whose id the
    pixel holds (ids / labs: the query's entries in order), every other id background."""
    g_in = np.asarray(gt).astype(np.int64)
    g = np.zeros(g_in.shape, np.int64)
    for i, l in reversed(list(zip(ids, labs))):       # descending: the earliest entry stays
        g[g_in == int(i)] = int(l)
    if ignore_value >= 0:
        g[g_in == ignore_value] = 255
    return g.astype(np.uint8)


def cand_native_ref(seg_u8, off, lab, nlabels, sizes, gts=None, class_ids=None, entry_ids=None, ignore_value=-1,
                    r_threshold=0.25, threshold=0.0, res=None, mx=None, target=None):
    """seg_u8 uint8 [E_cap, 3, Hs, Ws], off[0..B], lab[e] -> dict(labels=[uint8 [h, w]], counts=int64 [B, 2, nlabels+1] |
    None, area=int64 [E_cap, 2], mx=int32 [E_cap], seg_u8=[uint8 [K_q, 3, h, w]]), all numpy.
    res: resized(...) computed before (shared between calls, never written).  mx: thresholds from THESE maxima instead of
    the resized ones, and target(q, gt) -> uint8 map instead of the rules above: what the discrimination tests vary."""
    assert class_ids is None or entry_ids is None
    seg_u8 = np.asarray(torch.as_tensor(seg_u8).cpu())
    E_cap, B = seg_u8.shape[0], len(off) - 1
    off, lab = [int(x) for x in off], [int(x) for x in lab]
    res = resized(seg_u8, off, sizes) if res is None else res
    mx_res = maxima(res, E_cap)
    mx_thr = mx_res if mx is None else np.asarray(mx)
    labels, planes = [], []
    counts = None if gts is None else np.zeros((B, 2, nlabels + 1), np.int64)
    area = np.zeros((E_cap, 2), np.int64)
    for q, (h, w) in enumerate(sizes):
        lo, hi = off[q], off[q + 1]
        u8 = np.stack([res[e].numpy() for e in range(lo, hi)]) if hi > lo else np.zeros((0, 3, h, w), np.uint8)
        g = None
        if gts is not None:
            if target is not None:
                g = target(q, gts[q])
            elif entry_ids is not None:
                g = entry_target_map(gts[q], [entry_ids[e] for e in range(lo, hi)], lab[lo:hi], ignore_value)
            else:
                g = nnr.target_map(gts[q], nlabels, class_ids, ignore_value).numpy()
            g = g[None]
        l, c, a = cand_ref.seg_labels_cand(u8, mx_thr[lo:hi], [0, hi - lo], lab[lo:hi], nlabels, g, r_threshold, threshold)
        labels.append(l[0])
        planes.append(u8)
        area[lo:hi] = a
        if counts is not None:
            counts[q] = c[0]
    return dict(labels=labels, counts=counts, area=area, mx=mx_res, seg_u8=planes)


# ---------------------------------------------------------------------------------------------- the discriminating input
DISC_SRC = nnr.DISC_SRC                                     # (32, 32)
DISC_SIZES = [(41, 50), (23, 37), (40, 48)]                 # h * w even but w % 4 != 0 | h * w odd | the word path
DISC_LISTS = [(0, 2), (), (0, 1, 3)]                        # [(2, 0), (), (0, 1, 3)] as candidate_tables sorts them
DISC_N, DISC_E, DISC_E_CAP = 4, 5, 8
DISC_OFF = [0, 2, 2, 5]
DISC_CLASS_IDS = [10, 20, 30, 40]                           # the ground-truth id of class c
DISC_IGNORE = 255
_DISC_IMAGE = [0, 0, 1]                                     # which image of nway_native_ref's input a query's entries take


def disc_tables(labels="set"):
    """(lab [E_cap] with padding 0, nlabels, entry_ids [E_cap] with padding repeating the last)."""
    lab, ids = [], []
    for cs in DISC_LISTS:
        for pos, c in enumerate(cs):
            lab.append(1 + (c if labels == "set" else pos))
            ids.append(DISC_CLASS_IDS[c])
    pad = DISC_E_CAP - len(lab)
    return lab + [0] * pad, (DISC_N if labels == "set" else max(len(cs) for cs in DISC_LISTS)), ids + [ids[-1]] * pad


def discriminating_input():
    """uint8 [8, 3, 32, 32], entry-major, from nway_native_ref.discriminating_input(): query 0 holds classes (0, 2) of its
    image 0 -- class 0 is native_ref's overshoot block for 41 x 50, so the resized maximum is not the source's -- query 1
    nothing, query 2 classes (0, 1, 3) of image 1 with class 3 a copy of class 0 (a tie the earlier entry must win).  The
    three padding entries are filled with 255: nothing may look at them."""
    x = nnr.discriminating_input()
    planes = [x[c, _DISC_IMAGE[q]] for q, cs in enumerate(DISC_LISTS) for c in cs]
    pad = torch.full((DISC_E_CAP - len(planes), 3, *DISC_SRC), 255, dtype=torch.uint8)
    return torch.cat([torch.stack(planes), pad])


def disc_gts(kind, dtype=np.uint8):
    """Ground truth at DISC_SIZES.  kind "ids": class-id maps over DISC_CLASS_IDS (every class, so each query sees one that
    is not among its candidates), 0, 77 (no class) and the ignore value; kind "labels": label maps 0..4 with 77 (above
    nlabels) and the ignore value.  int32 maps also hold 1000 (past the 256-entry table) and -3."""
    rng = np.random.default_rng(17)
    base = [0] + (DISC_CLASS_IDS if kind == "ids" else [1, 2, 3, 4]) + [77, DISC_IGNORE]
    if np.dtype(dtype).itemsize == 4:
        base = base + [1000, -3]
    out = []
    for h, w in DISC_SIZES:
        # coarse blocks (objects) with per-pixel noise on top, so every value meets every label
        coarse = rng.integers(0, len(base), size=(-(-h // 6), -(-w // 6)))
        idx = np.kron(coarse, np.ones((6, 6), np.int64))[:h, :w]
        noise = rng.integers(0, len(base), size=(h, w))
        idx = np.where(rng.random((h, w)) < 0.2, noise, idx)
        out.append(np.asarray(base)[idx].astype(dtype))
    return out
