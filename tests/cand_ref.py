"""Numpy reference of label fusion over candidate classes per query (ops.seg_labels_cand / dfw_seg_labels_cand), pixel by
pixel on the host.  It shares no code with diffews_amd.ops or with tests/nway_ref.py.

Input: seg_u8 uint8 [E_cap, 3, H, W], entry-major -- entry e is one (query, candidate class) pair, the entries of a query
are adjacent; mx [E_cap], the maximum byte of every entry; off[0..B], query q owns entries [off[q], off[q+1]); lab[e], the
label byte written where entry e wins (entries from off[B] on are padding and never looked at).
  score_e = ((u0 / 255 + u1 / 255) + u2 / 255) / 3         fp32, one IEEE operation per step
  thr_e   = (mx[e] / 255) * r_threshold   when r_threshold > 0, else the fixed threshold
  label   = 0 with no entry above its threshold, else lab[e] of the one with the largest score; entries in ascending order,
            only a strictly larger score takes over, so the earliest entry wins a tie
  counts  int64 [B, 2, nlabels+1] with gt (0..nlabels; 255 and anything above nlabels dropped): row 0 label == gt == l,
          row 1 pred_l + gt_l - inter_l
  area    int64 [E_cap, 2]: pixels where e is foreground on its own, pixels where e won; every pixel counts, gt or not
"""
import numpy as np

f32 = np.float32


def maxima(seg_u8):
    """int32 [E_cap]: what a gt-less seg_postprocess leaves per entry."""
    seg_u8 = np.asarray(seg_u8)
    return seg_u8.reshape(seg_u8.shape[0], -1).max(axis=1).astype(np.int32)


def score(u0, u1, u2):
    return ((f32(u0) / f32(255.0) + f32(u1) / f32(255.0)) + f32(u2) / f32(255.0)) / f32(3.0)


def seg_labels_cand(seg_u8, mx, off, lab, nlabels, gt=None, r_threshold=0.25, threshold=0.0):
    """(labels uint8 [B, H, W], counts int64 [B, 2, nlabels+1] or None, area int64 [E_cap, 2])."""
    seg_u8 = np.asarray(seg_u8)
    E_cap, _, H, W = seg_u8.shape
    off, lab = [int(x) for x in off], [int(x) for x in lab]
    B = len(off) - 1
    labels = np.zeros((B, H, W), np.uint8)
    counts = None if gt is None else np.zeros((B, 2, nlabels + 1), np.int64)
    area = np.zeros((E_cap, 2), np.int64)
    thr = []
    for e in range(E_cap):
        thr.append(f32(int(mx[e])) / f32(255.0) * f32(r_threshold) if r_threshold > 0 else f32(threshold))
    for q in range(B):
        pred, gth, inter = (np.zeros(nlabels + 1, np.int64) for _ in range(3))
        for y in range(H):
            for x in range(W):
                best, won = f32(-1.0), -1
                for e in range(off[q], off[q + 1]):
                    s = score(seg_u8[e, 0, y, x], seg_u8[e, 1, y, x], seg_u8[e, 2, y, x])
                    if s > thr[e]:
                        area[e, 0] += 1
                        if s > best:
                            best, won = s, e
                l = 0
                if won >= 0:
                    area[won, 1] += 1
                    l = lab[won]
                labels[q, y, x] = l
                if gt is not None:
                    g = int(gt[q, y, x])
                    if g > nlabels:
                        continue
                    pred[l] += 1
                    gth[g] += 1
                    if l == g:
                        inter[l] += 1
        if gt is not None:
            counts[q, 0], counts[q, 1] = inter, pred + gth - inter
    return labels, counts, area
