"""Numpy reference of the score stage (dfw_seg_scores): the plane sum gathered through the plane table, np.bincount with
int64 weights for sum and count, np.minimum.at / np.maximum.at for the extremes.  brute_scores is an independent per-pixel
loop for tiny maps, and loop_ap a plain-loop average precision (sort, walk, interpolate) that shares nothing with
metrics.average_precision."""
import math

import numpy as np


def scores_image(ids, labels, seg_u8, table_row, cap):
    """ids int [H, W], labels uint8 [H, W], seg_u8 uint8 [P, 3, H, W], table_row int [nlabels + 1] -> int64 [cap, 4]."""
    ids, labels = np.asarray(ids).astype(np.int64).reshape(-1), np.asarray(labels).astype(np.int64).reshape(-1)
    u = np.asarray(seg_u8)
    P = u.shape[0]
    s = u.astype(np.int64).sum(1).reshape(P, -1)                        # [P, HW]
    row = np.asarray(table_row).astype(np.int64)
    nlabels = len(row) - 1
    lab_ok = (labels >= 1) & (labels <= nlabels)
    g = np.where(lab_ok, row[np.clip(labels, 0, nlabels)], -1)
    ok = (ids >= 1) & (ids <= cap) & lab_ok & (g >= 0) & (g < P)
    q = np.flatnonzero(ok)
    v, k = s[g[q], q], ids[q] - 1
    out = np.zeros((cap, 4), np.int64)
    out[:, 0] = np.bincount(k, weights=v, minlength=cap).astype(np.int64)      # exact: far below 2^53
    out[:, 1] = np.bincount(k, minlength=cap)
    lo, hi = np.full(cap, 766, np.int64), np.full(cap, -1, np.int64)
    np.minimum.at(lo, k, v)
    np.maximum.at(hi, k, v)
    out[:, 2] = np.where(out[:, 1] > 0, lo, 0)
    out[:, 3] = np.where(out[:, 1] > 0, hi, 0)
    return out


def scores(ids, labels, seg_u8, table, cap):
    """[B, H, W] maps, table [B, nlabels + 1] -> int64 [B, cap, 4]."""
    return np.stack([scores_image(ids[b], labels[b], seg_u8, table[b], cap) for b in range(len(ids))])


def brute_scores(ids, labels, seg_u8, table_row, cap):
    """The same table pixel by pixel, on nested lists."""
    H, W, P, nlabels = len(ids), len(ids[0]), len(seg_u8), len(table_row) - 1
    out = [[0, 0, 0, 0] for _ in range(cap)]
    for y in range(H):
        for x in range(W):
            k, l = ids[y][x], labels[y][x]
            if not 1 <= k <= cap or not 1 <= l <= nlabels:
                continue
            g = table_row[l]
            if not 0 <= g < P:
                continue
            s = seg_u8[g][0][y][x] + seg_u8[g][1][y][x] + seg_u8[g][2][y][x]
            r = out[k - 1]
            r[2] = s if r[1] == 0 else min(r[2], s)
            r[3] = s if r[1] == 0 else max(r[3], s)
            r[0] += s
            r[1] += 1
    return out


def mean(total, n):
    return total / (765 * n) if n else 0.0


def loop_ap(dets, npos, thresholds):
    """dets: a list of rows (class, sum, n, inter, union) in dataset order; npos: a list per class.  -> a list per class of
    lists per threshold, None for a class without positives."""
    out = []
    for c in range(len(npos)):
        if c == 0 or npos[c] <= 0:
            out.append(None)
            continue
        mine = [(d[1] / d[2], i, d) for i, d in enumerate(dets) if d[0] == c]
        mine.sort(key=lambda t: (-t[0], t[1]))                          # the score down, the dataset order within a tie
        per = []
        for num, den in thresholds:
            tp, recall, prec = 0, [], []
            for rank, (_, _, d) in enumerate(mine, 1):
                if d[4] > 0 and d[3] * den > num * d[4]:
                    tp += 1
                recall.append(tp / npos[c])
                prec.append(tp / rank)
            for i in range(len(prec) - 2, -1, -1):
                prec[i] = max(prec[i], prec[i + 1])
            q = []
            for k in range(101):
                at = 0
                while at < len(recall) and recall[at] < k / 100:
                    at += 1
                q.append(prec[at] if at < len(recall) else 0.0)
            per.append(math.fsum(q) / 101)
        out.append(per)
    return out


def loop_map(ap):
    vals = [v for per in ap if per is not None for v in per]
    return math.fsum(vals) / len(vals) if vals else float("nan")
