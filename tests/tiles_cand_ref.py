"""Host reference of per-window candidate classes in tiled segmentation (ops.tiles_labels_cand, pipe.segment_tiled with
`candidates`), stated through the two references the dense route already has: a (window, class) pair that is not listed is
an all-zero mask, so the entries are SCATTERED into a zero [N, T, 3, th, tw] array, tests/tiles_ref.py merges it and
tests/nway_ref.py labels the merged bytes.  The kernel gathers per pixel over an LDS table of the cell's windows and never
builds either array: the two share no indexing.  `area` is counted in numpy from the merged bytes.
"""
import numpy as np
import torch

import nway_ref
import tiles_ref as tr


def dense(ent, tab, N, T):
    """ent uint8 [E_cap, 3, th, tw], tab int [T + 1 + E_cap] (offsets, then classes) -> uint8 [N, T, 3, th, tw]."""
    ent, tab = np.asarray(ent), [int(v) for v in np.asarray(tab)]
    off, cls = tab[:T + 1], tab[T + 1:]
    win = np.zeros((N, T) + ent.shape[1:], np.uint8)
    for t in range(T):
        for e in range(off[t], off[t + 1]):
            win[cls[e], t] = ent[e]
    return win


def labels_cand(ent, tab, N, img_hw, ys, xs, ramp, gt=None, r_threshold=0.25, threshold=0.0, tile=None):
    """-> (labels uint8 [h, w], counts int64 [2, N+1] or None, mx int64 [N], area int64 [N, 2]), all torch / numpy on the
    host.  ent may be None (no entry anywhere) when `tile` is given."""
    T = len(ys) * len(xs)
    if ent is None:
        ent = np.zeros((1, 3) + tuple(tile), np.uint8)
    merged, mx = tr.merge(dense(ent, tab, N, T), img_hw, ys, xs, ramp)
    seg = torch.from_numpy(merged)[:, None]                                   # [N, 1, 3, h, w]
    gt_t = None if gt is None else torch.as_tensor(np.asarray(gt))[None]
    lab, cnt = nway_ref.seg_labels(seg, gt_t, r_threshold, threshold, False)
    fg = nway_ref.foreground(seg, r_threshold, threshold, False)[:, 0].numpy()
    won = lab[0].numpy()
    area = np.array([[int(fg[c].sum()), int((won == c + 1).sum())] for c in range(N)], np.int64).reshape(N, 2)
    return lab[0], (None if cnt is None else cnt[0]), torch.from_numpy(np.asarray(mx, np.int64)), torch.from_numpy(area)
