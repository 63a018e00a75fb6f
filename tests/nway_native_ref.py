"""CPU reference of N-way labels and counts at native size (ops.seg_labels_native): the two existing references composed.

Per (class, image): native_ref.resize_u8 -- Pillow's own `Image.fromarray(hwc).resize((w, h))` -- and the maximum of the
RESIZED bytes.  Per image: nway_ref.scores on the resized bytes of its N classes, thr_c = (m / 255) * r_threshold with
m = the resized maximum of (class, image), or of the class over the batch under batch_max, else the fixed threshold, and
nway_ref's walk (classes ascending, only a strictly larger score takes over).  Ground truth at native size: a pixel equal to
ignore_value (>= 0) is dropped; without class_ids the id is the label and ids outside 0..N are dropped; with class_ids the
label is 1 + the lowest c with class_ids[c] == id, every other id background.  Counts are nway_ref.counts' (dropped pixels
travel as 255, which it drops for every N <= 254).
"""
import numpy as np
import torch

import native_ref as nr
import nway_ref

F32 = torch.float32


def resized(seg_u8, sizes):
    """uint8 [N, B, 3, Hs, Ws] -> res[c][i] uint8 [3, h_i, w_i], through Pillow."""
    seg_u8 = seg_u8.cpu()
    return [[nr.resize_u8(seg_u8[c, i], h, w) for i, (h, w) in enumerate(sizes)] for c in range(seg_u8.shape[0])]


def maxima(res):
    """int32 [N, B]: maximum byte of every resized (class, image)."""
    return torch.tensor([[int(r.max()) for r in row] for row in res], dtype=torch.int32)


def thresholds(mx, r_threshold=0.25, threshold=0.0, batch_max=False):
    """fp32 [N, B] from the maxima int32 [N, B]: nway_ref.thresholds' expressions."""
    if not r_threshold > 0:
        return torch.full(tuple(mx.shape), float(threshold), dtype=F32)
    m = mx.amax(1, keepdim=True).expand_as(mx) if batch_max else mx
    return (m.to(F32) / torch.tensor(255.0, dtype=F32)) * torch.tensor(float(r_threshold), dtype=F32)


def walk(sc, thr):
    """sc fp32 [N, h, w], thr fp32 [N] -> uint8 [h, w]: nway_ref.labels' loop for one image."""
    best = torch.full(sc.shape[1:], -1.0, dtype=F32)
    lab = torch.zeros(sc.shape[1:], dtype=torch.uint8)
    for c in range(sc.shape[0]):                      # ascending, strictly larger takes over: lowest c wins a tie
        take = (sc[c] > thr[c]) & (sc[c] > best)
        best = torch.where(take, sc[c], best)
        lab = torch.where(take, torch.full_like(lab, c + 1), lab)
    return lab


def labels_of(planes, thr):
    """planes: N uint8 [3, h, w] tensors of one image, thr fp32 [N] -> uint8 [h, w]."""
    return walk(nway_ref.scores(torch.stack(planes)[:, None])[:, 0], thr)


def target_map(gt, N, class_ids=None, ignore_value=-1):
    """Integer ground truth [h, w] -> uint8 [h, w] of labels 0..N, dropped pixels 255."""
    ids = torch.as_tensor(np.asarray(gt).astype(np.int64))
    drop = (ids == ignore_value) if ignore_value >= 0 else torch.zeros_like(ids, dtype=torch.bool)
    if class_ids is None:
        drop = drop | (ids < 0) | (ids > N)
        g = ids.clone()
    else:
        g = torch.zeros_like(ids)
        for c in reversed(range(N)):                  # descending: the lowest c with class_ids[c] == id stays
            g[ids == int(class_ids[c])] = c + 1
    g[drop] = 255
    return g.to(torch.uint8)


def nway_native_ref(seg_u8, sizes, gts=None, class_ids=None, ignore_value=-1, r_threshold=0.25, threshold=0.0,
                    batch_max=False, res=None):
    """seg_u8 uint8 [N, B, 3, Hs, Ws] -> dict(labels=[uint8 [h, w]], counts=int64 [B, 2, N+1] | None, mx=int32 [N, B],
    seg_u8=[uint8 [N, 3, h, w]]).  res: resized(seg_u8, sizes) computed before (shared between calls, never written)."""
    N, B = seg_u8.shape[:2]
    res = resized(seg_u8, sizes) if res is None else res
    mx = maxima(res)
    thr = thresholds(mx, r_threshold, threshold, batch_max)
    labels = [labels_of([res[c][i] for c in range(N)], thr[:, i]) for i in range(B)]
    counts = None
    if gts is not None:
        counts = torch.cat([nway_ref.counts(labels[i][None], target_map(gts[i], N, class_ids, ignore_value)[None], N)
                            for i in range(B)])
    return dict(labels=labels, counts=counts, mx=mx, seg_u8=[torch.stack([res[c][i] for c in range(N)]) for i in range(B)])


DISC_SRC, DISC_SIZES = (32, 32), [(41, 50), (23, 37)]


def discriminating_input():
    """uint8 [4, 2, 3, 32, 32] for DISC_SIZES: blocks whose bicubic resize overshoots (so the resized maxima differ from the
    source's), ramps with unequal channels, and class 3 a copy of class 0 (a tie the lowest class must win).
    test_nway_native_cpu.test_discriminating_input_discriminates pins what it separates."""
    x = torch.zeros(4, 2, 3, 32, 32, dtype=torch.uint8)
    x[0, 0] = nr.overshoot_image()[0]
    x[0, 1, :, 18:30, 3:14] = 230
    x[1, 0, :, 8:25, 12:30] = 120
    x[1, 1, :, 8:25, 12:30] = 180
    ramp = torch.arange(32)
    x[2, 0] = (3 * ramp).to(torch.uint8).view(1, 1, 32).expand(3, 32, 32)      # along columns
    x[2, 1] = (7 * ramp).to(torch.uint8).view(1, 32, 1).expand(3, 32, 32)      # along rows
    x[2, :, 1] = x[2, :, 0] // 2
    x[3] = x[0]
    return x
