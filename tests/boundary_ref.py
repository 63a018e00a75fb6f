"""Numpy reference of the boundary stage (dfw_seg_boundary, dfw_seg_boundary_counts).  dist_ref follows the published
mask_to_boundary literally: per distinct value, the binary mask is padded with one ring of zeros and eroded with a 3 x 3
kernel, one iteration a step, by array shifts; a pixel that iteration k removes has distance k.  dist_loop is an independent
per-pixel search over growing squares, for tiny maps.  counts_ref applies the count rule pixel by pixel in Python integers."""
import math

import numpy as np


def erode(mask):
    """One 3 x 3 erosion of a boolean mask whose surroundings are zeros."""
    H, W = mask.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = mask
    out = np.ones((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + H, dx:dx + W]
    return out


def dist_image(m, dmax):
    m = np.asarray(m)
    dist = np.zeros(m.shape, np.int64)
    for v in np.unique(m):
        if v == 0:
            continue
        mask = m == v
        dist[mask] = dmax + 1
        for k in range(1, dmax + 1):
            nxt = erode(mask)
            dist[mask & ~nxt] = k
            mask = nxt
            if not mask.any():
                break
    return dist.astype(np.uint8)


def dist_ref(m, dmax):
    """[H, W] or [B, H, W] of any integer type -> uint8 dist of the same shape: 0 on background, else min(D, dmax + 1)."""
    m = np.asarray(m)
    assert 1 <= dmax <= 254
    if m.ndim == 2:
        return dist_image(m, dmax)
    return np.stack([dist_image(x, dmax) for x in m])


def dist_loop(m, dmax):
    """The definition, pixel by pixel: the smallest k for which the square of radius k holds a position outside the image
    or another value."""
    m = np.asarray(m)
    H, W = m.shape
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            v = m[y, x]
            if v == 0:
                continue
            k = 1
            while k <= dmax:
                hit = False
                for yy in range(y - k, y + k + 1):
                    for xx in range(x - k, x + k + 1):
                        if not (0 <= yy < H and 0 <= xx < W) or m[yy, xx] != v:
                            hit = True
                if hit:
                    break
                k += 1
            out[y, x] = k
    return out


def band_ref(m, dist, d):
    """The map restricted to 1 <= dist <= d."""
    m, dist = np.asarray(m), np.asarray(dist)
    return np.where((dist >= 1) & (dist <= d), m, 0).astype(m.dtype)


def width(h, w, ratio=0.02):
    return max(1, int(round(ratio * math.sqrt(h * h + w * w))))


def published_boundary(mask, d):
    """mask_to_boundary of the Boundary IoU paper's code with numpy shifts in place of cv2: pad the uint8 mask with one ring
    of zeros, erode with a 3 x 3 kernel of ones d times, cut the ring off, mask - eroded."""
    mask = np.asarray(mask).astype(np.uint8)
    h, w = mask.shape
    padded = np.zeros((h + 2, w + 2), np.uint8)
    padded[1:-1, 1:-1] = mask
    er = padded.astype(bool)
    for _ in range(d):
        # cv2.erode's default border is "+inf": the outermost ring of the padded mask is zero anyway, and stays zero
        q = np.ones((h + 4, w + 4), bool)
        q[1:-1, 1:-1] = er
        out = np.ones((h + 2, w + 2), bool)
        for dy in range(3):
            for dx in range(3):
                out &= q[dy:dy + h + 2, dx:dx + w + 2]
        er = out
    return mask - er[1:-1, 1:-1].astype(np.uint8)


def counts_ref(pred, pdist, gt, gdist, d, nlabels):
    """[B, H, W] maps -> int64 [B, 2, nlabels + 1] = (intersections, unions), in Python integers."""
    pred, pdist, gt, gdist = (np.asarray(a) for a in (pred, pdist, gt, gdist))
    B = pred.shape[0]
    out = np.zeros((B, 2, nlabels + 1), np.int64)
    for b in range(B):
        npred, ngt, inter = [0] * 256, [0] * 256, [0] * 256
        for p, pd, g, gd in zip(pred[b].reshape(-1).tolist(), pdist[b].reshape(-1).tolist(), gt[b].reshape(-1).tolist(),
                                gdist[b].reshape(-1).tolist()):
            if g > nlabels:
                continue
            l = p if 1 <= pd <= d else 0
            gg = g if 1 <= gd <= d else 0
            npred[l] += 1
            ngt[gg] += 1
            if l == gg:
                inter[l] += 1
        for c in range(nlabels + 1):
            out[b, 0, c] = inter[c]
            out[b, 1, c] = npred[c] + ngt[c] - inter[c]
    return out
