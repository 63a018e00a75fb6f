"""Plain numpy reference of ops.seg_components / dfw_seg_components: a flood fill, one component at a time.

Two pixels belong to one component when they carry the same NON-ZERO byte and a 4- or 8-connected path of that byte joins
them.  Components are found in row-major order of their first pixel (the smallest y * W + x), so that order IS the numbering;
a component with fewer than min_area pixels is removed and takes no number.  Per image:

  ids       int32 [H, W]   0 = background or removed, else 1..n
  filtered  uint8 [H, W]   the label bytes with the removed components set to 0
  n         (kept, found before the filter)
  stats     int32 [cap, 8] row id - 1 = (label, area, y0, x0, y1, x1 half-open, first pixel, 0); rows from min(n, cap) on zero
  counts    int64 [2, nlabels + 1], nway_ref.counts' rule on the FILTERED bytes; a filtered byte above nlabels has no bin
"""
import numpy as np

NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def flood(lab, connectivity=8):
    """lab uint8 [H, W] -> the components in row-major order of their first pixel: a list of (label, ys, xs), the first
    pixel at index 0 of ys / xs.  The slow part, independent of min_area and cap."""
    lab = np.asarray(lab, dtype=np.uint8)
    H, W = lab.shape
    nb = NEIGHBOURS[connectivity]
    seen = (lab == 0).tolist()
    rows = lab.tolist()
    out = []
    for y in range(H):
        for x in range(W):
            if seen[y][x]:
                continue
            c = rows[y][x]
            seen[y][x] = True
            stack, pix = [(y, x)], []
            while stack:
                py, px = stack.pop()
                pix.append((py, px))
                for dy, dx in nb:
                    qy, qx = py + dy, px + dx
                    if 0 <= qy < H and 0 <= qx < W and not seen[qy][qx] and rows[qy][qx] == c:
                        seen[qy][qx] = True
                        stack.append((qy, qx))
            out.append((c, np.array([p[0] for p in pix]), np.array([p[1] for p in pix])))
    return out


def assemble(lab, comps, min_area=0, cap=1024):
    """flood's components of lab, filtered and numbered -> (ids, filtered, (kept, found), stats)."""
    lab = np.asarray(lab, dtype=np.uint8)
    W = lab.shape[1]
    ids = np.zeros(lab.shape, dtype=np.int32)
    filtered = lab.copy()
    stats = np.zeros((cap, 8), dtype=np.int32)
    kept = 0
    for c, ys, xs in comps:
        if len(ys) < min_area:
            filtered[ys, xs] = 0
            continue
        kept += 1
        ids[ys, xs] = kept
        if kept <= cap:
            stats[kept - 1] = (c, len(ys), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1, ys[0] * W + xs[0], 0)
    return ids, filtered, (kept, len(comps)), stats


def components_image(lab, connectivity=8, min_area=0, cap=1024):
    """lab uint8 [H, W] -> (ids, filtered, (kept, found), stats)."""
    return assemble(lab, flood(lab, connectivity), min_area, cap)


def counts_image(filtered, gt, nlabels):
    """int64 [2, nlabels + 1]: row 0 filtered == gt == l, row 1 pred_l + gt_l - inter_l over the pixels with gt <= nlabels."""
    f, g = np.asarray(filtered).astype(np.int64).ravel(), np.asarray(gt).astype(np.int64).ravel()
    keep = g <= nlabels
    f, g = f[keep], g[keep]
    nb = nlabels + 1
    pred = np.bincount(f, minlength=256)[:nb]
    gth = np.bincount(g, minlength=nb)[:nb]
    inter = np.bincount(f[f == g], minlength=256)[:nb]
    return np.stack([inter, pred + gth - inter]).astype(np.int64)


def components(labels, connectivity=8, min_area=0, cap=1024, gt=None, nlabels=None, comps=None):
    """labels uint8 [B, H, W] (numpy or anything np.asarray takes) -> dict of numpy arrays: ids int32 [B, H, W], filtered
    uint8 [B, H, W], n int32 [B, 2], stats int32 [B, cap, 8], counts int64 [B, 2, nlabels + 1] or None.  comps: flood() of
    every image for this connectivity, when the caller already has it."""
    labels = np.asarray(labels, dtype=np.uint8)
    assert labels.ndim == 3
    comps = [flood(l, connectivity) for l in labels] if comps is None else comps
    per = [assemble(l, c, min_area, cap) for l, c in zip(labels, comps)]
    out = dict(ids=np.stack([p[0] for p in per]), filtered=np.stack([p[1] for p in per]),
               n=np.array([p[2] for p in per], dtype=np.int32), stats=np.stack([p[3] for p in per]), counts=None)
    if gt is not None:
        gt = np.asarray(gt, dtype=np.uint8)
        out["counts"] = np.stack([counts_image(f, g, nlabels) for f, g in zip(out["filtered"], gt)])
    return out
