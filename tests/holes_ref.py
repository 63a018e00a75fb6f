"""Plain numpy reference of ops.seg_holes / dfw_seg_holes, and a per-pixel search that states the definition.

A pixel whose labels byte is 0 is background.  A region is a connected component of background pixels under the dual
connectivity hc (4 when the objects' connectivity is 8, 8 when it is 4).  It is enclosed when none of its pixels lies on
the first or last row or column; its owner is the ids value left of its first pixel (the smallest y * W + x); its border
pixels are the non-background pixels in the hc-neighbourhood of its pixels.  It is FILLED when it is enclosed, owner >= 1,
every border pixel has ids == owner and its area is at most max_area (None: no limit; 0 fills nothing): every pixel of it
then takes the owner's id and the labels byte of the pixel left of the first pixel.

holes_image takes the regions from components_ref.flood on the inverted map and applies the rules with numpy;
holes_search walks every pixel in row-major order and decides each region by itself, with no helper.  Per image both give

  ids_out     int32 [H, W]
  labels_out  uint8 [H, W]
  holes       (regions filled, regions enclosed)
  filled      {owner id: filled pixels}
"""
import numpy as np

import components_ref as cr

NO_LIMIT = 2 ** 31 - 1


def dual(connectivity):
    return {8: 4, 4: 8}[connectivity]


def holes_image(lab, ids, connectivity=8, max_area=None):
    lab, ids = np.asarray(lab, dtype=np.uint8), np.asarray(ids, dtype=np.int32)
    H, W = lab.shape
    hc = dual(connectivity)
    limit = NO_LIMIT if max_area is None else int(max_area)
    ids_out, labels_out = ids.copy(), lab.copy()
    nfilled = nenclosed = 0
    filled = {}
    for _, ys, xs in cr.flood((lab == 0).astype(np.uint8), hc):
        if ys.min() == 0 or xs.min() == 0 or ys.max() == H - 1 or xs.max() == W - 1:
            continue
        nenclosed += 1
        owner = int(ids[ys[0], xs[0] - 1])
        ny = np.concatenate([ys + dy for dy, dx in cr.NEIGHBOURS[hc]])
        nx = np.concatenate([xs + dx for dy, dx in cr.NEIGHBOURS[hc]])
        border = lab[ny, nx] != 0
        if owner < 1 or len(ys) > limit or (ids[ny, nx][border] != owner).any():
            continue
        nfilled += 1
        ids_out[ys, xs] = owner
        labels_out[ys, xs] = lab[ys[0], xs[0] - 1]
        filled[owner] = filled.get(owner, 0) + len(ys)
    return ids_out, labels_out, (nfilled, nenclosed), filled


def holes_search(lab, ids, connectivity=8, max_area=None):
    """The definition, pixel by pixel."""
    lab, ids = np.asarray(lab, dtype=np.uint8).tolist(), np.asarray(ids, dtype=np.int32).tolist()
    H, W = len(lab), len(lab[0])
    steps = cr.NEIGHBOURS[dual(connectivity)]
    limit = NO_LIMIT if max_area is None else int(max_area)
    ids_out, labels_out = [row[:] for row in ids], [row[:] for row in lab]
    seen = [[False] * W for _ in range(H)]
    nfilled = nenclosed = 0
    filled = {}
    for y in range(H):
        for x in range(W):
            if lab[y][x] != 0 or seen[y][x]:
                continue
            seen[y][x] = True                                             # (y, x) is the region's first pixel
            todo, region, border, enclosed = [(y, x)], [], [], True
            while todo:
                py, px = todo.pop()
                region.append((py, px))
                if py == 0 or py == H - 1 or px == 0 or px == W - 1:
                    enclosed = False
                for dy, dx in steps:
                    qy, qx = py + dy, px + dx
                    if not (0 <= qy < H and 0 <= qx < W):
                        continue
                    if lab[qy][qx] != 0:
                        border.append((qy, qx))
                    elif not seen[qy][qx]:
                        seen[qy][qx] = True
                        todo.append((qy, qx))
            if not enclosed:
                continue
            nenclosed += 1
            owner = ids[y][x - 1]
            if owner < 1 or len(region) > limit or any(ids[qy][qx] != owner for qy, qx in border):
                continue
            nfilled += 1
            for py, px in region:
                ids_out[py][px] = owner
                labels_out[py][px] = lab[y][x - 1]
            filled[owner] = filled.get(owner, 0) + len(region)
    return np.array(ids_out, np.int32).reshape(H, W), np.array(labels_out, np.uint8).reshape(H, W), (nfilled, nenclosed), filled


def stats_image(stats, filled):
    """stats int32 [cap, 8] -> stats_out: column 1 grown by, column 7 set to, the filled pixels of the ids <= cap."""
    out = np.array(stats, dtype=np.int32, copy=True)
    for owner, k in filled.items():
        if owner <= out.shape[0]:
            out[owner - 1, 1] += k
            out[owner - 1, 7] = k
    return out


def holes(labels, ids, connectivity=8, max_area=None, stats=None, gt=None, nlabels=None, image=holes_image):
    """labels uint8 [B, H, W], ids int32 [B, H, W] -> dict of numpy arrays: ids int32 [B, H, W], labels uint8 [B, H, W],
    holes int32 [B, 2], stats int32 [B, cap, 8] or None, counts int64 [B, 2, nlabels + 1] or None."""
    labels, ids = np.asarray(labels, dtype=np.uint8), np.asarray(ids, dtype=np.int32)
    assert labels.ndim == 3 and ids.shape == labels.shape
    per = [image(l, i, connectivity, max_area) for l, i in zip(labels, ids)]
    out = dict(ids=np.stack([p[0] for p in per]), labels=np.stack([p[1] for p in per]),
               holes=np.array([p[2] for p in per], dtype=np.int32), stats=None, counts=None)
    if stats is not None:
        out["stats"] = np.stack([stats_image(s, p[3]) for s, p in zip(np.asarray(stats), per)])
    if gt is not None:
        out["counts"] = np.stack([cr.counts_image(f, g, nlabels) for f, g in zip(out["labels"], np.asarray(gt, dtype=np.uint8))])
    return out
