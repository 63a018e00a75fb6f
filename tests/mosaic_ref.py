"""A reference of ops.seg_components that stays affordable at millions of pixels: the label map is a MOSAIC, a grid of
rectangular cells separated by one background row and one background column, so that neither neighbourhood joins two cells.
Every cell is a crop of one of a handful of small label maps (TEMPLATES); each distinct (template, height, width) is flood
filled once by components_ref.flood, and every component of every cell instance is that cell's component shifted by the
cell's origin.  Components are then numbered by first pixel in row-major order over the whole image, and ids, filtered, n,
stats and counts follow with numpy only (assemble, on a component TABLE).

A table of one image is a dict of numpy arrays: ord int32 [H, W] = the component's index in row-major order of the first
pixels, -1 for background; label, area, y0, x0, y1, x1, first per component.  table_of_flood builds the same table from
components_ref.flood's list, so the numpy assemble serves the flood fill at sizes where components_ref.assemble's loop
over the components is the slow part."""
import numpy as np

import components_ref as cr

CELL_H, CELL_W = 70, 150            # larger than the 32 x 64 tile of the LDS pass in both axes
TEMPLATES = ("snake", "noise 0.3", "percolation 4", "percolation 8", "rings")
FEW_OBJECTS = ("discs",)            # three objects a cell, and compact ones, which a perturbation does not cut to pieces


def _snake(H, W):
    lab = np.zeros((H, W), np.uint8)
    lab[::2] = 1
    for y in range(1, H, 2):
        lab[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return lab


def templates(rs, nlabels=3, cell=(CELL_H, CELL_W)):
    """The distinct small label maps, one cell each: the snake and the percolation-density noise of
    tests/test_components_gpu.py (tile-local roots that really need flattening), noise at 0.3 of three classes, rings, and
    three discs."""
    H, W = cell
    yy, xx = np.mgrid[:H, :W]
    d = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
    discs = np.zeros((H, W), np.uint8)
    top = min(H // 2 - 1, W // 6 - 2)
    for k in range(3):                                                   # three discs, each inside its third of the width
        r = rs.randint(max(1, top // 2), top + 1) if top >= 1 else 0
        cy = rs.randint(r, H - r)
        discs[(yy - cy) ** 2 + (xx - (2 * k + 1) * W // 6) ** 2 <= r * r] = rs.randint(1, nlabels + 1)
    return {"snake": _snake(H, W), "discs": discs,
            "noise 0.3": ((rs.rand(H, W) < 0.3) * rs.randint(1, nlabels + 1, (H, W))).astype(np.uint8),
            "percolation 4": (rs.rand(H, W) < 0.6).astype(np.uint8) * 2,
            "percolation 8": (rs.rand(H, W) < 0.41).astype(np.uint8) * 3,
            "rings": (1 + d % 2).astype(np.uint8)}


def spans(total, cell, least):
    """[(origin, size)] along one axis: cells of `cell` pixels, one background pixel between two cells; the last cell takes
    what is left, and is wider than `least`.  The cells reach the image's last pixel."""
    assert total > least
    out, at = [], 0
    while total - at - (cell + 1) > least:
        out.append((at, cell))
        at += cell + 1
    out.append((at, total - at))
    assert least < out[-1][1] <= 2 * cell + 1
    return out


def layout(H, W, rs, names=TEMPLATES, cell=(CELL_H, CELL_W), least=(32, 64)):
    """[(y, x, h, w, template name)] of every cell of an H x W mosaic, the template drawn at random; every cell is larger
    than `least`, the tile, in both axes."""
    return [(y, x, h, w, names[rs.randint(len(names))]) for y, h in spans(H, cell[0], least[0])
            for x, w in spans(W, cell[1], least[1])]


def crop(t, h, w):
    """A cell of h x w from a template: the template tiled to the size, so a cell larger than the template is full."""
    return np.tile(t, (-(-h // t.shape[0]), -(-w // t.shape[1])))[:h, :w]


def table_of_flood(lab, comps):
    """components_ref.flood's list -> the table."""
    H, W = lab.shape
    n = len(comps)
    size = np.array([len(c[1]) for c in comps], np.int64)
    ys = np.concatenate([c[1] for c in comps]) if n else np.zeros(0, np.int64)
    xs = np.concatenate([c[2] for c in comps]) if n else np.zeros(0, np.int64)
    who = np.repeat(np.arange(n), size)
    ordm = np.full((H, W), -1, np.int32)
    ordm[ys, xs] = who
    start = np.concatenate([[0], np.cumsum(size)])[:-1]
    red = lambda f, v: f.reduceat(v, start) if n else np.zeros(0, np.int64)  # noqa: E731
    return dict(ord=ordm, label=np.array([c[0] for c in comps], np.int64), area=size, y0=red(np.minimum, ys), x0=red(np.minimum, xs),
                y1=red(np.maximum, ys) + 1, x1=red(np.maximum, xs) + 1,
                first=(ys[start] * W + xs[start]) if n else np.zeros(0, np.int64))


def mosaic(H, W, cells, temps, connectivity):
    """-> (label map uint8 [H, W], its table), every distinct cell flood filled once."""
    lab = np.zeros((H, W), np.uint8)
    ordm = np.full((H, W), -1, np.int64)
    done, cols, base = {}, {k: [] for k in ("label", "area", "y0", "x0", "y1", "x1", "first")}, 0
    for y, x, h, w, name in cells:
        key = (name, h, w)
        if key not in done:
            cell = crop(temps[name], h, w)
            done[key] = (cell, table_of_flood(cell, cr.flood(cell, connectivity)))
        cell, t = done[key]
        lab[y:y + h, x:x + w] = cell
        ordm[y:y + h, x:x + w] = np.where(t["ord"] >= 0, t["ord"] + base, -1)
        fy, fx = t["first"] // w, t["first"] % w
        for k, v in (("label", t["label"]), ("area", t["area"]), ("y0", t["y0"] + y), ("x0", t["x0"] + x), ("y1", t["y1"] + y),
                     ("x1", t["x1"] + x), ("first", (fy + y) * W + fx + x)):
            cols[k].append(v)
        base += len(t["area"])
    tab = {k: np.concatenate(v) for k, v in cols.items()}
    perm = np.argsort(tab["first"], kind="stable")                       # first pixels are distinct: the numbering
    rank = np.empty(base + 1, np.int32)
    rank[perm] = np.arange(base, dtype=np.int32)
    rank[base] = -1                                                      # background indexes the last entry
    tab = {k: v[perm] for k, v in tab.items()}
    tab["ord"] = rank[ordm]
    return lab, tab


def assemble(lab, tab, min_area=0, cap=1024):
    """components_ref.assemble on a table: (ids, filtered, (kept, found), stats), numpy only."""
    keep = tab["area"] >= min_area
    new = np.concatenate([np.where(keep, np.cumsum(keep), 0), [0]]).astype(np.int32)      # background indexes the last entry
    ids = new[tab["ord"]]
    filtered = np.where(ids > 0, lab, 0).astype(np.uint8)
    kept = int(keep.sum())
    stats = np.zeros((cap, 8), np.int32)
    rows = np.flatnonzero(keep)[:cap]
    for j, k in enumerate(("label", "area", "y0", "x0", "y1", "x1", "first")):
        stats[:len(rows), j] = tab[k][rows]
    return ids, filtered, (kept, len(keep)), stats


def components(labels, tables, min_area=0, cap=1024, gt=None, nlabels=None):
    """components_ref.components with the tables of the images in place of their flood fills."""
    per = [assemble(l, t, min_area, cap) for l, t in zip(labels, tables)]
    out = dict(ids=np.stack([p[0] for p in per]), filtered=np.stack([p[1] for p in per]),
               n=np.array([p[2] for p in per], dtype=np.int32), stats=np.stack([p[3] for p in per]), counts=None)
    if gt is not None:
        out["counts"] = np.stack([cr.counts_image(f, g, nlabels) for f, g in zip(out["filtered"], gt)])
    return out
