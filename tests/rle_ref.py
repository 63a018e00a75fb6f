"""Numpy reference of the run-length stage (dfw_seg_rle): flatten the id map in the asked order, keep ids 1..cap, find the
boundaries with np.diff, cut to max_runs in ascending start, then group by id with a stable argsort.  brute_runs is an
independent per-pixel loop for tiny maps."""
import numpy as np

ORDERS = ("row", "column")


def flatten(ids, order):
    """ids [H, W] -> the values by position: q = y * W + x ("row") or q = x * H + y ("column")."""
    assert order in ORDERS
    ids = np.asarray(ids)
    return (ids if order == "row" else ids.T).reshape(-1)


def rle_image(ids, cap, max_runs, order):
    """-> runs int32 [kept, 2] = (start, length) grouped by id, run_off int32 [cap + 1], (kept, found)."""
    v = flatten(ids, order).astype(np.int64)
    v = np.where((v >= 1) & (v <= cap), v, 0)
    ext = np.concatenate([v, [0]])                                     # position HW, behind the image, closes the last run
    edge = np.flatnonzero(np.diff(np.concatenate([[0], ext])))         # every q in 0..HW with v(q) != v(q - 1)
    starts = edge[ext[edge] != 0]
    # the run that starts at an edge ends at the next one: the next change of value
    nxt = edge[np.searchsorted(edge, starts, side="right")]
    found = len(starts)
    kept = min(found, max_runs)
    s, l, key = starts[:kept], (nxt - starts)[:kept], v[starts[:kept]]
    perm = np.argsort(key, kind="stable")
    runs = np.stack([s[perm], l[perm]], 1).astype(np.int32).reshape(-1, 2)
    run_off = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=cap + 1)[1:cap + 1])]).astype(np.int32)
    return runs, run_off, (kept, found)


def rle(ids, cap, max_runs, order):
    """ids [B, H, W] -> dict(runs: list of [kept_b, 2], run_off [B, cap + 1], nruns [B, 2])."""
    per = [rle_image(i, cap, max_runs, order) for i in ids]
    return dict(runs=[p[0] for p in per], run_off=np.stack([p[1] for p in per]), nruns=np.array([p[2] for p in per], np.int32))


def object_rows(runs, run_off, k):
    return runs[run_off[k - 1]:run_off[k]]


def brute_runs(ids, k, order):
    """The runs of object k, pixel by pixel: a list of (start, length)."""
    H, W = len(ids), len(ids[0])
    out, start, q = [], None, 0
    outer, inner = (H, W) if order == "row" else (W, H)
    for a in range(outer):
        for b in range(inner):
            on = (ids[a][b] if order == "row" else ids[b][a]) == k
            if on and start is None:
                start = q
            if not on and start is not None:
                out.append((start, q - start))
                start = None
            q += 1
    if start is not None:
        out.append((start, q - start))
    return out


# ------------------------------------------------------------------------------------------------ label maps to encode

def contents(H, W, rs):
    """uint8 label maps [H, W] by name: the contents of the components tests plus stripes two pixels thick, which give many
    runs per object in one order and, in the other, one run that wraps a line's end."""
    yy, xx = np.mgrid[:H, :W]
    snake = np.zeros((H, W), np.uint8)
    snake[::2] = 1
    for y in range(1, H, 2):
        snake[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    d = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
    noise = lambda p: ((rs.rand(H, W) < p) * rs.randint(1, 4, (H, W))).astype(np.uint8)  # noqa: E731
    return {"background": np.zeros((H, W), np.uint8), "one object": np.full((H, W), 7, np.uint8),
            "checkerboard": (((yy + xx) % 2) * 2).astype(np.uint8), "vertical stripes": (1 + xx // 2 % 2).astype(np.uint8),
            "horizontal stripes": (1 + yy // 2 % 2).astype(np.uint8), "snake": snake, "rings": (1 + d % 2).astype(np.uint8),
            "noise 0.3": noise(0.3), "noise 0.5": noise(0.5)}
