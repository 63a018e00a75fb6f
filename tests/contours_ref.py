"""Numpy / Python reference of the outline stage (dfw_seg_contours), by the definition in include/diffews_hip.h: the edges
come from numpy shifts, the successor rule is evaluated for all edges at once, and only the walk along the cycles is a
Python loop over the edges (never over the pixels), so maps of half a megapixel take seconds.

    values(ids, cap)                   the map with everything outside 1..cap set to 0
    edges(ids, cap)                    the sorted edge keys 4 * (y * W + x) + side
    successor(ids, cap, conn, keys)    per edge the index of its successor (-1: none, never for a bijection) and the turn
    trace(ids, cap, conn)              everything about one image: rings sorted by (id, leader), corners, areas, ring_off
    expected(ids, cap, conn, max_edges)  what the device call writes for a batch: n, rings, ring_off, verts
    rasterise(rings, h, w)             [(area, corners)] -> bool [h, w]
"""
import numpy as np

DY = np.array([0, 1, 0, -1])    # heading of side 0 (top, east), 1 (right, south), 2 (bottom, west), 3 (left, north)
DX = np.array([1, 0, -1, 0])
# start vertex of an edge relative to its pixel (x, y)
SX = np.array([0, 1, 1, 0])
SY = np.array([0, 0, 1, 1])


def values(ids, cap):
    ids = np.asarray(ids).astype(np.int64)
    return np.where((ids >= 1) & (ids <= cap), ids, 0)


def edges(ids, cap):
    v = values(ids, cap)
    H, W = v.shape
    P = np.pad(v, 1)
    across = [P[:-2, 1:-1], P[1:-1, 2:], P[2:, 1:-1], P[1:-1, :-2]]      # the pixel across the top, right, bottom, left
    keys = []
    for s in range(4):
        y, x = np.nonzero((v != 0) & (across[s] != v))
        keys.append(4 * (y * W + x) + s)
    return np.sort(np.concatenate(keys)).astype(np.int64)


def successor(ids, cap, connectivity, keys=None):
    assert connectivity in (4, 8)
    v = values(ids, cap)
    H, W = v.shape
    keys = edges(ids, cap) if keys is None else keys
    if len(keys) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    P = np.pad(v, 1)
    p, s = keys >> 2, keys & 3
    y, x = p // W, p % W
    i = v[y, x]
    dy, dx = DY[s], DX[s]
    ay, ax = y + dy, x + dx             # ahead
    ly, lx = ay - dx, ax + dy           # left of ahead, relative to the heading (y grows downwards)
    vA, vL = P[ay + 1, ax + 1], P[ly + 1, lx + 1]
    if connectivity == 8:
        left = vL == i
        straight = ~left & (vA == i)
    else:
        right = vA != i
        left = ~right & (vL == i)
        straight = ~right & ~left
    nk = np.where(left, 4 * (ly * W + lx) + (s + 3) % 4, np.where(straight, 4 * (ay * W + ax) + s, 4 * p + (s + 1) % 4))
    idx = np.clip(np.searchsorted(keys, nk), 0, len(keys) - 1)
    idx = np.where(keys[idx] == nk, idx, -1)
    turn = np.where(left, -1, np.where(straight, 0, 1))
    return idx, turn


def trace(ids, cap, connectivity):
    """One image [H, W] -> dict(nedges, keys, succ, rings int64 [r, 4] = (id, first, count, area), leaders [r] (keys),
    lengths [r], verts int64 [corners, 2], ring_off [cap + 1])."""
    v = values(ids, cap)
    H, W = v.shape
    keys = edges(ids, cap)
    succ, turn = successor(ids, cap, connectivity, keys)
    n = len(keys)
    assert (succ >= 0).all() and len(np.unique(succ)) == n, "the successor is not a bijection"
    p, s = keys >> 2, keys & 3
    y, x = p // W, p % W
    vx, vy = (x + SX[s]).tolist(), (y + SY[s]).tolist()
    term = np.where(s == 1, x + 1, np.where(s == 3, -x, 0)).tolist()
    eid = v[y, x].tolist()
    nxt, trn = succ.tolist(), turn.tolist()
    corner = [False] * n
    for c in range(n):
        if trn[c] != 0:
            corner[nxt[c]] = True                                         # its predecessor has another heading
    seen = [False] * n
    found = []
    for c in range(n):                                                     # ascending: the first edge met is the leader
        if seen[c]:
            continue
        pts, area, length, e = [], 0, 0, c
        while not seen[e]:
            seen[e] = True
            assert eid[e] == eid[c], "a ring belongs to one id"
            if corner[e]:
                pts.append((vx[e], vy[e]))
            area += term[e]
            length += 1
            e = nxt[e]
        assert e == c
        found.append((eid[c], int(keys[c]), length, area, pts))
    found.sort(key=lambda r: (r[0], r[1]))
    rings, verts, at = [], [], 0
    for i, k, length, area, pts in found:
        rings.append((i, at, len(pts), area))
        verts += pts
        at += len(pts)
    counts = np.bincount([r[0] for r in found], minlength=cap + 1)[:cap + 1]
    return dict(nedges=n, keys=keys, succ=succ, rings=np.array(rings, np.int64).reshape(-1, 4),
                leaders=np.array([r[1] for r in found], np.int64), lengths=np.array([r[2] for r in found], np.int64),
                verts=np.array(verts, np.int64).reshape(-1, 2), ring_off=np.cumsum(counts).astype(np.int64))


def expected(ids, cap, connectivity, max_edges):
    """ids [B, H, W] -> per image what dfw_seg_contours writes: a list of dict(n [4], rings [r, 4], verts [c, 2], ring_off
    [cap + 1]); an image with more than max_edges edges has n = (found, 0, 0, 0), no rows and a zero ring_off."""
    out = []
    for m in np.asarray(ids):
        found = len(edges(m, cap))
        if found > max_edges:
            out.append(dict(n=np.array([found, 0, 0, 0]), rings=np.zeros((0, 4), np.int64), verts=np.zeros((0, 2), np.int64),
                            ring_off=np.zeros(cap + 1, np.int64)))
            continue
        t = trace(m, cap, connectivity)
        out.append(dict(n=np.array([found, len(t["verts"]), len(t["rings"]), 1]), rings=t["rings"], verts=t["verts"],
                        ring_off=t["ring_off"]))
    return out


def object_rings(t, k):
    """Object k's rings of a trace as [(area, corners [c, 2])]."""
    lo, hi = (0 if k == 1 else t["ring_off"][k - 1]), t["ring_off"][k]
    return [(int(a), t["verts"][f:f + c]) for _, f, c, a in t["rings"][lo:hi].tolist()]


def rasterise(rings, h, w):
    """[(area, corners [c, 2])] -> bool [h, w]: every vertical side of every ring adds -1 (heading south, the object to
    its west) or +1 (heading north) per row it spans at its column, and the sum along x is the winding."""
    acc = np.zeros((h, w + 1), np.int64)
    for _, pts in rings:
        pts = np.asarray(pts, np.int64).reshape(-1, 2).tolist()
        for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
            if x0 == x1 and y1 > y0:
                acc[y0:y1, x0] -= 1
            elif x0 == x1 and y1 < y0:
                acc[y1:y0, x0] += 1
    return np.cumsum(acc, axis=1)[:, :w] > 0
