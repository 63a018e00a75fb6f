"""Numpy reference of the Euclidean side of the boundary stage (dfw_seg_boundary with metric = 1): the squared distance of
every pixel to its own contour, the band, and the inscribed-circle table.  All integers.

d2_search is the DEFINITION, pixel by pixel: for a pixel p = (y, x) with v = m[p] != 0, the smallest (y - y')^2 + (x - x')^2
over the integer positions (y', x') that lie outside the image or hold another value.  The nearest position outside the
image lies in the ring of width one around it, so the search covers [-1, H] x [-1, W].

d2_two_pass is the form the kernels use: h(y, x), the distance along the row to the nearest position that is outside the row
or holds another value (row_h), then per column
  D2(y, x) = min(min(y + 1, H - y)^2, min over dy of c(dy)),  c(0) = h(y, x)^2,
  c(dy) = dy^2 + h(y + dy, x)^2 while m[y + dy][x] == v, and dy^2 at the first row where it differs,
with nothing looked at beyond that row.  A row outside the image differs, which is the first term.  `cap` caps h first and
the result at cap^2 afterwards, as the library does with cap = dmax + 1.  tests/test_object_thickness_cpu.py shows that the
two agree, and that capping h changes no capped result, before any kernel is held against dist2_ref."""
import numpy as np


def d2_search(m):
    """[H, W] of any integer type -> int64 [H, W]: 0 on background, else the uncapped squared distance, by the definition."""
    m = np.asarray(m)
    H, W = m.shape
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            v = m[y, x]
            if v == 0:
                continue
            best = None
            for yy in range(-1, H + 1):
                for xx in range(-1, W + 1):
                    if not (0 <= yy < H and 0 <= xx < W) or m[yy, xx] != v:
                        c = (y - yy) ** 2 + (x - xx) ** 2
                        if best is None or c < best:
                            best = c
            out[y, x] = best
    return out


def row_h(m):
    """[H, W] -> int64 [H, W]: min(x - run start + 1, run end - x) of the run of equal values that holds x, run end exclusive;
    background pixels get their run's value as well (nobody reads it)."""
    m = np.asarray(m)
    H, W = m.shape
    h = np.zeros((H, W), np.int64)
    for y in range(H):
        x = 0
        while x < W:
            e = x
            while e < W and m[y, e] == m[y, x]:
                e += 1
            i = np.arange(x, e)
            h[y, x:e] = np.minimum(i - x + 1, e - i)
            x = e
    return h


def d2_two_pass(m, cap=None):
    """[H, W] -> int64 [H, W] by the two-pass form, array shifts over dy.  cap: h is capped at cap and the result at cap^2."""
    m = np.asarray(m)
    H, W = m.shape
    h = row_h(m)
    if cap is not None:
        h = np.minimum(h, cap)
    yy = np.arange(H)[:, None]
    best = np.minimum(h * h, np.broadcast_to(np.minimum(yy + 1, H - yy) ** 2, (H, W)))
    steps = max(H, 1) if cap is None else min(H, cap)
    for sign in (-1, 1):
        same = np.ones((H, W), bool)                   # the column holds v from y to y + sign * (dy - 1)
        for dy in range(1, steps + 1):
            there = np.zeros((H, W), bool)             # ... and at y + sign * dy, which lies inside the image
            hs = np.zeros((H, W), np.int64)
            if dy < H:
                if sign > 0:
                    there[:H - dy] = m[dy:] == m[:H - dy]
                    hs[:H - dy] = h[dy:]
                else:
                    there[dy:] = m[:H - dy] == m[dy:]
                    hs[dy:] = h[:H - dy]
            cand = np.where(there, dy * dy + hs * hs, dy * dy)
            best = np.where(same, np.minimum(best, cand), best)
            same &= there
            if not same.any():
                break
    best = np.where(m == 0, 0, best)
    return best if cap is None else np.minimum(best, cap * cap)


def dist2_ref(m, dmax):
    """[H, W] or [B, H, W] -> uint16 of the same shape: 0 on background, else min(D2, (dmax + 1)^2)."""
    m = np.asarray(m)
    assert 1 <= dmax <= 254
    if m.ndim == 2:
        return d2_two_pass(m, dmax + 1).astype(np.uint16)
    return np.stack([d2_two_pass(x, dmax + 1).astype(np.uint16) for x in m])


def band_ref(m, dist2, d):
    """The map restricted to 1 <= dist2 <= d^2."""
    m, dist2 = np.asarray(m), np.asarray(dist2).astype(np.int64)
    return np.where((dist2 >= 1) & (dist2 <= d * d), m, 0).astype(m.dtype)


def peak_key(r2, y, x, W):
    return (int(r2) << 32) | (0xFFFFFFFF - (int(y) * W + int(x)))


def peaks_ref(ids, dist2, cap):
    """ids, dist2 [B, H, W] -> int64 [B, cap]: row k - 1 = max over the pixels of id k of (dist2 << 32) | (2^32 - 1 - (y * W +
    x)), 0 when id k has no pixel; ids outside 1..cap are not counted.  Pixel by pixel, in Python integers."""
    ids, dist2 = np.asarray(ids), np.asarray(dist2)
    B, H, W = ids.shape
    out = np.zeros((B, cap), np.int64)
    for b in range(B):
        best = {}
        for p, (k, r2) in enumerate(zip(ids[b].reshape(-1).tolist(), dist2[b].reshape(-1).tolist())):
            if 1 <= k <= cap:
                key = (r2 << 32) | (0xFFFFFFFF - p)
                if key > best.get(k, 0):
                    best[k] = key
        for k, key in best.items():
            out[b, k - 1] = key
    return out


def decode_peak(key, W, dmax):
    """One row of peaks -> (r2, (y, x), capped), or (0, None, False) for an empty row."""
    key = int(key)
    if key == 0:
        return 0, None, False
    r2, pos = key >> 32, 0xFFFFFFFF - (key & 0xFFFFFFFF)
    return r2, (pos // W, pos % W), r2 == (dmax + 1) ** 2
