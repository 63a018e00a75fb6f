"""Numpy reference of the instance split: the nearest seed inside the object (dfw_seg_boundary with `seeds`), components of
equal (byte, key) pairs (dfw_seg_components with `keys`) and their composition, objects.split_objects.  All integers.

nearest_search is the DEFINITION of one pass, pixel by pixel.  For a pixel p = (y, x) with v = m[p] != 0 a candidate is a
position q = (y + dy, x + dx) with seeds[q] != 0, dy^2 + dx^2 <= R^2 and an L path from p to q on v, the column first: m[y +
t][x] == v for every t between 0 and dy, then m[y + dy][x + s] == v for every s between 0 and dx.  nearest[p] is seeds[q] of
the candidate with the smallest (dy^2 + dx^2, seeds[q]), 0 without one; dist[p] the winner's dy^2 + dx^2 (0 on a seed), (R +
1)^2 without one; background has 0 and 0.

nearest_two_pass is the form the kernels use: per pixel the nearest seed of its row inside its run of equal value (row_seeds:
distance h, R + 1 for none within R, and value lab, the smaller one of two equally near), then per column the smallest (dy^2 +
h(y + dy, x)^2, lab(y + dy, x)) within R^2 over the rows the column reaches on v.  It walks all R rows and ends nothing
early.  tests/test_object_split_cpu.py shows that the two agree before any kernel is held against nearest_ref.

passes: pass k > 1 is the pass with seeds := the result, and a pixel that holds a value keeps it and its dist.

components_keyed: scipy's label per (byte, key) pair, renumbered by first pixel, then components_ref.assemble -- filter,
numbering, stats and counts are that reference's.  split_ref is the composition, from edt_ref and the functions here."""
import numpy as np

import components_ref as cr
import edt_ref as er


def nearest_search(m, seeds, R):
    """[H, W] maps -> (nearest int64, dist int64) of one pass, by the definition."""
    m, seeds = np.asarray(m), np.asarray(seeds)
    H, W = m.shape
    near, dist = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            v = m[y, x]
            if v == 0:
                continue
            best = None
            for sy in (1, -1):
                for ady in range(0 if sy > 0 else 1, R + 1):
                    yy = y + sy * ady
                    if not 0 <= yy < H or m[yy, x] != v:
                        break                                          # the column leaves the value: nothing behind it
                    for sx in (1, -1):
                        for adx in range(0 if sx > 0 else 1, R + 1):
                            xx = x + sx * adx
                            if not 0 <= xx < W or m[yy, xx] != v or ady * ady + adx * adx > R * R:
                                break
                            if seeds[yy, xx] != 0:
                                key = (ady * ady + adx * adx, int(seeds[yy, xx]))
                                if best is None or key < best:
                                    best = key
            dist[y, x], near[y, x] = best if best is not None else ((R + 1) ** 2, 0)
    return near, dist


def row_seeds(m, seeds, R):
    """[H, W] -> (h, lab) int64: the distance along the row to the nearest seed inside the pixel's run of equal value, R + 1
    when there is none within R, and that seed's value (the smaller of two equally near, 0 for none)."""
    m, seeds = np.asarray(m), np.asarray(seeds).astype(np.int64)
    H, W = m.shape
    idx = np.broadcast_to(np.arange(W), (H, W))
    brk = np.ones((H, W), bool)
    brk[:, 1:] = m[:, 1:] != m[:, :-1]
    start = np.maximum.accumulate(np.where(brk, idx, -1), axis=1)                    # the run's first position
    nxt = np.full((H, W), W)
    nxt[:, :-1] = np.where(brk[:, 1:], idx[:, 1:], W)
    end = np.minimum.accumulate(nxt[:, ::-1], axis=1)[:, ::-1]                       # the next run's first position
    is_seed = seeds != 0
    left = np.maximum.accumulate(np.where(is_seed, idx, -1), axis=1)                 # last seed at or before
    right = np.minimum.accumulate(np.where(is_seed, idx, 2 * W + R + 2)[:, ::-1], axis=1)[:, ::-1]   # next seed at or behind
    big = R + 1
    dl = np.where(left >= start, idx - left, big)
    dr = np.where(right < end, right - idx, big)
    rows = np.arange(H)[:, None]
    vl = seeds[rows, np.clip(left, 0, W - 1)]
    vr = seeds[rows, np.clip(right, 0, W - 1)]
    h = np.minimum(np.minimum(dl, dr), big)
    lab = np.where(dl < dr, vl, np.where(dr < dl, vr, np.minimum(vl, vr)))
    return h, np.where(h <= R, lab, 0)


def nearest_two_pass(m, seeds, R):
    """[H, W] maps -> (nearest int64, dist int64) of one pass, by the two-pass form, array shifts over dy."""
    m = np.asarray(m)
    H, W = m.shape
    h, lab = row_seeds(m, seeds, R)
    none = np.iinfo(np.int64).max
    best = np.where(h <= R, h * h, none)
    bl = lab.copy()
    for sign in (-1, 1):
        alive = m != 0
        for dy in range(1, min(R, H - 1) + 1):
            there = np.zeros((H, W), bool)
            hs, ls = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
            if sign > 0:
                there[:H - dy] = m[dy:] == m[:H - dy]
                hs[:H - dy], ls[:H - dy] = h[dy:], lab[dy:]
            else:
                there[dy:] = m[:H - dy] == m[dy:]
                hs[dy:], ls[dy:] = h[:H - dy], lab[:H - dy]
            alive &= there
            cand = dy * dy + hs * hs
            take = alive & (hs <= R) & (cand <= R * R) & ((cand < best) | ((cand == best) & (ls < bl)))
            best, bl = np.where(take, cand, best), np.where(take, ls, bl)
    fg = m != 0
    dist = np.where(fg, np.where(best == none, (R + 1) ** 2, best), 0)
    return np.where(fg & (best != none), bl, 0), dist


def nearest_image(m, seeds, R, passes=1, one=nearest_two_pass, trace=None):
    """`passes` passes on one image -> (nearest, dist).  trace: a list that receives every pass's nearest."""
    near, dist = one(m, seeds, R)
    if trace is not None:
        trace.append(near.copy())
    for _ in range(passes - 1):
        n2, d2 = one(m, near, R)
        have = near != 0
        near, dist = np.where(have, near, n2), np.where(have, dist, d2)
        if trace is not None:
            trace.append(near.copy())
    return near, dist


def nearest_ref(m, seeds, R, passes=1, one=nearest_two_pass):
    """[B, H, W] or [H, W] -> (nearest int32, dist uint16) as the library writes them."""
    m, seeds = np.asarray(m), np.asarray(seeds)
    assert 1 <= R <= 254 and 1 <= passes <= 8 and m.shape == seeds.shape
    if m.ndim == 2:
        n, d = nearest_image(m, seeds, R, passes, one)
        return n.astype(np.int32), d.astype(np.uint16)
    per = [nearest_image(a, s, R, passes, one) for a, s in zip(m, seeds)]
    return np.stack([p[0] for p in per]).astype(np.int32), np.stack([p[1] for p in per]).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ keyed components

def flood_keyed(lab, keys, connectivity=8):
    """lab uint8 [H, W], keys [H, W] -> components_ref.flood's list for components of equal (byte, key): scipy's label per
    pair, ordered by first pixel."""
    from scipy import ndimage
    lab, keys = np.asarray(lab, dtype=np.uint8), np.asarray(keys).astype(np.int64)
    W = lab.shape[1]
    structure = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    out = []
    pair = lab.astype(np.int64) * (1 << 33) + (keys + (1 << 31))
    for code in np.unique(pair[lab != 0]):
        parts, k = ndimage.label(pair == code, structure=structure)
        flat = parts.ravel()
        order = np.argsort(flat, kind="stable")                        # pixels in row-major order inside every part
        cuts = np.searchsorted(flat[order], np.arange(1, k + 2))
        for i in range(k):
            p = order[cuts[i]:cuts[i + 1]]
            out.append((int(code >> 33), p // W, p % W))
    out.sort(key=lambda c: int(c[1][0]) * W + int(c[2][0]))
    return out


def components_keyed(labels, keys, connectivity=8, min_area=0, cap=1024, gt=None, nlabels=None):
    """components_ref.components with the second plane: labels uint8 [B, H, W], keys [B, H, W]."""
    labels = np.asarray(labels, dtype=np.uint8)
    comps = [flood_keyed(l, k, connectivity) for l, k in zip(labels, np.asarray(keys))]
    return cr.components(labels, connectivity, min_area, cap, gt, nlabels, comps=comps)


# ------------------------------------------------------------------------------------------------ the composition

def split_ref(ids, labels, radius, reach=None, passes=3, min_area=0, connectivity=8, cap=1024):
    """ids int32 and labels uint8 [B, H, W] of a label_objects result -> dict: components_keyed's entries of the instances
    plus parent int32 [B, cap], cores (the cores' n), nearest int32 [B, H, W] and core_ids (the seeds)."""
    ids, labels = np.asarray(ids), np.asarray(labels, dtype=np.uint8)
    reach = min(254, 2 * radius + 2) if reach is None else reach
    d2 = er.dist2_ref(ids, max(radius, 1)).astype(np.int64)
    core = np.where(d2 > radius * radius, labels, 0).astype(np.uint8)
    cores = cr.components(core, connectivity, 0, cap)
    nearest, _ = nearest_ref(ids, cores["ids"], reach, passes)
    r = components_keyed(labels, nearest, connectivity, min_area, cap)
    B, H, W = ids.shape
    parent = np.zeros((B, cap), np.int32)
    for b in range(B):
        k = min(int(r["n"][b, 0]), cap)
        parent[b, :k] = ids[b].reshape(-1)[r["stats"][b, :k, 6]]
    return dict(r, parent=parent, cores=cores["n"], nearest=nearest, core_ids=cores["ids"])


# ------------------------------------------------------------------------------------------------ the case tables

def named_cases():
    """{name: (map, seeds, R)} of int32 [H, W] maps, one per way a pass can go wrong."""
    out = {}
    m = np.full((1, 9), 5)
    s = np.zeros((1, 9), np.int64)
    s[0, 2], s[0, 6] = 7, 3
    out["a tie left and right in a row: the smaller value"] = (m, s, 4)
    out["a tie up and down in a column"] = (m.T.copy(), s.T.copy(), 4)
    m = np.full((7, 7), 2)
    s = np.zeros((7, 7), np.int64)
    s[3, 6], s[0, 3], s[6, 3], s[3, 0] = 9, 4, 2, 8                         # all 3 from the centre
    out["equal distances, different values"] = (m, s, 3)
    m = np.full((3, 9), 1)
    m[1, 4] = 2
    s = np.zeros((3, 9), np.int64)
    s[1, 7] = 5
    out["a seed behind a gap of another value"] = (m, s, 8)
    m = np.zeros((2, 12), np.int64)
    m[:, :5], m[:, 6:] = 3, 4
    s = np.zeros((2, 12), np.int64)
    s[0, 8] = 6
    out["a seed of another object in the same row"] = (m, s, 11)
    m = np.full((5, 5), 1)
    s = np.zeros((5, 5), np.int64)
    s[0, 0], s[4, 4] = (1 << 31) - 1, -(1 << 31)
    s[0, 4] = -1
    out["seed values 2^31 - 1 and negative"] = (m, s, 4)
    m = np.zeros((6, 5), np.int64)
    m[1:5, 1:4] = 7
    s = np.zeros((6, 5), np.int64)
    s[0, 0], s[2, 2] = 4, 1                                                # a seed on background is never found
    out["a seed on background"] = (m, s, 3)
    comb = np.zeros((12, 17), np.int64)                                    # a spine with teeth: the spine lies row-first of the seed
    comb[1, 1:16] = 6
    comb[1:11, 1:16:2] = 6
    s = np.zeros_like(comb)
    s[10, 1] = 3
    out["a comb seeded at the tip of its first tooth"] = (comb, s, 20)
    u = np.zeros((12, 9), np.int64)                                        # a U: the far arm needs a second pass
    u[1:11, 1], u[1:11, 7], u[10, 1:8] = 4, 4, 4
    s = np.zeros_like(u)
    s[1, 1] = 8
    out["a U seeded at the top of its left arm"] = (u, s, 30)
    return {k: (a.astype(np.int32), b.astype(np.int32), R) for k, (a, b, R) in out.items()}


FAMILY = dict(radius=2, reach=8, passes=3, connectivity=8)                # what the random family is split with


def family(seed, H=48, W=56):
    """A uint8 label map [H, W] of the random family (H >= 40, W >= 52): ragged discs of three classes that touch and
    overlap, a sliver with no core, and a square with a corridor one pixel wide that turns seven times -- one horizontal
    and one vertical piece a pass, so its end stays unassigned after FAMILY's passes."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    lab = np.zeros((H, W), np.uint8)
    for _ in range(7):
        cy, cx, r = rs.randint(4, H - 18), rs.randint(4, W - 4), rs.randint(4, 8)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rs.randint(1, 4)
    a, b = rs.randint(6, 12), rs.randint(22, W - 21)                       # two discs of one class that touch over a neck
    lab[((yy - a) ** 2 + (xx - b) ** 2 <= 36) | ((yy - a) ** 2 + (xx - b - 11) ** 2 <= 36)] = 2
    lab[rs.rand(H, W) < 0.02] = 0
    lab[H - 16:, :] = 0
    lab[H - 15, 1:20] = 3                                                  # the sliver
    y0 = H - 13
    lab[y0:y0 + 9, 1:10] = 1                                               # the square: its core is 5 x 5 at radius 2
    x, y = 10, y0 + 4
    for k in range(4):                                                     # H1 V1 H2 V2 H3 V3 H4
        lab[y, x:x + 5] = 1
        x += 4
        if k < 3:
            y2 = y - 4 if k % 2 == 0 else y + 4
            lab[min(y, y2):max(y, y2) + 1, x] = 1
            y = y2
    return lab


FAMILY_SEEDS = (1, 2, 3)                                                   # the members the GPU tests use
