"""Numpy reference of the matching stage (dfw_seg_match), truncation included: the key stream p * (cap_g + 1) + g with
skipped pixels and ids outside 1..cap as 0, its records by np.diff, cut to max_records in ascending start; the pairs by
np.unique on the kept records, cut to max_pairs in ascending key; areas as row and column sums of the kept pairs; the match
rule in exact Python integers.  pixel_pairs and brute_matches are independent per-pixel / per-object loops for tiny maps."""
import numpy as np


def classes_of(stats, cap):
    """Column 0 of a stats table [cap, 8] (or a plain class list), or 1 for every object without one."""
    if stats is None:
        return [1] * cap
    s = np.asarray(stats)
    return (s[:, 0] if s.ndim == 2 else s).tolist()


def keys(pids, gids, cap_p, cap_g, skip=None):
    p = np.asarray(pids).astype(np.int64).reshape(-1)
    g = np.asarray(gids).astype(np.int64).reshape(-1)
    p = np.where((p >= 1) & (p <= cap_p), p, 0)
    g = np.where((g >= 1) & (g <= cap_g), g, 0)
    k = p * (cap_g + 1) + g
    if skip is not None:
        k = np.where(np.asarray(skip).reshape(-1) == 255, 0, k)
    return k


def records(k, max_records):
    """The key stream -> (key, length) of the kept records in ascending start, (kept, found)."""
    ext = np.concatenate([k, [0]])                                     # position HW, behind the image, closes the last record
    edge = np.flatnonzero(np.diff(np.concatenate([[0], ext])))
    starts = edge[ext[edge] != 0]
    nxt = edge[np.searchsorted(edge, starts, side="right")]
    found = len(starts)
    kept = min(found, max_records)
    return k[starts[:kept]], (nxt - starts)[:kept], (kept, found)


def match_image(pids, gids, cap_p, cap_g, nlabels, max_records, max_pairs, pstats=None, gstats=None, skip=None, iou=(1, 2)):
    """-> dict(n [4], pairs [kept, 3], pair_off [cap_p + 2], area [cap_p + cap_g + 2], match [cap_p, 3], gmatch [cap_g],
    pq int64 [nlabels + 1, 4]) of one image."""
    num, den = iou
    assert 1 <= num <= den <= 65535 and 2 * num >= den
    rk, rl, (rkept, rfound) = records(keys(pids, gids, cap_p, cap_g, skip), max_records)
    uk, inv = np.unique(rk, return_inverse=True)
    inter = np.bincount(inv.reshape(-1), weights=rl, minlength=len(uk)).astype(np.int64)
    pfound = len(uk)
    pkept = min(pfound, max_pairs)
    uk, inter = uk[:pkept], inter[:pkept]
    pp, gg = uk // (cap_g + 1), uk % (cap_g + 1)
    pairs = np.stack([pp, gg, inter], 1).astype(np.int32).reshape(-1, 3)
    pair_off = np.concatenate([[0], np.cumsum(np.bincount(pp, minlength=cap_p + 1)[:cap_p + 1])]).astype(np.int32)
    area_p = np.bincount(pp, weights=inter, minlength=cap_p + 1).astype(np.int64)
    area_g = np.bincount(gg, weights=inter, minlength=cap_g + 1).astype(np.int64)
    pcls, gcls = classes_of(pstats, cap_p), classes_of(gstats, cap_g)
    match = np.zeros((cap_p, 3), np.int32)
    gmatch = np.zeros(cap_g, np.int32)
    pq = [[0, 0, 0, 0] for _ in range(nlabels + 1)]
    for p, g, i in pairs.tolist():
        if p == 0 or g == 0:
            continue
        c = int(pcls[p - 1])
        if c != int(gcls[g - 1]) or not 1 <= c <= nlabels:
            continue
        union = int(area_p[p]) + int(area_g[g]) - i
        if i * den > num * union:
            assert match[p - 1, 0] == 0 and gmatch[g - 1] == 0, "a second partner"
            match[p - 1] = (g, i, union)
            gmatch[g - 1] = p
            pq[c][0] += 1
            pq[c][3] += (i << 32) // union
    for p in range(1, cap_p + 1):
        c = int(pcls[p - 1])
        if area_p[p] > 0 and match[p - 1, 0] == 0 and 1 <= c <= nlabels:
            pq[c][1] += 1
    for g in range(1, cap_g + 1):
        c = int(gcls[g - 1])
        if area_g[g] > 0 and gmatch[g - 1] == 0 and 1 <= c <= nlabels:
            pq[c][2] += 1
    return dict(n=np.array([pkept, pfound, rkept, rfound], np.int32), pairs=pairs, pair_off=pair_off,
                area=np.concatenate([area_p, area_g]).astype(np.int32), match=match, gmatch=gmatch, pq=np.array(pq, np.int64))


def match(pids, gids, cap_p, cap_g, nlabels, max_records, max_pairs, pstats=None, gstats=None, skip=None, iou=(1, 2)):
    """[B, H, W] maps -> the same dict with a leading batch axis; pairs is a list of [kept_b, 3]."""
    B = len(pids)
    per = [match_image(pids[b], gids[b], cap_p, cap_g, nlabels, max_records, max_pairs,
                       None if pstats is None else pstats[b], None if gstats is None else gstats[b],
                       None if skip is None else skip[b], iou) for b in range(B)]
    out = {k: np.stack([p[k] for p in per]) for k in ("n", "pair_off", "area", "match", "gmatch", "pq")}
    out["pairs"] = [p["pairs"] for p in per]
    return out


# ------------------------------------------------------------------------------------------------ independent loops

def pixel_pairs(pids, gids, cap_p, cap_g, skip=None):
    """{(p, g): pixels} by a loop over the pixels, (0, 0) left out."""
    out = {}
    H, W = len(pids), len(pids[0])
    for y in range(H):
        for x in range(W):
            if skip is not None and skip[y][x] == 255:
                continue
            p, g = pids[y][x], gids[y][x]
            p, g = (p if 1 <= p <= cap_p else 0), (g if 1 <= g <= cap_g else 0)
            if (p, g) != (0, 0):
                out[(p, g)] = out.get((p, g), 0) + 1
    return out


def brute_matches(pids, gids, cap_p, cap_g, pcls, gcls, nlabels, skip=None, iou=(1, 2)):
    """The matches from masks, object against object: [(p, g, inter, union)], with the uniqueness the rule promises
    asserted; and the (TP, FP, FN) lists per class."""
    num, den = iou
    pids, gids = np.asarray(pids), np.asarray(gids)
    keep = np.ones(pids.shape, bool) if skip is None else np.asarray(skip) != 255
    out, pseen, gseen = [], set(), set()
    for p in range(1, cap_p + 1):
        mp = (pids == p) & keep
        for g in range(1, cap_g + 1):
            mg = (gids == g) & keep
            i, u = int((mp & mg).sum()), int((mp | mg).sum())
            if i and pcls[p - 1] == gcls[g - 1] and 1 <= pcls[p - 1] <= nlabels and i * den > num * u:
                assert p not in pseen and g not in gseen, "the partner is not unique"
                pseen.add(p)
                gseen.add(g)
                out.append((p, g, i, u))
    counts = [[0, 0, 0] for _ in range(nlabels + 1)]
    for p, g, i, u in out:
        counts[pcls[p - 1]][0] += 1
    for p in range(1, cap_p + 1):
        if ((pids == p) & keep).any() and p not in pseen and 1 <= pcls[p - 1] <= nlabels:
            counts[pcls[p - 1]][1] += 1
    for g in range(1, cap_g + 1):
        if ((gids == g) & keep).any() and g not in gseen and 1 <= gcls[g - 1] <= nlabels:
            counts[gcls[g - 1]][2] += 1
    return out, counts


# ------------------------------------------------------------------------------------------------ maps to match

def blobs(H, W, rs, nlabels=3, count=None, radius=None):
    """A uint8 label map of random discs of classes 1..nlabels on background."""
    lab = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[:H, :W]
    count = max(2, H * W // 60) if count is None else count
    for _ in range(count):
        r = rs.randint(1, max(2, min(H, W) // 5) + 1) if radius is None else radius
        cy, cx = rs.randint(0, H), rs.randint(0, W)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rs.randint(1, nlabels + 1)
    return lab


def perturb(lab, rs, ignore=0.03):
    """A ground truth for `lab` ([H, W], or a stack of such maps): shifted by a pixel, a few pixels flipped to background
    or another class, some set to the ignore value 255."""
    gt = np.roll(lab, (rs.randint(-1, 2), rs.randint(-1, 2)), (-2, -1)).copy()
    flip = rs.rand(*lab.shape) < 0.05
    gt[flip] = rs.randint(0, 4, int(flip.sum()))
    gt[rs.rand(*lab.shape) < ignore] = 255
    return gt
