"""Python-integer reference of the simplified rings (the optional last stage of dfw_seg_contours), by the definition in
include/diffews_hip.h: Douglas-Peucker with a tolerance of tol4 quarter pixels on a closed ring of corners, all integers.

    measure(pa, pb, p)                 (m, line): |cross| against the line pa pb, or the squared distance when pa == pb
    keeps(pa, pb, m, tol4)             the strict test 16 m^2 > tol4^2 L (line mode) / 16 m > tol4^2 (point mode)
    simplify(pts, tol4, rule3=True)    the recursive definition -> the sorted ranks kept
    simplify_rounds(pts, tol4)         the level-synchronous form the device runs -> (ranks kept, rounds)
    expected(ids, cap, conn, max_edges, tol4)   what the device writes for a batch, on top of contours_ref.expected
"""
import numpy as np

import contours_ref as ct


def measure(pa, pb, p):
    ux, uy, vx, vy = pb[0] - pa[0], pb[1] - pa[1], p[0] - pa[0], p[1] - pa[1]
    if ux == 0 and uy == 0:
        return vx * vx + vy * vy, False
    return abs(ux * vy - uy * vx), True


def keeps(pa, pb, m, tol4):
    ux, uy = pb[0] - pa[0], pb[1] - pa[1]
    if ux == 0 and uy == 0:
        return 16 * m > tol4 * tol4
    return 16 * m * m > tol4 * tol4 * (ux * ux + uy * uy)


def _pts(pts):
    return [(int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2).tolist()]


def anchor(P):
    """Rule 1: the corner farthest from P[0], the lowest rank on ties."""
    return max(range(len(P)), key=lambda i: (measure(P[0], P[0], P[i])[0], -i))


def winner(P, a, b):
    """Rule 2: (w, m) of the chain (a, b), b - a >= 2; P[len(P)] means P[0]."""
    c = len(P)
    pa, pb = P[a], P[b % c]
    w = max(range(a + 1, b), key=lambda i: (measure(pa, pb, P[i])[0], -abs(2 * i - (a + b)), -i))
    return w, measure(pa, pb, P[w])[0]


def _rule3(P, f, kept, on=True):
    if len(kept) == 2 and on:
        kept.add(max((i for i in range(len(P)) if i not in (0, f)), key=lambda i: (measure(P[0], P[f], P[i])[0], -i)))
    return sorted(kept)


def simplify(pts, tol4, rule3=True):
    """The ranks kept, ascending.  rule3=False: rules 1 and 2 alone, which may leave the two anchors only."""
    P = _pts(pts)
    c = len(P)
    assert c >= 4
    f = anchor(P)
    kept = {0, f}
    stack = [(0, f), (f, c)]
    while stack:                                   # the recursion, with a list instead of Python's call stack
        a, b = stack.pop()
        if b - a < 2:
            continue
        w, m = winner(P, a, b)
        if keeps(P[a], P[b % c], m, tol4):
            kept.add(w)
            stack += [(a, w), (w, b)]
    return _rule3(P, f, kept, rule3)


def simplify_rounds(pts, tol4):
    """Every round all live chains pick their winner at once; a chain whose winner is kept splits in two for the next
    round, any other chain is finished.  Returns (ranks kept, rounds run: those with at least one live chain)."""
    P = _pts(pts)
    c = len(P)
    assert c >= 4
    f = anchor(P)
    kept = {0, f}
    live = [s for s in ((0, f), (f, c)) if s[1] - s[0] >= 2]
    rounds = 0
    while live:
        rounds += 1
        nxt = []
        for a, b in live:
            w, m = winner(P, a, b)
            if keeps(P[a], P[b % c], m, tol4):
                kept.add(w)
                nxt += [s for s in ((a, w), (w, b)) if s[1] - s[0] >= 2]
        live = nxt
    return _rule3(P, f, kept), rounds


def simplify_tables(e, tol4):
    """One image's entry of contours_ref.expected -> dict(n [4], rings [r, 4], verts [k, 2], ring_off, rounds)."""
    if not e["n"][3]:
        return dict(n=np.zeros(4, np.int64), rings=np.zeros((0, 4), np.int64), verts=np.zeros((0, 2), np.int64),
                    ring_off=e["ring_off"], rounds=0)
    rings, verts, at, rounds = [], [], 0, 0
    for i, first, count, area in e["rings"].tolist():
        pts = e["verts"][first:first + count]
        keep, r = simplify_rounds(pts, tol4)
        rounds = max(rounds, r)
        rings.append((i, at, len(keep), area))
        verts += pts[keep].tolist()
        at += len(keep)
    return dict(n=np.array([e["n"][1], at, len(rings), 1]), rings=np.array(rings, np.int64).reshape(-1, 4),
                verts=np.array(verts, np.int64).reshape(-1, 2), ring_off=e["ring_off"], rounds=rounds)


def expected(ids, cap, connectivity, max_edges, tol4, base=None):
    """ids [B, H, W] -> per image what the stage writes: simp_n = (corners in, corners kept, rings, complete), simp_rings,
    simp_verts; an image that is not complete has n = 0 and no row.  `base`: contours_ref.expected of the same arguments,
    when the caller has it already."""
    base = ct.expected(ids, cap, connectivity, max_edges) if base is None else base
    return [simplify_tables(e, tol4) for e in base]
