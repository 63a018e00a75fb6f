"""CPU tests of the simplified rings (the optional last stage of dfw_seg_contours): the two forms of tests/simplify_ref.py
against each other and against properties that do not depend on either; the bounds of the header over the size limits; the
C ABI -- struct fields, sizeof, the new query, the version --; every host-side refusal of the new arguments (host pointers,
null stream: nothing is launched, nothing written); and the tolerance rule of diffews_amd.objects.  All exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import components_ref as cr
import contours_cases as cc
import contours_ref as ct
import simplify_ref as sr
import test_object_contours_cpu as tcc
from seg_args_cases import check_overlap_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ESHAPE, DFW_ERANGE, DFW_EWORKSPACE = -1, -2, -3, -4
TOLS = (0, 2, 4, 6, 8, 16, 40)


def square(n):
    return np.ones((n, n), np.int32)


def plus(arm=3):
    a = np.zeros((3 * arm, 3 * arm), np.int32)
    a[arm:2 * arm], a[:, arm:2 * arm] = 1, 1
    return a


def staircase(n):
    """The lower left triangle of n x n: one ring of 2 n + 2 corners, a perfect 45 degree staircase."""
    return np.tril(np.ones((n, n), np.int32))


def diagonal_squares():
    a = np.zeros((6, 6), np.int32)
    a[:3, :3], a[3:, 3:] = 1, 1
    return a


def _rings(ids, cap, conn):
    t = ct.trace(ids, cap, conn)
    return [t["verts"][f:f + c] for _, f, c, _ in t["rings"].tolist()]


def _blob_rings():
    rs = np.random.RandomState(23)
    for k in range(6):
        lab = cc.blobs(70 + 7 * k, 90 - 5 * k, rs, n=25)
        for conn in (4, 8):
            ids = cr.components(lab[None], conn, 0, 1)["ids"][0]
            yield from _rings(ids, int(ids.max()), conn)


# ------------------------------------------------------------------------------------------------ the reference

def test_recursive_and_level_synchronous_forms_agree_and_hold_the_properties():
    corners = 0
    for pts in _blob_rings():
        corners += len(pts)
        P = [tuple(p) for p in pts.tolist()]
        c = len(P)
        for tol4 in TOLS:
            keep = sr.simplify(pts, tol4)
            lvl, rounds = sr.simplify_rounds(pts, tol4)
            assert keep == lvl and rounds <= max(c - 2, 0)
            assert keep[0] == 0 and len(keep) >= 3 and keep == sorted(set(keep))
            if tol4 == 0:
                assert keep == list(range(c))
            two = sr.simplify(pts, tol4, rule3=False)                    # rules 1 and 2: the chains between kept corners
            f = sr.anchor(P)
            if len(two) == 2:                                            # rule 3 adds the corner farthest from P[0] P[f]
                g, = set(keep) - set(two)
                assert two == [0, f] and sr.measure(P[0], P[f], P[g])[0] == max(sr.measure(P[0], P[f], p)[0] for p in P) > 0
            else:
                assert two == keep
            for a, b in zip(two, two[1:] + [c]):
                for i in range(a + 1, b):
                    m, _ = sr.measure(P[a], P[b % c], P[i])
                    assert not sr.keeps(P[a], P[b % c], m, tol4), (tol4, a, b, i)
    assert corners > 4000


def test_named_cases_of_the_reference():
    diamond, = _rings(np.array([[1, 0], [0, 1]]), 1, 8)
    assert diamond.tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]
    assert sr.simplify(diamond, 4) == [0, 1, 4] and sr.simplify_rounds(diamond, 4) == ([0, 1, 4], 1)      # rule 3
    assert sr.simplify(diamond, 0) == list(range(8))
    one, = _rings(np.ones((1, 1), int), 1, 8)
    for tol4 in (0, 4, 32768):
        assert sr.simplify(one, tol4) in ([0, 1, 2, 3], [0, 1, 2]) and sr.simplify(one, tol4)[:3] == [0, 1, 2]
    assert sr.simplify(one, 0) == [0, 1, 2, 3] and sr.simplify(one, 32768) == [0, 1, 2]
    # a square: the opposite corner is the anchor and each chain holds one corner.  The plus sign has ties in the measure
    sq, = _rings(square(5), 1, 8)
    assert sr.anchor([tuple(p) for p in sq.tolist()]) == 2 and sr.simplify(sq, 8) == [0, 1, 2, 3]
    assert sr.simplify(sq, 32768) == [0, 1, 2]                                                        # rule 3, lowest rank
    pl, = _rings(plus(), 1, 8)
    P = [tuple(p) for p in pl.tolist()]
    f = sr.anchor(P)
    ties = [sr.measure(P[0], P[f], P[i])[0] for i in range(1, f)]
    assert len(pl) == 12 and ties.count(max(ties)) >= 1
    for tol4 in (0, 4, 12, 40):
        assert sr.simplify(pl, tol4) == sr.simplify_rounds(pl, tol4)[0]
    # two 3 x 3 squares touching diagonally: the ring passes (3, 3) twice; a chain between the two visits is in point mode
    ds, = _rings(diagonal_squares(), 1, 8)
    P = [tuple(p) for p in ds.tolist()]
    assert P.count((3, 3)) == 2
    assert sr.simplify(ds, 2) == sr.simplify_rounds(ds, 2)[0] and len(sr.simplify(ds, 2)) == len(P)
    # the unit staircase at half a pixel: the middle rule splits it in the middle, few rounds for many corners
    st, = _rings(staircase(40), 1, 8)
    keep, rounds = sr.simplify_rounds(st, 2)
    assert len(st) == 82 and keep == sr.simplify(st, 2) and rounds <= 12
    assert len(sr.simplify(st, 4)) == 3 and sr.simplify(st, 3) != sr.simplify(st, 2)


def test_the_middle_rule_and_the_tie_order():
    """Three interior corners at one distance from the anchors' line: the middle one wins; of two at equal distance from
    the middle the lower rank."""
    P = [(0, 0), (1, 2), (2, 2), (3, 2), (4, 0), (2, -5)]                    # chain (0, 4): ranks 1, 2, 3 tie at m = 8
    assert sr.anchor(P) == 5
    assert [sr.measure(P[0], P[4], P[i])[0] for i in (1, 2, 3)] == [8, 8, 8] and sr.winner(P, 0, 4) == (2, 8)
    Q = [(0, 0), (1, 2), (2, 1), (3, 1), (4, 2), (5, 0), (2, -9)]            # ranks 1 and 4 tie, equally far from the middle
    assert sr.winner(Q, 0, 5)[0] == 1
    assert sr.measure((3, 3), (3, 3), (5, 4)) == (5, False) and sr.keeps((3, 3), (3, 3), 1, 4) is False
    assert sr.keeps((3, 3), (3, 3), 2, 4) is True                           # 16 * 2 > 16, strictly
    assert sr.keeps((0, 0), (4, 0), 4, 4) is False and sr.keeps((0, 0), (4, 0), 5, 4) is True      # exactly one pixel: dropped


def test_bounds_over_the_size_limits():
    """The header's bounds, in Python integers: whatever H and W the stage accepts, every product fits 64 unsigned bits and
    the packed key's two parts do not meet."""
    for H, W in ((65535, 8192), (8192, 65535), (23170, 23170), (1, 65535), (65535, 1)):
        assert 4 * H * W <= 2 ** 31 - 1
        worst = 0
        for pa, pb, p in (((0, 0), (W, H), (W, 0)), ((0, H), (W, 0), (0, 0)), ((0, 0), (W, H), (0, H))):
            m, line = sr.measure(pa, pb, p)
            assert line and m <= 2 * H * W < 2 ** 30
            worst = max(worst, m)
        assert worst == H * W and 16 * (2 * H * W) ** 2 < 2 ** 64
        L = W * W + H * H
        assert L <= 2 * 65535 ** 2 < 2 ** 33 and 32768 ** 2 * L < 2 ** 63
        pm, line = sr.measure((0, 0), (0, 0), (W, H))
        assert not line and pm == L and 16 * pm < 2 ** 64 and pm < 2 ** 33
    # the key: m << 31 with m < 2^33, and a low part 2^31 - 1 - t with 0 <= t < 2^31 - 1 for every chain of a ring whose
    # corners are rows of verts, fewer than 2^30 (B * max_edges * 2 <= 2^31 - 1)
    c = (2 ** 31 - 1) // 2
    t = 2 * (c - 2) + 1
    assert 0 < 2 ** 31 - 1 - t < 2 ** 31 and (2 * 65535 ** 2 << 31) + 2 ** 31 - 1 < 2 ** 64


# ------------------------------------------------------------------------------------------------ the C ABI

def test_struct_symbol_and_version(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    fields = tcc._fields(hdr, "dfw_seg_contours_args")
    assert fields[-4:] == ["simp_verts", "simp_rings", "simp_n", "tol4"] and fields == [f[0] for f in L.SegContoursArgs._fields_]
    trips = tcc._fields(hdr, "dfw_seg_contours_trips")
    assert trips[-2:] == ["launches", "simplify_launches"] and trips == [f[0] for f in L.SegContoursTrips._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "diffews_hip.h"\n'
                   'int main(){printf("%zu %zu %zu %zu", sizeof(dfw_seg_contours_args), sizeof(dfw_seg_contours_trips),'
                   'offsetof(dfw_seg_contours_args, simp_verts), offsetof(dfw_seg_contours_args, tol4));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    A = L.SegContoursArgs
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [C.sizeof(A), C.sizeof(L.SegContoursTrips),
                                                                            A.simp_verts.offset, A.tol4.offset]
    assert L.SYMBOLS["dfw_seg_contours_simplify_block"] == (C.c_int32, [C.POINTER(C.c_int32)])
    assert hip_lib.dfw_version() >= 123
    v = C.c_int32()
    assert hip_lib.dfw_seg_contours_simplify_block(None) == DFW_EINVAL
    assert hip_lib.dfw_seg_contours_simplify_block(C.byref(v)) == 0 and v.value >= 256 and v.value % 2 == 0
    from diffews_amd import ops
    assert ops.seg_contours_simplify_block() == v.value


def test_workspace_is_what_it_was_and_the_extra_launches_are_fixed(hip_lib):
    """The state of the stage lives in 12 of the 16 words per edge the workspace always had in front: the query's value is
    the sum of the parts the header lists, as before, and simplify_launches does not depend on the arguments."""
    P, E = cc.block(hip_lib)
    for B, H, W, cap, M in ((1, 1, 1, 1, 4), (2, 5, 7, 4, 8), (3, 70, 60, 300, 4096), (1, 512, 512, 131072, 1 << 19), (2, 64, 65, 1 << 24, E + 4)):
        t = cc.trips(hip_lib, B, H, W, cap, M)
        assert t["simplify_launches"] == 3 and t["launches"] == 14 + 2 * t["doubling"] + 3 * t["passes"]
        Q = M // 4
        words = B * (16 * M + 6 + H * W + t["blocks"] + t["ring_blocks"] + 5 * Q + 256 * -(-Q // 2048))
        assert hip_lib.dfw_seg_contours_workspace_bytes(B, H, W, cap, M) == 4 * words, (B, H, W, cap, M)
        assert 6 * M + Q + 2 <= 12 * M                                     # the stage's words per image, inside state and lead


def _valid(lib, tol4=4, **kw):
    """tests/test_object_contours_cpu.py's valid call with the three new outputs on host memory of their own."""
    a, raws = tcc._valid(lib, **kw)
    B, E = a.B, a.max_edges
    keep = {}
    for name, words in (("simp_verts", B * E * 2), ("simp_rings", B * E), ("simp_n", B * 4)):
        raw = np.zeros(words + 4, np.int32)
        off = (-raw.ctypes.data % 16) // 4
        keep[name] = raw[off:off + words]
        raws.append(raw)
        setattr(a, name, keep[name].ctypes.data)
    a.tol4 = tol4
    return a, raws


def test_every_refusal_of_the_new_arguments_comes_before_any_launch(hip_lib):
    kept = []
    call = lambda a: hip_lib.dfw_seg_contours(C.byref(a), None)   # noqa: E731

    def broken(**kw):
        a, raws = _valid(hip_lib)
        kept.append(raws)
        for k, v in kw.items():
            setattr(a, k, v)
        return call(a)

    new = ("simp_verts", "simp_rings", "simp_n")
    for i in range(1, 7):                                              # partial pointer sets: one or two of the three
        gone = {f: None for k, f in enumerate(new) if i >> k & 1}
        assert broken(**gone) == DFW_EINVAL, gone
    for tol4 in (-1, 32769, -32768, 1 << 30):
        assert broken(tol4=tol4) == DFW_EINVAL, tol4
    for tol4 in (1, 4, 32768, -1):                                     # the stage off and a tolerance
        assert broken(simp_verts=None, simp_rings=None, simp_n=None, tol4=tol4) == DFW_EINVAL, tol4
    # they belong to the pointers and scalars: before the sizes and the workspace, behind nothing but a null of the old ones
    assert broken(tol4=-1, H=65536) == DFW_EINVAL and broken(simp_n=None, ws_bytes=0) == DFW_EINVAL
    assert broken(tol4=32769, max_edges=1 << 29) == DFW_EINVAL
    assert broken(ids=None, tol4=-1, H=65536) == DFW_EINVAL and broken(ids=None) == DFW_EINVAL
    assert broken(H=65536, W=1) == DFW_ERANGE and broken(ws_bytes=0) == DFW_EWORKSPACE                # the old order stays
    a, raws = _valid(hip_lib)
    kept.append(raws)
    a.simp_verts, a.ws_bytes = a.ids, 0
    assert call(a) == DFW_EWORKSPACE                                   # the workspace before overlap
    # each new output on ids, verts, rings, n, ring_off, ws and on each other
    old = ("ids", "verts", "rings", "ring_off", "n", "ws")
    for f in new:
        for g in old + tuple(x for x in new if x != f):
            a, raws = _valid(hip_lib)
            kept.append(raws)
            setattr(a, f, getattr(a, g))
            assert call(a) == DFW_EINVAL, (f, g)
    # off their alignment
    for f, shift in (("simp_verts", 4), ("simp_rings", 8), ("simp_rings", 4), ("simp_n", 8), ("simp_n", 4)):
        a, raws = _valid(hip_lib)
        kept.append(raws)
        setattr(a, f, getattr(a, f) + shift)
        assert call(a) == DFW_ESHAPE, (f, shift)
    a, raws = _valid(hip_lib)
    kept.append(raws)
    a.simp_verts += 8                                                  # 8 bytes are enough for rows of 8
    a.simp_n += 4
    assert call(a) == DFW_ESHAPE
    assert all(not r.any() for raws in kept for r in raws)             # nothing was written by any of these
    ws = hip_lib.dfw_seg_contours_workspace_bytes(2, 5, 7, 4, 8)
    check_overlap_rule(call, lambda: _valid(hip_lib), dict(ids=(4 * 2 * 5 * 7, 4)),
                       dict(verts=(2 * 8 * 8, 8), rings=(2 * 2 * 16, 16), ring_off=(2 * 5 * 4, 4), n=(2 * 16, 16),
                            simp_verts=(2 * 8 * 8, 8), simp_rings=(2 * 2 * 16, 16), simp_n=(2 * 16, 16), ws=(ws, 16)))


# ------------------------------------------------------------------------------------------------ the Python layer

def test_tolerance_rule_and_buffers_without_a_device(hip_lib):
    import torch

    from diffews_amd import objects, ops
    ids = np.zeros((5, 7), np.int32)
    for bad in (-0.25, 0.1, 0.3, 8192.25, 1e9, float("nan"), "1", True, [1.0]):
        with pytest.raises(ValueError, match="multiple of 0.25 pixels in 0..8192"):
            objects.object_contours(ids, max_components=4, tolerance=bad)
    for good, tol4 in ((0, 0), (0.25, 1), (1, 4), (1.5, 6), (8192, 32768), (2.0, 8)):
        assert objects._tol4(good) == tol4
    assert objects._tol4(None) is None
    b = objects.ContourBuffers(2, 5, 7, 3, device="cpu")
    assert not b.simplify and b.simp_verts is None and b.simp_rings is None and b.simp_n is None
    s = objects.ContourBuffers(2, 5, 7, 3, device="cpu", simplify=True)
    assert s.simplify and s.simp_verts.shape == s.verts.shape and s.simp_rings.shape == s.rings.shape and s.simp_n.shape == (2, 4)
    assert s.simp_verts.dtype == torch.int32 and s.ws.numel() == b.ws.numel()
    assert s.simp_verts.data_ptr() != s.verts.data_ptr()
    assert "rectilinear" in objects.rings_to_mask.__doc__.lower() and "simplified" in objects.contours_to_host.__doc__
    import inspect
    sig = inspect.signature(ops.seg_contours).parameters
    assert [sig[k].default for k in ("simp_verts", "simp_rings", "simp_n", "tol4")] == [None, None, None, 0]
    assert inspect.signature(objects.object_contours).parameters["tolerance"].default is None


def test_ops_still_pass_the_allocation_scan():
    import test_launch_guard_cpu as scan
    seen = scan._allocating_functions(os.path.join(ROOT, "diffews_amd", "ops.py"))
    assert "seg_contours" not in seen and "seg_contours_simplify_block" not in seen
    scan.test_every_allocation_of_the_wrappers_is_reachable_and_declared()


def test_host_helpers_take_the_simplified_form():
    """contours_to_host, rings_to_geojson and rings_to_coco on the reference's simplified tables (host tensors)."""
    import torch

    from diffews_amd import objects
    rs = np.random.RandomState(3)
    lab = np.stack([cc.blobs(40, 50, rs, n=12), cc.blobs(40, 50, rs, n=9)])
    ids = cr.components(lab, 8, 0, 1)["ids"]
    cap, E = int(ids.max()) + 1, 4096
    base = ct.expected(ids, cap, 8, E)
    simp = sr.expected(ids, cap, 8, E, 4, base=base)
    verts, rings = np.full((2, E, 2), -7, np.int32), np.full((2, E // 4, 4), -7, np.int32)
    for b, e in enumerate(simp):
        verts[b, :len(e["verts"])], rings[b, :len(e["rings"])] = e["verts"], e["rings"]
    c = dict(verts=torch.from_numpy(verts), rings=torch.from_numpy(rings), n=torch.from_numpy(np.stack([e["n"] for e in simp]).astype(np.int32)),
             ring_off=torch.from_numpy(np.stack([e["ring_off"] for e in simp]).astype(np.int32)), shape=(40, 50), connectivity=8, tolerance=1.0)
    host, incomplete = objects.contours_to_host(c)
    assert not incomplete
    for b in range(2):
        assert len(host[b]) == int(ids[b].max())
        assert sum(len(p) for o in host[b] for _, p in o) == simp[b]["n"][1] < base[b]["n"][1]
        for k, o in enumerate(host[b], 1):
            assert sum(a for a, _ in o) == (ids[b] == k).sum()                  # the original rings' areas
            g = objects.rings_to_geojson(o)
            assert all(r[0] == r[-1] and len(r) >= 4 for r in g["coordinates"])
            assert len(objects.rings_to_coco(o)) == 2 * len(o[0][1]) >= 6
