"""CPU tests of the outline stage: the reference tests/contours_ref.py against facts that do not depend on it (the masks,
the pixel counts, scipy's count of enclosed background components), the header's literal examples, the C ABI of
dfw_seg_contours -- header, ctypes mirror, sizeof, the workspace, block and rounds queries and every host-side refusal
(host pointers, null stream: nothing is launched) --, the host helpers of diffews_amd.objects, and the proof that every
sized case of tests/test_object_contours_gpu.py reaches the size it claims.  Every comparison is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as cr
import contours_cases as cc
import contours_ref as ct
from seg_args_cases import check_overlap_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ESHAPE, DFW_ERANGE, DFW_EWORKSPACE = -1, -2, -3, -4
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
EIGHT = np.ones((3, 3), int)


def _ids(lab, conn):
    return cr.components(lab[None], conn, 0, 1)["ids"][0]


def _enclosed(ndi, mask, conn):
    """Components of the complement of `mask` under the dual connectivity that do not reach the padded frame."""
    lab, n = ndi.label(np.pad(~mask, 1, constant_values=True), structure=FOUR if conn == 8 else EIGHT)
    return n - 1


# ------------------------------------------------------------------------------------------------ the reference

def _random_maps(count, seed):
    rs = np.random.RandomState(seed)
    for _ in range(count):
        H, W = rs.randint(1, 14), rs.randint(1, 14)
        yield ((rs.rand(H, W) < rs.choice([0.3, 0.5, 0.7])) * rs.randint(1, 3, (H, W))).astype(np.uint8)


def test_reference_against_independent_facts():
    ndi = pytest.importorskip("scipy.ndimage")
    for lab in _random_maps(300, 7):
        H, W = lab.shape
        for conn in (4, 8):
            ids = _ids(lab, conn)
            top = int(ids.max())
            t = ct.trace(ids, top + 2, conn)
            assert t["lengths"].sum() == t["nedges"] and t["ring_off"][0] == 0 and t["ring_off"][-1] == len(t["rings"])
            assert (t["rings"][:, 2] % 2 == 0).all() and (t["rings"][:, 2] >= 4).all()
            for k in range(1, top + 1):
                rings = ct.object_rings(t, k)
                mask = ids == k
                assert np.array_equal(ct.rasterise(rings, H, W), mask), (conn, k)
                assert sum(a for a, _ in rings) == mask.sum()
                assert rings[0][0] > 0 and all(a < 0 for a, _ in rings[1:])
                lo = t["ring_off"][k - 1]
                assert t["leaders"][lo] % 4 == 0 and (t["leaders"][lo + 1:t["ring_off"][k]] % 4 != 0).all()
                assert len(rings) - 1 == _enclosed(ndi, mask, conn), (conn, k)


def test_the_successor_is_a_bijection_on_any_map():
    """Also for ids that do not match the connectivity, negative ids and ids above cap."""
    rs = np.random.RandomState(11)
    for _ in range(300):
        H, W = rs.randint(1, 14), rs.randint(1, 14)
        ids = rs.randint(-2, 6, (H, W)).astype(np.int32)
        for conn in (4, 8):
            for cap in (1, 3, 9):
                keys = ct.edges(ids, cap)
                succ, _ = ct.successor(ids, cap, conn, keys)
                assert (succ >= 0).all() and len(np.unique(succ)) == len(keys)
                v = ct.values(ids, cap)
                assert (v.ravel()[keys >> 2] == v.ravel()[keys[succ] >> 2]).all()      # a ring belongs to one id
                t = ct.trace(ids, cap, conn)
                for k in range(1, cap + 1):
                    assert np.array_equal(ct.rasterise(ct.object_rings(t, k), H, W), v == k)


def test_literal_examples_of_the_header():
    t = ct.trace(np.array([[1, 1, 1, 1], [1, 0, 0, 1], [1, 1, 1, 1]]), 1, 8)
    assert t["nedges"] == 20 and t["rings"].tolist() == [[1, 0, 4, 12], [1, 4, 4, -2]] and t["ring_off"].tolist() == [0, 2]
    assert t["verts"].tolist() == [[0, 0], [4, 0], [4, 3], [0, 3], [1, 1], [1, 2], [3, 2], [3, 1]]
    assert t["leaders"][1] % 4 == 2                     # the hole's smallest key is the bottom of pixel (1, 0): its start,
    assert [3, 1] not in t["verts"][4:5].tolist()       # (2, 1), lies on a straight stretch and is no corner
    diamond = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]])
    t = ct.trace(diamond, 1, 8)
    assert t["nedges"] == 16 and t["rings"].tolist() == [[1, 0, 12, 5], [1, 12, 4, -1]]
    assert t["verts"][0].tolist() == [1, 0] and t["verts"][12:].tolist() == [[2, 1], [1, 1], [1, 2], [2, 2]]
    four = np.array([[0, 1, 0], [2, 0, 3], [0, 4, 0]])
    t = ct.trace(four, 4, 4)
    assert t["rings"].tolist() == [[k + 1, 4 * k, 4, 1] for k in range(4)] and t["ring_off"].tolist() == [0, 1, 2, 3, 4]
    assert t["verts"][:4].tolist() == [[1, 0], [2, 0], [2, 1], [1, 1]]
    # the device's answer to an overflow: nothing but the count
    e = ct.expected(diamond[None], 1, 8, 12)[0]
    assert e["n"].tolist() == [16, 0, 0, 0] and len(e["rings"]) == 0 and not e["ring_off"].any()


# ------------------------------------------------------------------------------------------------ the C ABI

def _fields(hdr, name):
    body = re.search(r"typedef struct \{([^{}]*)\}\s*" + name + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.replace("*", " ").replace(",", " ").split()
        names += [p for p in parts if p not in ("const", "void", "int32_t", "int64_t", "size_t", "uint8_t")]
    return names


def test_struct_mirror_and_sizeof(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    assert _fields(hdr, "dfw_seg_contours_args") == [f[0] for f in L.SegContoursArgs._fields_]
    assert _fields(hdr, "dfw_seg_contours_trips") == [f[0] for f in L.SegContoursTrips._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\n'
                   'int main(){printf("%zu %zu", sizeof(dfw_seg_contours_args), sizeof(dfw_seg_contours_trips));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [C.sizeof(L.SegContoursArgs), C.sizeof(L.SegContoursTrips)]
    i32 = C.c_int32
    assert L.SYMBOLS["dfw_seg_contours"] == (i32, [C.POINTER(L.SegContoursArgs), C.c_void_p])
    assert L.SYMBOLS["dfw_seg_contours_workspace_bytes"] == (C.c_size_t, [i32] * 5)
    assert L.SYMBOLS["dfw_seg_contours_block"] == (i32, [C.POINTER(i32), C.POINTER(i32)])
    assert L.SYMBOLS["dfw_seg_contours_rounds"] == (i32, [i32] * 5 + [C.POINTER(L.SegContoursTrips)])
    assert hip_lib.dfw_version() >= 121
    assert "seg_contours.hip" in __import__("diffews_amd.build", fromlist=["SOURCES"]).SOURCES


def test_workspace_query_is_zero_for_invalid_arguments_and_monotone(hip_lib):
    from diffews_amd import ops
    q = hip_lib.dfw_seg_contours_workspace_bytes
    P, E = cc.block(hip_lib)
    assert P >= 1 and E >= 1 and hip_lib.dfw_seg_contours_block(None, None) == DFW_EINVAL
    p = C.c_int32()
    assert hip_lib.dfw_seg_contours_block(C.byref(p), None) == DFW_EINVAL and hip_lib.dfw_seg_contours_block(None, C.byref(p)) == DFW_EINVAL
    sizes = [1, 2, 37, 64, 65]
    for B in (1, 3):
        for H in sizes:
            for W in sizes:
                for cap in (1, 255, 256, 65535, 65536, 1 << 24):
                    for M in (4, E - 4, E, E + 4, 4 * E + 8):
                        got = q(B, H, W, cap, M)
                        assert got == ops.seg_contours_workspace(B, H, W, cap, M)
                        assert got >= 4 * B * H * W + 64 * B * M and got % 4 == 0, (B, H, W, cap, M)
                        assert q(B + 1, H, W, cap, M) >= got and q(B, H + 1, W, cap, M) >= got
                        assert q(B, H, W + 1, cap, M) >= got and q(B, H, W, cap + 1, M) >= got and q(B, H, W, cap, M + 4) >= got
    assert q(2, 16384, 16384, 1024, 1 << 24) >= (2 << 30) + (2 << 30)     # no 32-bit arithmetic on the way
    for bad in ((0, 5, 5, 4, 8), (1, 0, 5, 4, 8), (1, 5, -1, 4, 8), (1, 5, 5, 0, 8), (1, 5, 5, 4, 0), (1, 5, 5, 4, 3),
                (1, 5, 5, 4, 6), (1, 5, 5, 4, -4)):
        assert q(*bad) == 0, bad


def test_rounds_query_and_its_error_order(hip_lib):
    from diffews_amd import _lib as L
    P, E = cc.block(hip_lib)
    out = L.SegContoursTrips()
    f = hip_lib.dfw_seg_contours_rounds
    assert f(1, 5, 5, 4, 8, None) == DFW_EINVAL
    assert f(0, 5, 5, 4, 8, C.byref(out)) == DFW_EINVAL and f(1, 5, 5, 4, 6, C.byref(out)) == DFW_EINVAL
    assert f(1, 5, 5, 0, 8, C.byref(out)) == DFW_EINVAL and f(1, 5, 5, 4, 0, C.byref(out)) == DFW_EINVAL
    assert f(1, 65536, 1, 4, 8, C.byref(out)) == DFW_ERANGE and f(65536, 5, 5, 4, 8, C.byref(out)) == DFW_ERANGE
    assert f(1, 32768, 16384, 4, 8, C.byref(out)) == DFW_ERANGE            # 4 * H * W = 2^31: a key would not fit
    assert f(1, 23170, 23170, 4, 8, C.byref(out)) == 0                    # 4 * 23170^2 < 2^31
    assert f(0, 65536, 5, 4, 8, C.byref(out)) == DFW_EINVAL                # a size below 1 wins over one out of range
    assert f(1, 5, 5, 4, 1 << 30, C.byref(out)) == DFW_ERANGE and f(1, 5, 5, 0x7fffffff, 8, C.byref(out)) == DFW_ERANGE
    for M, R in ((4, 2), (8, 3), (60, 6), (64, 6), (68, 7), (1 << 21, 21), ((1 << 21) + 4, 22)):
        t = cc.trips(hip_lib, 2, 70, 60, 300, M)
        assert t["doubling"] == R and 2 ** R >= M > 2 ** (R - 1), M
        assert t["passes"] == 2 and t["launches"] == 14 + 2 * R + 3 * 2
        assert t["blocks"] == -(-70 * 60 // P) and t["ring_blocks"] == -(-M // E)
        assert t["corners_scan"] == -(-(M // 4) // 1024) and t["offsets_scan"] == 1


def _valid(lib, B=2, H=5, W=7, cap=4, max_edges=8, connectivity=8):
    """A fully valid call on host memory (never launched: every test below breaks one thing)."""
    from diffews_amd import _lib as L
    ws_bytes = lib.dfw_seg_contours_workspace_bytes(B, H, W, cap, max_edges)
    assert ws_bytes > 0

    def aligned(words):
        raw = np.zeros(words + 4, np.int32)
        off = (-raw.ctypes.data % 16) // 4
        return raw, raw[off:off + words]
    raws, keep = [], {}
    for name, words in (("ids", B * H * W), ("verts", B * max_edges * 2), ("rings", B * max_edges), ("ring_off", B * (cap + 1)),
                        ("n", B * 4), ("ws", ws_bytes // 4)):
        raw, keep[name] = aligned(words)
        raws.append(raw)
    a = L.SegContoursArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.ws_bytes, a.B, a.H, a.W, a.cap, a.max_edges, a.connectivity = ws_bytes, B, H, W, cap, max_edges, connectivity
    return a, raws


def test_every_refusal_comes_from_the_host_before_any_launch(hip_lib):
    kept = []

    def broken(**kw):
        a, raws = _valid(hip_lib)
        kept.append(raws)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.dfw_seg_contours(C.byref(a), None)

    assert hip_lib.dfw_seg_contours(None, None) == DFW_EINVAL
    for field in ("ids", "verts", "rings", "ring_off", "n", "ws"):
        assert broken(**{field: None}) == DFW_EINVAL, field
    for field in ("B", "H", "W", "cap", "max_edges"):
        for v in (0, -1):
            assert broken(**{field: v}) == DFW_EINVAL, field
    for conn in (0, 6, -8, 16):
        assert broken(connectivity=conn) == DFW_EINVAL, conn
    for m in (1, 2, 3, 5, 6, 10):
        assert broken(max_edges=m) == DFW_EINVAL, m
    outs = ("verts", "rings", "ring_off", "n", "ws")
    for field in outs:                                                # an output on top of the input
        for shift in (0, 16 * 3, 4 * (2 * 5 * 7 - 1)):
            a, raws = _valid(hip_lib)
            setattr(a, field, a.ids + shift)
            assert hip_lib.dfw_seg_contours(C.byref(a), None) == DFW_EINVAL, (field, shift)
    for i, f in enumerate(outs):                                      # two outputs on top of each other
        for g in outs[i + 1:]:
            a, raws = _valid(hip_lib)
            setattr(a, f, getattr(a, g))
            assert hip_lib.dfw_seg_contours(C.byref(a), None) == DFW_EINVAL, (f, g)
    a, raws = _valid(hip_lib)
    a.ids = a.verts + 8                                               # the input inside an output
    assert hip_lib.dfw_seg_contours(C.byref(a), None) == DFW_EINVAL
    # DFW_ERANGE: the sizes are checked before the workspace, which could not be that large here
    assert broken(H=65536, W=1) == DFW_ERANGE and broken(H=1, W=65536) == DFW_ERANGE
    assert broken(H=32768, W=16384) == DFW_ERANGE                    # 4 * H * W = 2^31
    assert broken(B=65536) == DFW_ERANGE
    assert broken(max_edges=1 << 29) == DFW_ERANGE                   # B * max_edges * 2 = 2^31
    assert broken(cap=1 << 30) == DFW_ERANGE and broken(cap=0x7fffffff) == DFW_ERANGE
    # DFW_EWORKSPACE: one byte short; anything larger on the same workspace
    a, raws = _valid(hip_lib)
    a.ws_bytes -= 1
    assert hip_lib.dfw_seg_contours(C.byref(a), None) == DFW_EWORKSPACE
    assert broken(ws_bytes=0) == DFW_EWORKSPACE and broken(H=6) == DFW_EWORKSPACE and broken(B=3) == DFW_EWORKSPACE
    assert broken(max_edges=12) == DFW_EWORKSPACE
    # DFW_ESHAPE: records off their alignment
    for field, shift in (("ids", 2), ("ring_off", 2), ("verts", 4), ("rings", 8), ("n", 8), ("ws", 8), ("rings", 4), ("n", 4)):
        a, raws = _valid(hip_lib)
        setattr(a, field, getattr(a, field) + shift)
        assert hip_lib.dfw_seg_contours(C.byref(a), None) == DFW_ESHAPE, (field, shift)
    # the order of the house: a null pointer wins over a size out of range, that over the workspace, that over overlap
    assert broken(ids=None, H=65536) == DFW_EINVAL
    a, raws = _valid(hip_lib)
    a.H, a.ws_bytes = 70000, 0
    assert hip_lib.dfw_seg_contours(C.byref(a), None) == DFW_ERANGE
    a, raws = _valid(hip_lib)
    a.verts, a.ws_bytes = a.ids, 0
    assert hip_lib.dfw_seg_contours(C.byref(a), None) == DFW_EWORKSPACE
    assert all(not r.any() for raws in kept for r in raws)           # nothing was written by any of these
    # the buffer rule of the object stages: every output and the workspace against every input and each other
    check_overlap_rule(lambda a: hip_lib.dfw_seg_contours(C.byref(a), None), lambda: _valid(hip_lib), dict(ids=(4 * 2 * 5 * 7, 4)),
                       dict(verts=(2 * 8 * 8, 8), rings=(2 * 2 * 16, 16), ring_off=(2 * 5 * 4, 4), n=(2 * 16, 16),
                            ws=(hip_lib.dfw_seg_contours_workspace_bytes(2, 5, 7, 4, 8), 16)))
    assert hip_lib.dfw_version() >= 122


def test_ops_pass_the_allocation_scan():
    import test_launch_guard_cpu as scan
    seen = scan._allocating_functions(os.path.join(ROOT, "diffews_amd", "ops.py"))
    assert "seg_contours" not in seen and "seg_contours_workspace" not in seen
    scan.test_every_allocation_of_the_wrappers_is_reachable_and_declared()


def test_wrappers_refuse_wrong_arguments_without_a_device(hip_lib):
    from diffews_amd import objects
    with pytest.raises(ValueError):
        objects.object_contours(np.zeros((5, 7), np.int32))          # an id map without max_components
    with pytest.raises(ValueError):
        objects.object_contours(np.zeros((5, 7), np.int32), max_components=4, connectivity=6)
    with pytest.raises(ValueError):
        objects.ContourBuffers(1, 5, 7, max_components=0, device="cpu")
    with pytest.raises(ValueError):
        objects.ContourBuffers(1, 5, 7, max_edges=10, device="cpu")
    b = objects.ContourBuffers(2, 5, 7, 3, device="cpu")
    assert b.max_edges == 4096 and b.verts.shape == (2, 4096, 2) and b.rings.shape == (2, 1024, 4)
    assert b.ring_off.shape == (2, 4) and b.n.shape == (2, 4) and b.ws.numel() == hip_lib.dfw_seg_contours_workspace_bytes(2, 5, 7, 3, 4096)
    assert objects.ContourBuffers(1, 300, 301, device="cpu").max_edges == 300 * 301 // 8 // 4 * 4


# ------------------------------------------------------------------------------------------------ the host helpers

def _tables(ids, cap, conn, max_edges):
    """The device's buffers for a batch, from the reference, as torch tensors on the host; rows behind the kept ones
    hold -7."""
    import torch
    exp = ct.expected(ids, cap, conn, max_edges)
    B = len(exp)
    verts, rings = np.full((B, max_edges, 2), -7, np.int32), np.full((B, max_edges // 4, 4), -7, np.int32)
    for b, e in enumerate(exp):
        verts[b, :len(e["verts"])], rings[b, :len(e["rings"])] = e["verts"], e["rings"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))  # noqa: E731
    return dict(verts=t(verts), rings=t(rings), ring_off=t(np.stack([e["ring_off"] for e in exp])), n=t(np.stack([e["n"] for e in exp])),
                shape=ids.shape[1:], connectivity=conn)


def test_contours_to_host_and_the_converters():
    from diffews_amd.objects import contours_to_host, rings_to_coco, rings_to_geojson, rings_to_mask
    rs = np.random.RandomState(3)
    lab = ((rs.rand(2, 12, 13) < 0.6) * rs.randint(1, 3, (2, 12, 13))).astype(np.uint8)
    lab[1, 3:9, 3:9], lab[1, 5:7, 5:7] = 1, 0                                   # a hole for certain
    ids = np.stack([_ids(l, 8) for l in lab])
    cap = int(ids.max()) + 2
    c = _tables(ids, cap, 8, 1024)
    host, incomplete = contours_to_host(c)
    assert not incomplete and len(host) == 2
    for b in range(2):
        assert len(host[b]) == ids[b].max()
        for k, rings in enumerate(host[b], 1):
            assert np.array_equal(rings_to_mask(rings, 12, 13), ids[b] == k)
            assert sum(a for a, _ in rings) == (ids[b] == k).sum()
            g = rings_to_geojson(rings)
            assert g["type"] == "Polygon" and len(g["coordinates"]) == len(rings)
            for (area, pts), closed in zip(rings, g["coordinates"]):
                assert closed[0] == closed[-1] and closed[:-1] == pts.tolist() and pts.dtype == np.int32
                shoelace = sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(closed, closed[1:]))
                assert shoelace == 2 * area                                    # y down: clockwise on screen is positive
            assert rings_to_coco(rings) == [v for xy in rings[0][1].tolist() for v in xy]
    assert any(len(r) > 1 for r in host[1])
    assert rings_to_coco([]) == []
    # one image of a [H, W] result; an image that is not complete has an empty list
    one, incomplete = contours_to_host({k: (v[0] if k in ("verts", "rings", "ring_off", "n") else v) for k, v in c.items()})
    assert not incomplete and all(np.array_equal(p, q) for r0, r1 in zip(one, host[0]) for (_, p), (_, q) in zip(r0, r1))
    found = [len(ct.edges(i, cap)) for i in ids]
    small = cc.up4(min(found)) if min(found) != max(found) else None
    assert small is not None and small < max(found)
    host2, incomplete = contours_to_host(_tables(ids, cap, 8, small))
    lo, hi = int(np.argmin(found)), int(np.argmax(found))
    assert incomplete and host2[hi] == [] and len(host2[lo]) == len(host[lo])
    # a list result
    many, incomplete = contours_to_host({k: [v[0], v[1]] if k in ("verts", "rings", "ring_off", "n") else [v, v] for k, v in c.items()})
    assert not incomplete and len(many) == 2 and len(many[1]) == len(host[1])


# ------------------------------------------------------------------------------------------------ the sizes of the GPU cases

def test_every_sized_gpu_case_reaches_its_size(hip_lib):
    P, E = cc.block(hip_lib)
    # one long ring: lengths around 64 and around 2 E, each needing one doubling round more than the length below
    rings = cc.long_rings(hip_lib)
    for name, (ids, length) in rings.items():
        t = ct.trace(ids, 1, 8)
        assert t["nedges"] == length and t["lengths"].tolist() == [length], name
        r = cc.trips(hip_lib, 1, *ids.shape, 1, cc.up4(length))["doubling"]
        assert 2 ** r >= length > 2 ** (r - 1) - 4, name
    assert ct.trace(cc.serpentine(), 1, 4)["lengths"].tolist() == [528] and cc.serpentine().shape == (15, 32)
    d = {n: cc.trips(hip_lib, 1, *rings[n][0].shape, 1, cc.up4(rings[n][1]))["doubling"] for n in rings}
    assert d["row30"] == d["row31"] == 6 and d["row32"] == 7
    assert d[f"row{E - 2}"] == d[f"row{E - 1}"] and d[f"row{E}"] == d[f"row{E - 1}"] + 1 and 2 ** d[f"row{E - 1}"] == 2 * E
    assert rings["row-above-block"][1] > E
    # sort passes
    for H, W, cap, passes in cc.SORT_CASES:
        n = int(cc.checkerboard(H, W).max())
        assert n <= cap and cc.trips(hip_lib, 1, H, W, cap, 4 * n)["passes"] == passes
    assert cc.SORT_CASES[-1][:2] == (512, 512) and int(cc.checkerboard(512, 512).max()) == 131072
    # second trips: the case goes round twice, and one step less in the argument that drives it does not
    for name, case in cc.second_trip_cases(hip_lib).items():
        H, W = case["ids"].shape
        f = case["field"]
        assert cc.trips(hip_lib, 2, H, W, case["cap"], case["max_edges"])[f] == 2, name
        less = dict(block_scan=(H - 1 if H > 1 else H, W if H > 1 else W - 1, case["cap"], case["max_edges"]),
                    offsets_scan=(H, W, case["cap"] - 1, case["max_edges"])).get(f, (H, W, case["cap"], case["max_edges"] - 4))
        assert cc.trips(hip_lib, 2, *less)[f] == 1, name
        found = len(ct.edges(case["ids"], case["cap"]))
        assert found <= case["max_edges"], name
        if f != "ring_scan":
            assert {"block_scan": (np.nonzero(case["ids"].ravel())[0].max() >= 1024 * P),
                    "table_scan": found == case["max_edges"], "offsets_scan": int(case["ids"].max()) == case["cap"] == 1024,
                    "corners_scan": found // 4 == 1025}[f], name
    # a map of the random family crosses a block of pixels and a block of edges
    assert 3 * P < 75 * (3 * P // 75 + 2) < 4 * P
