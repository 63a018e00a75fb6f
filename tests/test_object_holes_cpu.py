"""CPU tests of the hole-filling stage: tests/holes_ref.py against a per-pixel search that states the definition, the four
properties the definition promises (objects keep label, box and first pixel; re-labelling the filled map gives the filled
ids; the stage is idempotent; a one-class map at connectivity 8 equals scipy's binary_fill_holes whenever every enclosed
region was filled), the C ABI of dfw_seg_holes (struct mirror, sizeof, signatures, the workspace query, every refusal in its
documented order on host memory -- validation precedes any launch), and the ValueErrors of the objects layer.  All
integers: every comparison is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import components_ref as cr
import holes_ref as hr
from seg_args_cases import check_overlap_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ESHAPE, DFW_ERANGE, DFW_EWORKSPACE = -1, -2, -3, -4
AREAS = (1, 3, None)


# ------------------------------------------------------------------------------------------------ the reference

def _random_maps(seed, count):
    """Maps of up to 13 x 13 pixels with 1 or 2 classes at densities 0.5, 0.7 and 0.85, as the definition was tried on."""
    rs = np.random.RandomState(seed)
    for trial in range(count):
        H, W = rs.randint(1, 14), rs.randint(1, 14)
        density, classes = (0.5, 0.7, 0.85)[trial % 3], 1 + (trial // 3) % 2
        yield ((rs.rand(H, W) < density) * rs.randint(1, classes + 1, (H, W))).astype(np.uint8), classes


def _objects(lab, conn, min_area=0, cap=64):
    ids, filtered, n, stats = cr.components_image(lab, conn, min_area, cap)
    return ids, filtered, n, stats


def test_reference_equals_the_pixel_search():
    enclosed = filled = 0
    for lab, _ in _random_maps(1, 120):
        for conn in (4, 8):
            ids, filtered, _, _ = _objects(lab, conn)
            for max_area in AREAS:
                got = hr.holes_image(filtered, ids, conn, max_area)
                want = hr.holes_search(filtered, ids, conn, max_area)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (lab.tolist(), conn, max_area)
                assert got[2] == want[2] and got[3] == want[3], (lab.tolist(), conn, max_area)
                enclosed += got[2][1]
                filled += got[2][0]
    assert enclosed > 300 and 100 < filled < enclosed                     # the maps do have holes, of both kinds


# Two 4-connected objects of class 1 that touch diagonally twice around a hole.  Under the dual connectivity 8 a diagonal
# touch with background on both other corners is a leak, so one corner of each touch carries a pixel of class 2.
SAME_CLASS = np.array([[0, 0, 0, 0, 0, 0, 0],
                       [0, 1, 1, 1, 2, 0, 0],
                       [0, 1, 0, 0, 1, 0, 0],
                       [0, 2, 1, 1, 1, 0, 0],
                       [0, 0, 0, 0, 0, 0, 0]], np.uint8)


def test_hand_made_maps():
    ring = np.ones((5, 5), np.uint8) * 3
    ring[2, 2] = 0
    ids = (ring > 0).astype(np.int32)
    io, lo, h, f = hr.holes_search(ring, ids, 8)
    assert (lo == 3).all() and (io == 1).all() and h == (1, 1) and f == {1: 1}
    assert hr.holes_search(ring, ids, 8, 0)[2] == (0, 1)
    # a diagonal gap: closed for 8-connected objects (the hole joins over 4), a leak for 4-connected ones (it joins over 8)
    leak = np.ones((5, 5), np.uint8)
    leak[2, 2] = leak[3, 3] = leak[4, 4] = 0
    i4, i8 = cr.components_image(leak, 4)[0], cr.components_image(leak, 8)[0]
    assert hr.holes_search(leak, i8, 8)[2] == (2, 2) and hr.holes_search(leak, i4, 4)[2] == (0, 0)
    # two owners, of two classes and of one class (4-connected objects touching diagonally): left alone
    two = np.array([[1, 1, 1, 2, 2], [1, 0, 0, 0, 2], [1, 1, 2, 2, 2]], np.uint8)
    assert hr.holes_search(two, cr.components_image(two, 8)[0], 8)[2] == (0, 1)
    ids = cr.components_image(SAME_CLASS, 4)[0]
    assert ids.max() == 4 and ids[1, 1] == 1 and ids[3, 4] == 3 and SAME_CLASS[1, 1] == SAME_CLASS[3, 4]
    assert hr.holes_search(SAME_CLASS, ids, 4)[2] == (0, 1) and hr.holes_image(SAME_CLASS, ids, 4)[2] == (0, 1)
    # an island inside a hole: the hole touches the island, so it stays; min_area removes the island first
    isl = np.ones((7, 7), np.uint8)
    isl[1:6, 1:6] = 0
    isl[3, 3] = 2
    ids = cr.components_image(isl, 8)[0]
    io, lo, h, _ = hr.holes_search(isl, ids, 8)
    assert h == (0, 1) and np.array_equal(lo, isl)
    ids, filtered, _, _ = cr.components_image(isl, 8, min_area=2)
    io, lo, h, f = hr.holes_search(filtered, ids, 8)
    assert h == (1, 1) and (lo == 1).all() and f == {1: 25}
    # owner 0: labels that the id map does not cover
    assert hr.holes_search(ring, np.zeros((5, 5), np.int32), 8)[2] == (0, 1)


def test_the_four_properties():
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    checked = 0
    for lab, classes in _random_maps(7, 90):
        for conn in (4, 8):
            cap = 200
            ids, filtered, n, stats = _objects(lab, conn, cap=cap)
            for max_area in AREAS:
                io, lo, h, f = hr.holes_image(filtered, ids, conn, max_area)
                so = hr.stats_image(stats, f)
                # 1: label, box and first pixel stay, the area only grows
                assert np.array_equal(so[:, [0, 2, 3, 4, 5, 6]], stats[:, [0, 2, 3, 4, 5, 6]])
                assert (so[:, 1] >= stats[:, 1]).all() and np.array_equal(so[:, 1] - stats[:, 1], so[:, 7])
                assert so[:, 7].sum() == (io != ids).sum() == sum(f.values())
                # 2: re-labelling the filled labels gives the filled ids, and the stats with column 7 zeroed
                ri, rf, rn, rs_ = cr.components_image(lo, conn, 0, cap)
                zero7 = so.copy()
                zero7[:, 7] = 0
                assert np.array_equal(ri, io) and np.array_equal(rf, lo) and rn[0] == n[0] and np.array_equal(rs_, zero7)
                # 3: idempotent
                io2, lo2, h2, f2 = hr.holes_image(lo, io, conn, max_area)
                assert np.array_equal(io2, io) and np.array_equal(lo2, lo) and h2[0] == 0 and not f2
                # 4: scipy's fill, where it is the same question
                if ndimage is not None and classes == 1 and conn == 8 and max_area is None and h[0] == h[1]:
                    assert np.array_equal(lo > 0, ndimage.binary_fill_holes(filtered > 0))
                    checked += 1
    assert ndimage is None or checked > 20


def test_batched_reference_with_stats_and_counts():
    rs = np.random.RandomState(3)
    lab = ((rs.rand(2, 11, 13) < 0.8) * rs.randint(1, 3, (2, 11, 13))).astype(np.uint8)
    gt = rs.randint(0, 4, lab.shape).astype(np.uint8)
    gt[0, 0, :3] = 255
    comp = cr.components(lab, 8, 0, 50)
    r = hr.holes(comp["filtered"], comp["ids"], 8, None, comp["stats"], gt, 2)
    assert r["ids"].shape == lab.shape and r["holes"].shape == (2, 2) and r["stats"].shape == (2, 50, 8)
    for b in range(2):
        assert np.array_equal(r["counts"][b], cr.counts_image(r["labels"][b], gt[b], 2))
        assert np.array_equal(hr.holes(comp["filtered"], comp["ids"], 8, None, image=hr.holes_search)["ids"][b], r["ids"][b])


# ------------------------------------------------------------------------------------------------ the C ABI

def _fields(hdr, name):
    body = re.search(r"typedef struct \{([^{}]*)\}\s*" + name + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.replace("*", " ").replace(",", " ").split()
        names += [p for p in parts if p not in ("const", "void", "int32_t", "int64_t", "size_t", "uint8_t")]
    return names


def test_struct_mirror_sizeof_and_signatures(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    assert _fields(hdr, "dfw_seg_holes_args") == [f[0] for f in L.SegHolesArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\nint main(){printf("%zu", sizeof(dfw_seg_holes_args));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(L.SegHolesArgs)
    i32 = C.c_int32
    assert L.SYMBOLS["dfw_seg_holes"] == (i32, [C.POINTER(L.SegHolesArgs), C.c_void_p])
    assert L.SYMBOLS["dfw_seg_holes_workspace_bytes"] == (C.c_size_t, [i32] * 3)
    assert hip_lib.dfw_version() >= 120
    assert "seg_holes.hip" in __import__("diffews_amd.build", fromlist=["SOURCES"]).SOURCES


def test_workspace_query(hip_lib):
    from diffews_amd import ops
    q = hip_lib.dfw_seg_holes_workspace_bytes
    for B in (1, 2, 3, 65535):
        for H, W in ((1, 1), (1, 37), (37, 1), (32, 64), (33, 65), (4096, 4096), (65535, 16384), (32768, 32768)):
            got = q(B, H, W)
            assert got == 8 * B * H * W, (B, H, W)                         # parent and area, one word each a pixel
            assert ops.seg_holes_workspace(B, H, W) == got
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, -2), (65536, 1, 1), (1, 65536, 1), (1, 1, 65536), (1, 65535, 32768),
                (1, 32768, 32769)):
        assert q(*bad) == 0, bad


B_, H_, W_, CAP_, NLAB_ = 2, 5, 7, 3, 3


def _valid(lib):
    """A fully valid dfw_seg_holes call on host memory (never launched: every test below breaks one thing)."""
    from diffews_amd import _lib as L
    ws_bytes = lib.dfw_seg_holes_workspace_bytes(B_, H_, W_)
    assert ws_bytes > 0
    n = B_ * H_ * W_
    keep = dict(labels=np.zeros(n + 8, np.uint8), ids=np.zeros(n + 2, np.int32), stats=np.zeros(B_ * CAP_ * 8 + 2, np.int32),
                gt=np.zeros(n + 8, np.uint8), ids_out=np.zeros(n + 2, np.int32), labels_out=np.zeros(n + 8, np.uint8),
                holes=np.zeros(2 * B_ + 2, np.int32), stats_out=np.zeros(B_ * CAP_ * 8 + 2, np.int32),
                counts=np.zeros(B_ * 2 * (NLAB_ + 1) + 2, np.int64), ws=np.zeros(ws_bytes // 8 + 2, np.int64))
    a = L.SegHolesArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.ws_bytes, a.B, a.H, a.W, a.connectivity, a.max_area, a.cap, a.nlabels = ws_bytes, B_, H_, W_, 8, 5, CAP_, NLAB_
    return a, keep


# field -> (extent in bytes, alignment)
INPUTS = dict(labels=(B_ * H_ * W_, 1), ids=(4 * B_ * H_ * W_, 4), stats=(32 * B_ * CAP_, 4), gt=(B_ * H_ * W_, 1))
OUTPUTS = dict(ids_out=(4 * B_ * H_ * W_, 4), labels_out=(B_ * H_ * W_, 1), holes=(8 * B_, 4), stats_out=(32 * B_ * CAP_, 4),
               counts=(16 * B_ * (NLAB_ + 1), 8), ws=(8 * B_ * H_ * W_, 4))


def test_every_refusal_comes_from_the_host(hip_lib):
    kept = []

    def broken(**kw):
        a, keep = _valid(hip_lib)
        kept.append(keep)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.dfw_seg_holes(C.byref(a), None)

    assert hip_lib.dfw_seg_holes(None, None) == DFW_EINVAL
    for field in ("labels", "ids", "ids_out", "labels_out", "holes", "ws"):
        assert broken(**{field: None}) == DFW_EINVAL, field
    for field in ("B", "H", "W"):
        for v in (0, -1):
            assert broken(**{field: v}) == DFW_EINVAL, field
    for v in (0, 1, 6, 16, -8):
        assert broken(connectivity=v) == DFW_EINVAL, v
    for v in (-1, -2 ** 31):
        assert broken(max_area=v) == DFW_EINVAL, v
    assert broken(stats=None) == DFW_EINVAL                                # stats_out without stats
    for v in (0, -1):
        assert broken(cap=v) == DFW_EINVAL, v                              # stats_out without cap
    assert broken(gt=None) == DFW_EINVAL                                   # counts without gt
    for v in (0, -1, 255, 1000):
        assert broken(nlabels=v) == DFW_EINVAL, v
    assert broken(H=65536, W=1) == DFW_ERANGE
    assert broken(H=1, W=65536) == DFW_ERANGE
    assert broken(H=65535, W=32768) == DFW_ERANGE                          # H * W above 2^30
    assert broken(B=65536) == DFW_ERANGE
    assert broken(cap=2 ** 27) == DFW_ERANGE                               # B * cap * 8 above 2^31 - 1
    a, keep = _valid(hip_lib)
    a.ws_bytes -= 1
    assert hip_lib.dfw_seg_holes(C.byref(a), None) == DFW_EWORKSPACE
    assert broken(ws_bytes=0) == DFW_EWORKSPACE
    assert broken(B=3) == DFW_EWORKSPACE
    # every output (the workspace is one) on every input, at its start and on its last byte; the outputs on each other
    check_overlap_rule(lambda a: hip_lib.dfw_seg_holes(C.byref(a), None), lambda: _valid(hip_lib), INPUTS, OUTPUTS)
    assert hip_lib.dfw_version() >= 122
    # DFW_ESHAPE: words off their natural alignment
    for field, shift in (("ws", 2), ("ws", 1), ("ids", 2), ("ids_out", 1), ("holes", 2), ("stats", 2), ("stats_out", 1), ("counts", 4),
                         ("counts", 1)):
        a, keep = _valid(hip_lib)
        setattr(a, field, getattr(a, field) + shift)
        assert hip_lib.dfw_seg_holes(C.byref(a), None) == DFW_ESHAPE, (field, shift)
    # the order of the house: null before everything, EINVAL before ERANGE, sizes before the workspace, the workspace before
    # overlap, overlap before alignment
    assert broken(labels=None, H=65536) == DFW_EINVAL
    assert broken(H=65536, connectivity=5) == DFW_EINVAL
    assert broken(H=65536, max_area=-1) == DFW_EINVAL
    assert broken(H=65536, nlabels=0) == DFW_EINVAL
    assert broken(H=65536, ws_bytes=0) == DFW_ERANGE
    a, keep = _valid(hip_lib)
    a.ids_out, a.ws_bytes = a.ids, 0
    assert hip_lib.dfw_seg_holes(C.byref(a), None) == DFW_EWORKSPACE
    a, keep = _valid(hip_lib)
    a.ids_out = a.ids + 2
    assert hip_lib.dfw_seg_holes(C.byref(a), None) == DFW_EINVAL


# ------------------------------------------------------------------------------------------------ the objects layer

def test_value_errors_of_the_objects_layer(hip_lib):
    """Every check precedes the launch and the call's own allocations, so host tensors are enough."""
    from diffews_amd import objects
    o = dict(ids=torch.zeros(4, 4, dtype=torch.int32), labels=torch.zeros(4, 4, dtype=torch.uint8),
             n=torch.zeros(2, dtype=torch.int32), stats=torch.zeros(8, 8, dtype=torch.int32), counts=None)
    with pytest.raises(ValueError, match="label_objects result"):
        objects.fill_holes(o)                                              # host tensors
    for conn in (0, 6, "8"):
        with pytest.raises(ValueError, match="connectivity"):
            objects.fill_holes(o, connectivity=conn)
    for area in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="max_area"):
            objects.fill_holes(o, max_area=area)
    lists = {k: [v] for k, v in o.items()}
    with pytest.raises(ValueError, match="one gt / buffers entry per item"):
        objects.fill_holes(lists, buffers=[None, None])
    with pytest.raises(ValueError, match="max_components"):
        objects.HoleBuffers(1, 8, 8, 0, device="cpu")
    for shape in ((0, 8, 8), (1, 65536, 1), (1, 32768, 32769)):
        with pytest.raises(ValueError, match="refuses these sizes"):
            objects.HoleBuffers(*shape, device="cpu")
    buf = objects.HoleBuffers(2, 5, 7, 3, device="cpu")
    assert buf.ids.shape == (2, 5, 7) and buf.labels.dtype == torch.uint8 and buf.holes.shape == (2, 2)
    assert buf.stats.shape == (2, 3, 8) and buf.ws.numel() == hip_lib.dfw_seg_holes_workspace_bytes(2, 5, 7)
    assert buf.counts(4).shape == (2, 2, 5) and buf.counts(4) is buf.counts(4)
