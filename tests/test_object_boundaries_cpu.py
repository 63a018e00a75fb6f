"""CPU tests of the boundary stage: tests/boundary_ref.py against a per-pixel search and against the published
mask_to_boundary written out per class, the C ABI of dfw_seg_boundary and dfw_seg_boundary_counts (struct mirrors, sizeof,
signatures, every refusal in its documented order on host memory -- validation precedes any launch --, the workspace and
block queries), metrics.boundary_width / boundary_iou, and the width limit of the objects layer.  All integers: every
comparison is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import boundary_ref as br
from seg_args_cases import check_overlap_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ESHAPE, DFW_ERANGE, DFW_EWORKSPACE = -1, -2, -3, -4


# ------------------------------------------------------------------------------------------------ the reference

def _maps(shape, rs):
    H, W = shape
    yield "constant", np.full((H, W), 3, np.int32)
    yield "empty", np.zeros((H, W), np.int32)
    for trial in range(4):
        yield f"random {trial}", rs.randint(0, 4, (H, W)).astype(np.int32) * np.array([1, 257, -3, 85])[trial]
    big = np.kron(rs.randint(0, 3, ((H + 3) // 4, (W + 3) // 4)), np.ones((4, 4), np.int64))[:H, :W]
    yield "blocks", big.astype(np.int32)


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (5, 7), (12, 13)])
def test_reference_equals_the_pixel_loop(shape):
    rs = np.random.RandomState(100 * shape[0] + shape[1])
    for name, m in _maps(shape, rs):
        for dmax in (1, 2, 5, 40):                                         # 40: a radius larger than the image
            want = br.dist_loop(m, dmax)
            got = br.dist_ref(m, dmax)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, shape, dmax)
            assert np.array_equal(got == 0, m == 0) and got.max() <= dmax + 1
            assert np.array_equal(br.dist_ref(m[None], dmax)[0], want)
        deep = br.dist_ref(m, 40)
        for dmax in (1, 2, 5):                                             # one dist answers every smaller radius
            assert np.array_equal(br.dist_ref(m, dmax), np.minimum(deep, dmax + 1))
        if name == "constant":
            yy, xx = np.mgrid[:shape[0], :shape[1]]
            edge = np.minimum(np.minimum(yy + 1, shape[0] - yy), np.minimum(xx + 1, shape[1] - xx))
            assert np.array_equal(deep, edge)


def test_worked_example_of_the_header():
    m = np.full((3, 5), 7, np.uint8)
    dist = br.dist_ref(m, 2)
    assert dist.tolist() == [[1, 1, 1, 1, 1], [1, 2, 2, 2, 1], [1, 1, 1, 1, 1]]
    band = br.band_ref(m, dist, 1)
    assert band.dtype == np.uint8 and band.tolist() == [[7, 7, 7, 7, 7], [7, 0, 0, 0, 7], [7, 7, 7, 7, 7]]


@pytest.mark.parametrize("shape", [(1, 1), (9, 1), (12, 13), (30, 41)])
def test_band_is_the_published_boundary_per_class(shape):
    """mask - eroded of mask_to_boundary, for the binary mask of every value and every width up to the radius."""
    rs = np.random.RandomState(shape[0] + shape[1])
    for name, m in _maps(shape, rs):
        dist = br.dist_ref(m, 6)
        for d in (1, 2, 3, 6):
            band = br.band_ref(m, dist, d)
            for v in np.unique(m):
                if v != 0:
                    assert np.array_equal(band == v, br.published_boundary(m == v, d) == 1), (name, shape, d, int(v))
            assert not band[m == 0].any()


def test_counts_reference_on_a_hand_made_map():
    pred = np.array([[[1, 1, 2, 0, 9]]], np.uint8)
    gt = np.array([[[1, 2, 2, 255, 1]]], np.uint8)
    pdist = np.array([[[1, 2, 1, 0, 1]]], np.uint8)
    gdist = np.array([[[1, 1, 2, 1, 1]]], np.uint8)
    # d = 1: l = 1, 0, 2, -, 9 and g = 1, 2, 0, dropped, 1 -> inter: class 1 once; pred: 1, 2 once each (9 has no bin), bin 0
    # once; gt: class 1 twice, class 2 once, bin 0 once
    assert br.counts_ref(pred, pdist, gt, gdist, 1, 2).tolist() == [[[0, 1, 0], [2, 2, 2]]]
    # d = 2: l = 1, 1, 2, -, 9 and g = 1, 2, 2, dropped, 1
    assert br.counts_ref(pred, pdist, gt, gdist, 2, 2).tolist() == [[[0, 1, 1], [0, 3, 2]]]
    # nlabels = 1: gt 2 is dropped as well
    assert br.counts_ref(pred, pdist, gt, gdist, 2, 1).tolist() == [[[0, 1], [0, 2]]]


# ------------------------------------------------------------------------------------------------ the C ABI

def _fields(hdr, name):
    body = re.search(r"typedef struct \{([^{}]*)\}\s*" + name + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.replace("*", " ").replace(",", " ").split()
        names += [p for p in parts if p not in ("const", "void", "int32_t", "int64_t", "size_t", "uint8_t")]
    return names


def test_struct_mirrors_sizeof_and_signatures(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    assert _fields(hdr, "dfw_seg_boundary_args") == [f[0] for f in L.SegBoundaryArgs._fields_]
    assert _fields(hdr, "dfw_seg_boundary_counts_args") == [f[0] for f in L.SegBoundaryCountsArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\n'
                   'int main(){printf("%zu %zu", sizeof(dfw_seg_boundary_args), sizeof(dfw_seg_boundary_counts_args));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [C.sizeof(L.SegBoundaryArgs),
                                                                             C.sizeof(L.SegBoundaryCountsArgs)]
    i32 = C.c_int32
    assert L.SYMBOLS["dfw_seg_boundary"] == (i32, [C.POINTER(L.SegBoundaryArgs), C.c_void_p])
    assert L.SYMBOLS["dfw_seg_boundary_counts"] == (i32, [C.POINTER(L.SegBoundaryCountsArgs), C.c_void_p])
    assert L.SYMBOLS["dfw_seg_boundary_workspace_bytes"] == (C.c_size_t, [i32] * 4)
    assert L.SYMBOLS["dfw_seg_boundary_block"] == (i32, [C.POINTER(i32)] * 3)
    assert hip_lib.dfw_version() >= 119
    assert "seg_boundary.hip" in __import__("diffews_amd.build", fromlist=["SOURCES"]).SOURCES


def test_block_and_workspace_queries(hip_lib):
    from diffews_amd import ops
    r, c, p = C.c_int32(), C.c_int32(), C.c_int32()
    for args in ((None, C.byref(c), C.byref(p)), (C.byref(r), None, C.byref(p)), (C.byref(r), C.byref(c), None)):
        assert hip_lib.dfw_seg_boundary_block(*args) == DFW_EINVAL
    assert hip_lib.dfw_seg_boundary_block(C.byref(r), C.byref(c), C.byref(p)) == 0
    assert ops.seg_boundary_block() == (r.value, c.value, p.value)
    assert r.value >= 1 and c.value % 16 == 0 and p.value % 64 == 0 and 256 % (c.value // 4) == 0
    q = hip_lib.dfw_seg_boundary_workspace_bytes
    for B in (1, 2, 3, 65535):
        for H, W in ((1, 1), (1, 37), (37, 1), (16, 64), (17, 65), (4096, 4096), (65535, 16384), (32768, 32768)):
            for elem in (1, 4):
                got = q(B, H, W, elem)
                assert got >= B * H * W > 0, (B, H, W, elem)               # one byte a pixel
                assert ops.seg_boundary_workspace(B, H, W, elem) == got
                assert (H == 65535 or q(B, H + 1, W, elem) >= got) if H * W < 1 << 29 else True
    for bad in ((0, 4, 4, 1), (-1, 4, 4, 1), (1, 0, 4, 1), (1, 4, -2, 4), (65536, 1, 1, 1), (1, 65536, 1, 1), (1, 1, 65536, 4),
                (1, 65535, 32768, 1), (1, 32768, 32769, 4), (1, 4, 4, 0), (1, 4, 4, 2), (1, 4, 4, 8)):
        assert q(*bad) == 0, bad


def _valid(lib, B=2, H=5, W=7, elem=4, dmax=3, d=2):
    """A fully valid dfw_seg_boundary call on host memory (never launched: every test below breaks one thing)."""
    from diffews_amd import _lib as L
    ws_bytes = lib.dfw_seg_boundary_workspace_bytes(B, H, W, elem)
    assert ws_bytes > 0
    keep = dict(map=np.zeros((B, H, W), np.int32), dist=np.zeros((B, H, W + 1), np.uint8), band=np.zeros((B, H, W), np.int32),
                ws=np.zeros(ws_bytes // 8 + 2, np.int64))
    a = L.SegBoundaryArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.ws_bytes, a.elem, a.B, a.H, a.W, a.dmax, a.d = ws_bytes, elem, B, H, W, dmax, d
    return a, keep


def test_every_refusal_of_seg_boundary_comes_from_the_host(hip_lib):
    kept = []

    def broken(**kw):
        a, keep = _valid(hip_lib)
        kept.append(keep)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.dfw_seg_boundary(C.byref(a), None)

    assert hip_lib.dfw_seg_boundary(None, None) == DFW_EINVAL
    for field in ("map", "dist", "ws"):
        assert broken(**{field: None}) == DFW_EINVAL, field
    for v in (0, 2, 3, 8, -1):
        assert broken(elem=v) == DFW_EINVAL, v
    for v in (0, -1, 255, 1000):
        assert broken(dmax=v, d=1) == DFW_EINVAL, v
    for v in (0, -1, 4, 255):
        assert broken(d=v) == DFW_EINVAL, v                              # outside 1..dmax, with a band
    for field in ("B", "H", "W"):
        for v in (0, -1):
            assert broken(**{field: v}) == DFW_EINVAL, field
    assert broken(H=65536, W=1) == DFW_ERANGE
    assert broken(H=1, W=65536) == DFW_ERANGE
    assert broken(H=65535, W=32768) == DFW_ERANGE                        # H * W above 2^30
    assert broken(B=65536) == DFW_ERANGE
    a, keep = _valid(hip_lib)
    a.ws_bytes -= 1
    assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_EWORKSPACE
    assert broken(ws_bytes=0) == DFW_EWORKSPACE
    assert broken(B=3) == DFW_EWORKSPACE
    # every output on the input, at its start and inside it; the outputs on each other and on the workspace
    last = 4 * (2 * 5 * 7 - 1)
    for out in ("dist", "band", "ws"):
        for shift in (0, last):
            a, keep = _valid(hip_lib)
            setattr(a, out, a.map + shift)
            assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_EINVAL, (out, shift)
    for out, on, shift in (("band", "dist", 0), ("dist", "band", 4 * 69), ("ws", "dist", 68), ("ws", "band", 8), ("dist", "ws", 16)):
        a, keep = _valid(hip_lib)
        setattr(a, out, getattr(a, on) + shift)
        assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_EINVAL, (out, on, shift)
    # DFW_ESHAPE: words off their natural alignment
    for field, shift in (("map", 2), ("map", 1), ("band", 2), ("ws", 2), ("ws", 1)):
        a, keep = _valid(hip_lib)
        setattr(a, field, getattr(a, field) + shift)
        assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_ESHAPE, (field, shift)
    # the order of the house: null before everything, EINVAL before ERANGE, sizes before the workspace, the workspace
    # before overlap, overlap before alignment; without a band d is not looked at
    assert broken(map=None, H=65536) == DFW_EINVAL
    assert broken(H=65536, dmax=0) == DFW_EINVAL
    assert broken(H=65536, elem=2) == DFW_EINVAL
    assert broken(H=65536, ws_bytes=0) == DFW_ERANGE
    a, keep = _valid(hip_lib)
    a.dist, a.ws_bytes = a.map, 0
    assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_EWORKSPACE
    a, keep = _valid(hip_lib)
    a.dist = a.map + 2
    assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_EINVAL
    assert broken(band=None, d=0, ws_bytes=0) == DFW_EWORKSPACE
    assert broken(band=None, d=99, H=65536) == DFW_ERANGE
    # the buffer rule of the object stages: every output and the workspace against every input and each other
    check_overlap_rule(lambda a: hip_lib.dfw_seg_boundary(C.byref(a), None), lambda: _valid(hip_lib), dict(map=(4 * 2 * 5 * 7, 4)),
                       dict(dist=(2 * 5 * 7, 1), band=(4 * 2 * 5 * 7, 4), ws=(hip_lib.dfw_seg_boundary_workspace_bytes(2, 5, 7, 4), 4)))
    assert hip_lib.dfw_version() >= 122


def _valid_counts(B=2, H=5, W=7, d=2, nlabels=3):
    from diffews_amd import _lib as L
    keep = {k: np.zeros((B, H, W + 1), np.uint8) for k in ("pred", "pdist", "gt", "gdist")}
    keep["counts"] = np.zeros((B, 2, nlabels + 2), np.int64)
    a = L.SegBoundaryCountsArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.B, a.H, a.W, a.d, a.nlabels = B, H, W, d, nlabels
    return a, keep


def test_every_refusal_of_seg_boundary_counts_comes_from_the_host(hip_lib):
    kept = []

    def broken(**kw):
        a, keep = _valid_counts()
        kept.append(keep)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.dfw_seg_boundary_counts(C.byref(a), None)

    assert hip_lib.dfw_seg_boundary_counts(None, None) == DFW_EINVAL
    for field in ("pred", "pdist", "gt", "gdist", "counts"):
        assert broken(**{field: None}) == DFW_EINVAL, field
    for v in (0, -1, 255, 1000):
        assert broken(d=v) == DFW_EINVAL, v
        assert broken(nlabels=v) == DFW_EINVAL, v
    for field in ("B", "H", "W"):
        for v in (0, -1):
            assert broken(**{field: v}) == DFW_EINVAL, field
    assert broken(H=65536, W=1) == DFW_ERANGE
    assert broken(H=1, W=65536) == DFW_ERANGE
    assert broken(H=65535, W=32768) == DFW_ERANGE
    assert broken(B=65536) == DFW_ERANGE
    for inp in ("pred", "pdist", "gt", "gdist"):
        for shift in (0, 2 * 5 * 7 - 1):
            a, keep = _valid_counts()
            a.counts = getattr(a, inp) + shift
            assert hip_lib.dfw_seg_boundary_counts(C.byref(a), None) == DFW_EINVAL, (inp, shift)
    a, keep = _valid_counts()
    a.gt = a.counts + 8
    assert hip_lib.dfw_seg_boundary_counts(C.byref(a), None) == DFW_EINVAL
    for shift in (1, 2, 4):
        a, keep = _valid_counts()
        a.counts += shift
        assert hip_lib.dfw_seg_boundary_counts(C.byref(a), None) == DFW_ESHAPE, shift
    assert broken(pred=None, H=65536) == DFW_EINVAL
    assert broken(H=65536, nlabels=0) == DFW_EINVAL
    a, keep = _valid_counts()
    a.counts = a.pred + 1                                                  # overlap before alignment
    assert hip_lib.dfw_seg_boundary_counts(C.byref(a), None) == DFW_EINVAL
    # the buffer rule of the object stages: every output and the workspace against every input and each other
    check_overlap_rule(lambda a: hip_lib.dfw_seg_boundary_counts(C.byref(a), None), _valid_counts,
                       {k: (2 * 5 * 7, 1) for k in ("pred", "pdist", "gt", "gdist")}, dict(counts=(2 * 2 * 4 * 8, 8)))


# ------------------------------------------------------------------------------------------------ metrics and the limit

def test_boundary_width():
    from diffews_amd import metrics
    assert metrics.boundary_width(512, 512) == 14
    assert metrics.boundary_width(4096, 4096) == 116
    assert metrics.boundary_width(10, 10) == 1
    assert metrics.boundary_width(1, 1) == 1
    assert metrics.boundary_width(100, 100, ratio=0.05) == 7
    for h, w in ((512, 512), (4096, 4096), (10, 10), (37, 1), (1080, 1920)):
        assert metrics.boundary_width(h, w) == br.width(h, w)
    assert metrics.boundary_width(9000, 9000) == 255                       # a diagonal of 12 728: one above the limit


def test_the_objects_layer_refuses_a_width_above_254():
    """The check precedes every launch and every allocation of the call's own, so it needs no GPU -- only a tensor that
    says it is on one."""
    from diffews_amd import objects

    class Fake:
        is_cuda, dtype, shape = True, torch.uint8, (1, 9000, 9000)

        def dim(self):
            return 3
    with pytest.raises(ValueError, match="254"):
        objects.boundary_bands(Fake())
    with pytest.raises(ValueError, match="254"):
        objects.boundary_bands(Fake(), d=3, dmax=255)
    with pytest.raises(ValueError):
        objects.boundary_bands(torch.zeros(4, 4, dtype=torch.uint8))      # a host tensor
    with pytest.raises(ValueError, match="254"):
        objects.BoundaryBuffers(1, 8, 8, 255, device="cpu")


def test_boundary_iou_on_hand_made_counts():
    from diffews_amd import metrics
    counts = torch.tensor([[[50, 3, 0, 0], [60, 4, 5, 0]], [[10, 1, 2, 0], [20, 4, 3, 0]]], dtype=torch.int64)
    iou, miou = metrics.boundary_iou(counts)
    want = [100.0 * 60 / 80, 100.0 * 4 / 8, 100.0 * 2 / 8, 0.0]
    assert iou.dtype == torch.float64 and iou.tolist() == want
    assert miou == (want[1] + want[2]) / 2                                 # class 3 has no union, bin 0 is not a class
    both = metrics.nway_iou(counts)
    assert both[0].tolist() == want and both[1] == miou
    per_item = metrics.boundary_iou([counts[0], counts[1]])               # ragged sizes: a list of [2, N + 1] tables
    assert per_item[0].tolist() == want and per_item[1] == miou
