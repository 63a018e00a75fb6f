"""CPU tests of the connected-components stage: the numpy reference tests/components_ref.py on hand-written answers and
(where scipy is installed) against scipy.ndimage.label as a partition, and the C ABI of dfw_seg_components -- header,
ctypes mirror, sizeof, the workspace query and every host-side refusal (host pointers, null stream: nothing is launched).
Every comparison is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as cr
from seg_args_cases import check_overlap_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ESHAPE, DFW_ERANGE, DFW_EWORKSPACE = -1, -2, -3, -4


def _img(rows):
    return np.array([[int(c) for c in r.split()] for r in rows], dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the reference

def test_diagonal_touch_is_one_object_only_with_eight_neighbours():
    lab = _img(["1 0 0 0 0 0 0",
                "0 1 1 0 0 0 0",
                "0 0 0 1 0 0 0",
                "0 0 0 0 0 0 0",
                "0 0 0 0 0 0 1"])
    ids, filt, n, stats = cr.components_image(lab, 4, 0, 8)
    assert n == (4, 4)
    assert ids.tolist() == [[1, 0, 0, 0, 0, 0, 0], [0, 2, 2, 0, 0, 0, 0], [0, 0, 0, 3, 0, 0, 0], [0] * 7, [0, 0, 0, 0, 0, 0, 4]]
    assert stats[:4].tolist() == [[1, 1, 0, 0, 1, 1, 0, 0], [1, 2, 1, 1, 2, 3, 8, 0], [1, 1, 2, 3, 3, 4, 17, 0],
                                  [1, 1, 4, 6, 5, 7, 34, 0]]
    assert not stats[4:].any() and np.array_equal(filt, lab)
    ids, filt, n, stats = cr.components_image(lab, 8, 0, 8)
    assert n == (2, 2)
    assert ids.tolist() == [[1, 0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0], [0] * 7, [0, 0, 0, 0, 0, 0, 2]]
    assert stats[:2].tolist() == [[1, 4, 0, 0, 3, 4, 0, 0], [1, 1, 4, 6, 5, 7, 34, 0]] and not stats[2:].any()


def test_two_classes_side_by_side_do_not_merge():
    lab = _img(["0 0 0 0 0 0 0",
                "0 1 1 2 2 0 0",
                "0 1 1 2 2 0 0",
                "0 0 0 0 3 3 0",
                "0 0 0 0 0 0 0"])
    for conn in (4, 8):
        ids, filt, n, stats = cr.components_image(lab, conn, 0, 4)
        assert n == (3, 3)
        assert ids.tolist() == [[0] * 7, [0, 1, 1, 2, 2, 0, 0], [0, 1, 1, 2, 2, 0, 0], [0, 0, 0, 0, 3, 3, 0], [0] * 7]
        assert stats.tolist() == [[1, 4, 1, 1, 3, 3, 8, 0], [2, 4, 1, 3, 3, 5, 10, 0], [3, 2, 3, 4, 4, 6, 25, 0], [0] * 8]


def test_ring_around_a_dot_is_numbered_by_first_pixel():
    """The ring starts at pixel 0 and encloses the dot; the lone pixel at the end of row 0 comes before the dot."""
    lab = _img(["1 1 1 1 1 0 3",
                "1 0 0 0 1 0 0",
                "1 0 2 0 1 0 0",
                "1 0 0 0 1 0 0",
                "1 1 1 1 1 0 0"])
    for conn in (4, 8):
        ids, filt, n, stats = cr.components_image(lab, conn, 0, 3)
        assert n == (3, 3)
        assert ids.tolist() == [[1, 1, 1, 1, 1, 0, 2], [1, 0, 0, 0, 1, 0, 0], [1, 0, 3, 0, 1, 0, 0], [1, 0, 0, 0, 1, 0, 0],
                                [1, 1, 1, 1, 1, 0, 0]]
        assert stats.tolist() == [[1, 16, 0, 0, 5, 5, 0, 0], [3, 1, 0, 6, 1, 7, 6, 0], [2, 1, 2, 2, 3, 3, 16, 0]]
    # the table truncates, nothing else does
    ids2, _, n2, stats2 = cr.components_image(lab, 8, 0, 2)
    assert n2 == (3, 3) and np.array_equal(ids2, ids) and stats2.tolist() == stats[:2].tolist()


def test_area_equal_to_min_area_stays_and_one_less_goes():
    lab = _img(["1 1 1 0 2 2 0",
                "0 0 0 0 0 0 0",
                "5 0 0 4 4 0 0",
                "0 0 0 4 0 0 0",
                "0 0 0 0 0 0 9"])
    ids, filt, n, stats = cr.components_image(lab, 4, 3, 8)
    assert n == (2, 5)
    assert ids.tolist() == [[1, 1, 1, 0, 0, 0, 0], [0] * 7, [0, 0, 0, 2, 2, 0, 0], [0, 0, 0, 2, 0, 0, 0], [0] * 7]
    assert filt.tolist() == [[1, 1, 1, 0, 0, 0, 0], [0] * 7, [0, 0, 0, 4, 4, 0, 0], [0, 0, 0, 4, 0, 0, 0], [0] * 7]
    assert stats[:2].tolist() == [[1, 3, 0, 0, 1, 3, 0, 0], [4, 3, 2, 3, 4, 5, 17, 0]] and not stats[2:].any()
    for keep_all in (0, 1):
        assert cr.components_image(lab, 4, keep_all, 8)[2] == (5, 5)
    assert cr.components_image(lab, 4, 4, 8)[2] == (0, 5)
    # counts are taken on the FILTERED bytes: the removed 2-pixel object of class 2 no longer meets its ground truth
    gt = lab.copy()
    gt[4, 6] = 255
    c = cr.counts_image(filt, gt, 5)
    assert c.tolist() == [[25, 3, 0, 0, 3, 0], [28, 3, 2, 0, 3, 1]]
    assert cr.counts_image(lab, gt, 5).tolist() == [[25, 3, 2, 0, 3, 1], [25, 3, 2, 0, 3, 1]]
    # a predicted byte above nlabels (the 9, the 5 with nlabels = 4) has no bin; a gt byte above it drops the pixel
    gt2 = np.zeros_like(lab)
    assert cr.counts_image(lab, gt2, 4).tolist() == [[25, 0, 0, 0, 0], [35, 3, 2, 0, 3]]
    r = cr.components(lab[None], 4, 3, 8, gt[None], 5)
    assert r["n"].tolist() == [[2, 5]] and np.array_equal(r["counts"][0], c) and r["ids"].shape == (1, 5, 7)


@pytest.mark.parametrize("classes", [1, 3])
def test_reference_is_scipy_labels_partition(classes):
    """Per class, scipy.ndimage.label's components and the reference's ids of that class are the same partition: a
    bijection between the two numberings; the reference's own numbers ascend with the first pixel."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5 + classes)
    structure = {4: ndi.generate_binary_structure(2, 1), 8: ndi.generate_binary_structure(2, 2)}
    for density in (0.3, 0.5, 0.65):
        lab = ((rng.random((23, 31)) < density) * rng.integers(1, classes + 1, (23, 31))).astype(np.uint8)
        for conn in (4, 8):
            ids, filt, (kept, found), stats = cr.components_image(lab, conn, 0, 1024)
            assert kept == found and np.array_equal(filt, lab) and np.array_equal(ids > 0, lab > 0)
            total = 0
            for c in range(1, classes + 1):
                want, k = ndi.label(lab == c, structure[conn])
                total += k
                pairs = set(zip(want[lab == c].tolist(), ids[lab == c].tolist()))
                assert len(pairs) == k and len({a for a, _ in pairs}) == k and len({b for _, b in pairs}) == k
            assert total == kept
            first = stats[:kept, 6]
            assert (np.diff(first) > 0).all()
            flat = ids.ravel()
            assert all(flat[first[i]] == i + 1 and not (flat[:first[i]] == i + 1).any() for i in range(kept))
            assert stats[:kept, 1].tolist() == np.bincount(flat, minlength=kept + 1)[1:].tolist()


# ------------------------------------------------------------------------------------------------ the C ABI

def test_struct_mirror_and_sizeof(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\}\s*dfw_seg_components_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.replace("*", " ").replace(",", " ").split()
        names += [p for p in parts if p not in ("const", "void", "int32_t", "int64_t", "size_t", "uint8_t")]
    assert names == [f[0] for f in L.SegComponentsArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\n'
                   'int main(){printf("%zu", sizeof(dfw_seg_components_args));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(L.SegComponentsArgs)
    i32 = C.c_int32
    assert L.SYMBOLS["dfw_seg_components"] == (i32, [C.POINTER(L.SegComponentsArgs), C.c_void_p])
    assert L.SYMBOLS["dfw_seg_components_workspace_bytes"] == (C.c_size_t, [i32, i32, i32])
    assert L.SYMBOLS["dfw_seg_components_tile"] == (i32, [C.POINTER(i32), C.POINTER(i32)])
    assert hip_lib.dfw_version() >= 114
    assert "seg_components.hip" in __import__("diffews_amd.build", fromlist=["SOURCES"]).SOURCES


def _tile(lib):
    th, tw = C.c_int32(), C.c_int32()
    assert lib.dfw_seg_components_tile(C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


def test_workspace_query_is_monotone_and_bounded(hip_lib):
    q = hip_lib.dfw_seg_components_workspace_bytes
    th, tw = _tile(hip_lib)
    assert th >= 1 and tw >= 1 and hip_lib.dfw_seg_components_tile(None, None) == DFW_EINVAL
    sizes = [1, 2, 5, th - 1, th, th + 1, tw, tw + 1, 2 * th + 3, 3 * tw + 5, 512, 4096]
    for B in (1, 2, 3, 7):
        for H in sizes:
            for W in sizes:
                got = q(B, H, W)
                tiles = -(-H // th) * -(-W // tw)
                assert 8 * B * H * W <= got <= 8 * B * H * W + 8 * B * tiles, (B, H, W)
                assert q(B + 1, H, W) >= got and q(B, H + 1, W) >= got and q(B, H, W + 1) >= got
    assert q(1, 32768, 32768) >= 8 << 30                      # no 32-bit arithmetic on the way
    assert q(0, 5, 5) == 0 and q(1, 0, 5) == 0 and q(1, 5, -1) == 0


def _valid(lib, B=2, H=5, W=7, cap=4, nlabels=3):
    """A fully valid call on host memory (never launched: every test below breaks one thing)."""
    from diffews_amd import _lib as L
    ws_bytes = lib.dfw_seg_components_workspace_bytes(B, H, W)
    keep = dict(labels=np.zeros((B, H, W), np.uint8), ids=np.zeros((B, H, W), np.int32), filtered=np.zeros((B, H, W), np.uint8),
                n=np.zeros((B, 2), np.int32), stats=np.zeros((B, cap, 8), np.int32), gt=np.zeros((B, H, W), np.uint8),
                counts=np.zeros((B, 2, nlabels + 1), np.int64), ws=np.zeros(ws_bytes // 8 + 1, np.int64))
    a = L.SegComponentsArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.ws_bytes, a.B, a.H, a.W, a.connectivity, a.min_area, a.cap, a.nlabels = ws_bytes, B, H, W, 8, 0, cap, nlabels
    return a, keep


def test_every_refusal_comes_from_the_host_before_any_launch(hip_lib):
    def broken(**kw):
        a, keep = _valid(hip_lib)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.dfw_seg_components(C.byref(a), None)

    assert hip_lib.dfw_seg_components(None, None) == DFW_EINVAL
    for field in ("labels", "ids", "n", "ws"):
        assert broken(**{field: None}) == DFW_EINVAL, field
    for field in ("B", "H", "W"):
        for v in (0, -1):
            assert broken(**{field: v}) == DFW_EINVAL, field
    for conn in (0, 1, 6, 9, -8):
        assert broken(connectivity=conn) == DFW_EINVAL, conn
    assert broken(min_area=-1) == DFW_EINVAL
    for cap in (0, -3):
        assert broken(cap=cap) == DFW_EINVAL                     # stats with cap < 1
    assert broken(gt=None) == DFW_EINVAL                         # counts without gt
    for nl in (0, -1, 255, 1000):
        assert broken(nlabels=nl) == DFW_EINVAL, nl              # gt with nlabels outside 1..254
    a, keep = _valid(hip_lib)
    a.filtered = a.labels
    assert hip_lib.dfw_seg_components(C.byref(a), None) == DFW_EINVAL
    # DFW_ERANGE: the sizes are checked before the workspace, which could not be that large here
    assert broken(H=65536, W=1) == DFW_ERANGE
    assert broken(H=1, W=65536) == DFW_ERANGE
    assert broken(H=65535, W=32768) == DFW_ERANGE                # H * W above 2^30
    assert broken(B=65536) == DFW_ERANGE
    assert broken(cap=1 << 28) == DFW_ERANGE                     # B * cap * 8 words no longer fit the zeroing launch
    # DFW_EWORKSPACE: one byte short; a larger image on the same workspace
    a, keep = _valid(hip_lib)
    a.ws_bytes -= 1
    assert hip_lib.dfw_seg_components(C.byref(a), None) == DFW_EWORKSPACE
    assert broken(H=6) == DFW_EWORKSPACE
    assert broken(B=3) == DFW_EWORKSPACE
    assert broken(H=32768, W=32768) == DFW_EWORKSPACE            # exactly 2^30 pixels: in range
    # DFW_ESHAPE: words off their natural alignment
    a, keep = _valid(hip_lib)
    a.ids += 2
    assert hip_lib.dfw_seg_components(C.byref(a), None) == DFW_ESHAPE
    a, keep = _valid(hip_lib)
    a.counts += 4
    assert hip_lib.dfw_seg_components(C.byref(a), None) == DFW_ESHAPE
    # the order of the house: a null pointer wins over a size that is out of range, that over the workspace
    assert broken(labels=None, H=65536) == DFW_EINVAL
    a, keep = _valid(hip_lib)
    a.H, a.ws_bytes = 70000, 0
    assert hip_lib.dfw_seg_components(C.byref(a), None) == DFW_ERANGE
    # nothing was written by any of these
    assert not keep["ids"].any() and not keep["n"].any()
    # the buffer rule of the object stages: every output and the workspace against every input and each other
    px, ws = 2 * 5 * 7, hip_lib.dfw_seg_components_workspace_bytes(2, 5, 7)
    check_overlap_rule(lambda a: hip_lib.dfw_seg_components(C.byref(a), None), lambda: _valid(hip_lib),
                       dict(labels=(px, 1), gt=(px, 1)),
                       dict(ids=(4 * px, 4), n=(2 * 8, 4), filtered=(px, 1), stats=(2 * 4 * 32, 4), counts=(2 * 2 * 4 * 8, 8),
                            ws=(ws, 4)))
    assert hip_lib.dfw_version() >= 122


def test_optional_outputs_may_be_absent(hip_lib):
    """filtered / stats / gt / counts null pass the checks: the call gets as far as the workspace check."""
    a, keep = _valid(hip_lib)
    a.filtered = a.stats = a.gt = a.counts = None
    a.cap, a.nlabels, a.ws_bytes = 0, 0, 0
    assert hip_lib.dfw_seg_components(C.byref(a), None) == DFW_EWORKSPACE
    a, keep = _valid(hip_lib)
    a.counts, a.ws_bytes = None, 0                                # gt without counts is allowed (and unused)
    assert hip_lib.dfw_seg_components(C.byref(a), None) == DFW_EWORKSPACE


def test_ops_still_pass_the_allocation_scan():
    """ops.seg_components / seg_components_workspace allocate nothing: test_launch_guard_cpu's scan of ops.py, whose
    lists of allocating functions live in existing test files, neither sees them nor fails."""
    import test_launch_guard_cpu as scan
    seen = scan._allocating_functions(os.path.join(ROOT, "diffews_amd", "ops.py"))
    assert "seg_components" not in seen and "seg_components_workspace" not in seen
    scan.test_every_allocation_of_the_wrappers_is_reachable_and_declared()
