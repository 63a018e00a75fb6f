"""CPU tests of the run-length stage: the numpy reference tests/rle_ref.py against a per-pixel loop, by round trip through
objects.runs_to_mask and on the header's worked example, and the C ABI of dfw_seg_rle -- header, ctypes mirror, sizeof,
the workspace query and every host-side refusal (host pointers, null stream: nothing is launched).  Every comparison is
exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as cr
import rle_ref as rr
from seg_args_cases import check_overlap_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ESHAPE, DFW_ERANGE, DFW_EWORKSPACE = -1, -2, -3, -4


def _ids(lab, conn):
    return cr.components(lab[None], conn, 0, 1)["ids"][0]


# ------------------------------------------------------------------------------------------------ the reference

def test_worked_example_of_the_header():
    from diffews_amd.objects import runs_to_coco, runs_to_mask
    ids = np.array([[1, 1, 0], [2, 1, 1]], np.int32)
    runs, off, n = rr.rle_image(ids, 2, 100, "row")
    assert runs.tolist() == [[0, 2], [4, 2], [3, 1]] and off.tolist() == [0, 2, 3] and n == (3, 3)
    runs, off, n = rr.rle_image(ids, 2, 100, "column")
    assert rr.flatten(ids, "column").tolist() == [1, 2, 1, 1, 0, 1]
    assert runs.tolist() == [[0, 1], [2, 2], [5, 1], [1, 1]] and off.tolist() == [0, 3, 4] and n == (4, 4)
    one = rr.object_rows(runs, off, 1)
    assert runs_to_coco(one, 2, 3) == {"size": [2, 3], "counts": [0, 1, 1, 2, 1, 1]}
    assert runs_to_coco(rr.object_rows(runs, off, 2), 2, 3)["counts"] == [1, 1, 4]
    assert runs_to_coco(np.zeros((0, 2), np.int32), 2, 3)["counts"] == [6]
    assert np.array_equal(runs_to_mask(one, 2, 3, "column"), ids == 1)
    with pytest.raises(ValueError):
        runs_to_coco(one, 2, 3, order="row")
    with pytest.raises(ValueError):
        runs_to_mask(one, 2, 3, "diagonal")
    # ids above cap and negative ids are background; truncation keeps the runs that start first
    runs, off, n = rr.rle_image(np.array([[3, -1, 1], [1, 2, 2]], np.int32), 2, 100, "row")
    assert runs.tolist() == [[2, 2], [4, 2]] and off.tolist() == [0, 1, 2] and n == (2, 2)
    runs, off, n = rr.rle_image(ids, 2, 2, "column")
    assert runs.tolist() == [[0, 1], [1, 1]] and off.tolist() == [0, 1, 2] and n == (2, 4)


@pytest.mark.parametrize("shape", [(5, 7), (9, 11), (1, 37)])
def test_reference_equals_the_pixel_loop_and_round_trips(shape):
    from diffews_amd.objects import runs_to_mask
    H, W = shape
    rs = np.random.RandomState(100 * H + W)
    for name, lab in rr.contents(H, W, rs).items():
        for conn in (4, 8):
            ids = _ids(lab, conn)
            n = int(ids.max())
            for order in rr.ORDERS:
                runs, off, (kept, found) = rr.rle_image(ids, n + 2, H * W, order)
                assert kept == found == len(runs) and off[0] == 0 and off[-1] == kept and (np.diff(off) >= 0).all()
                for k in range(1, n + 1):
                    mine = rr.object_rows(runs, off, k)
                    assert [tuple(r) for r in mine.tolist()] == rr.brute_runs(ids.tolist(), k, order), (name, conn, order, k)
                    assert np.array_equal(runs_to_mask(mine, H, W, order), ids == k), (name, conn, order, k)
                assert off[n] == kept                                      # nothing behind the last object
                # a cap below n drops the higher ids and nothing else
                if n > 1:
                    r2, o2, _ = rr.rle_image(ids, 1, H * W, order)
                    assert np.array_equal(r2, rr.object_rows(runs, off, 1)) and o2.tolist() == [0, len(r2)]


# ------------------------------------------------------------------------------------------------ the C ABI

def test_struct_mirror_and_sizeof(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\}\s*dfw_seg_rle_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.replace("*", " ").replace(",", " ").split()
        names += [p for p in parts if p not in ("const", "void", "int32_t", "int64_t", "size_t", "uint8_t")]
    assert names == [f[0] for f in L.SegRleArgs._fields_]
    assert names == ["ids", "runs", "run_off", "nruns", "ws", "ws_bytes", "B", "H", "W", "cap", "max_runs", "order"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\n'
                   'int main(){printf("%zu", sizeof(dfw_seg_rle_args));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(L.SegRleArgs)
    i32 = C.c_int32
    assert L.SYMBOLS["dfw_seg_rle"] == (i32, [C.POINTER(L.SegRleArgs), C.c_void_p])
    assert L.SYMBOLS["dfw_seg_rle_workspace_bytes"] == (C.c_size_t, [i32] * 6)
    assert L.SYMBOLS["dfw_seg_rle_block"] == (i32, [C.POINTER(i32), C.POINTER(i32)])
    assert hip_lib.dfw_version() >= 115
    assert "seg_rle.hip" in __import__("diffews_amd.build", fromlist=["SOURCES"]).SOURCES


def _block(lib):
    p, r = C.c_int32(), C.c_int32()
    assert lib.dfw_seg_rle_block(C.byref(p), C.byref(r)) == 0
    return p.value, r.value


def test_block_sizes_are_the_shared_ones(hip_lib):
    """The run-length and the matching stage use one compaction and one sort (csrc/seg_sort.h, seg_sort.hip): both block
    queries report the same (pixels, records)."""
    p, r = C.c_int32(), C.c_int32()
    assert hip_lib.dfw_seg_match_block(C.byref(p), C.byref(r)) == 0
    assert (p.value, r.value) == _block(hip_lib)
    assert "seg_sort.hip" in __import__("diffews_amd.build", fromlist=["SOURCES"]).SOURCES


def test_workspace_query_is_monotone(hip_lib):
    q = hip_lib.dfw_seg_rle_workspace_bytes
    P, R = _block(hip_lib)
    assert P >= 1 and R >= 1 and hip_lib.dfw_seg_rle_block(None, None) == DFW_EINVAL
    p, r = C.c_int32(), C.c_int32()
    assert hip_lib.dfw_seg_rle_block(C.byref(p), None) == DFW_EINVAL and hip_lib.dfw_seg_rle_block(None, C.byref(r)) == DFW_EINVAL
    sizes = [1, 2, 37, 64, 65]
    for B in (1, 3):
        for H in sizes:
            for W in sizes:
                for cap in (1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24):
                    for M in (1, R - 1, R, R + 1, 3 * R + 5):
                        got = [q(B, H, W, cap, M, o) for o in (0, 1)]
                        assert got[1] >= got[0] + 4 * B * H * W > 0, (B, H, W, cap, M)      # the transposed plane
                        assert got[0] >= 4 * (3 * B * M + B * -(-(H * W) // P)), (B, H, W, cap, M)
                        for o in (0, 1):
                            assert q(B + 1, H, W, cap, M, o) >= got[o] and q(B, H + 1, W, cap, M, o) >= got[o]
                            assert q(B, H, W + 1, cap, M, o) >= got[o] and q(B, H, W, cap + 1, M, o) >= got[o]
                            assert q(B, H, W, cap, M + 1, o) >= got[o]
    assert q(2, 32768, 32768, 1024, 1 << 20, 1) >= 8 << 30               # no 32-bit arithmetic on the way
    for bad in ((0, 5, 5, 4, 4, 0), (1, 0, 5, 4, 4, 0), (1, 5, -1, 4, 4, 0), (1, 5, 5, 0, 4, 0), (1, 5, 5, 4, 0, 0),
                (1, 5, 5, 4, 4, 2), (1, 5, 5, 4, 4, -1)):
        assert q(*bad) == 0, bad


def _valid(lib, B=2, H=5, W=7, cap=4, max_runs=6, order=1):
    """A fully valid call on host memory (never launched: every test below breaks one thing)."""
    from diffews_amd import _lib as L
    ws_bytes = lib.dfw_seg_rle_workspace_bytes(B, H, W, cap, max_runs, order)
    assert ws_bytes > 0
    keep = dict(ids=np.zeros((B, H, W), np.int32), runs=np.zeros((B, max_runs, 2), np.int32),
                run_off=np.zeros((B, cap + 1), np.int32), nruns=np.zeros((B, 2), np.int32), ws=np.zeros(ws_bytes // 8 + 1, np.int64))
    a = L.SegRleArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.ws_bytes, a.B, a.H, a.W, a.cap, a.max_runs, a.order = ws_bytes, B, H, W, cap, max_runs, order
    return a, keep


def test_every_refusal_comes_from_the_host_before_any_launch(hip_lib):
    kept = []

    def broken(**kw):
        a, keep = _valid(hip_lib)
        kept.append(keep)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.dfw_seg_rle(C.byref(a), None)

    assert hip_lib.dfw_seg_rle(None, None) == DFW_EINVAL
    for field in ("ids", "runs", "run_off", "nruns", "ws"):
        assert broken(**{field: None}) == DFW_EINVAL, field
    for field in ("B", "H", "W", "cap", "max_runs"):
        for v in (0, -1):
            assert broken(**{field: v}) == DFW_EINVAL, field
    for order in (2, -1, 8):
        assert broken(order=order) == DFW_EINVAL, order
    # an output on top of the input, at its start and inside it
    for field in ("runs", "run_off", "nruns"):
        for shift in (0, 4 * 11, 4 * (2 * 5 * 7 - 1)):
            a, keep = _valid(hip_lib)
            setattr(a, field, a.ids + shift)
            assert hip_lib.dfw_seg_rle(C.byref(a), None) == DFW_EINVAL, (field, shift)
    a, keep = _valid(hip_lib)
    a.ids = a.runs + 8                                               # the input inside an output
    assert hip_lib.dfw_seg_rle(C.byref(a), None) == DFW_EINVAL
    # DFW_ERANGE: the sizes are checked before the workspace, which could not be that large here
    assert broken(H=65536, W=1) == DFW_ERANGE
    assert broken(H=1, W=65536) == DFW_ERANGE
    assert broken(H=65535, W=32768) == DFW_ERANGE                    # H * W above 2^30
    assert broken(B=65536) == DFW_ERANGE
    assert broken(max_runs=1 << 29) == DFW_ERANGE                    # B * max_runs * 2 = 2^31
    assert broken(B=1, max_runs=1 << 30) == DFW_ERANGE
    assert broken(cap=1 << 30) == DFW_ERANGE                         # B * (cap + 1) above 2^31 - 1
    assert broken(cap=0x7fffffff) == DFW_ERANGE                      # cap + 1 itself
    # DFW_EWORKSPACE: one byte short; anything larger on the same workspace
    a, keep = _valid(hip_lib)
    a.ws_bytes -= 1
    assert hip_lib.dfw_seg_rle(C.byref(a), None) == DFW_EWORKSPACE
    assert broken(order=0, ws_bytes=0) == DFW_EWORKSPACE
    assert broken(H=6) == DFW_EWORKSPACE
    assert broken(B=3) == DFW_EWORKSPACE
    assert broken(max_runs=7) == DFW_EWORKSPACE
    a, keep = _valid(hip_lib, order=0)
    a.order = 1                                                      # the transposed plane is missing
    assert hip_lib.dfw_seg_rle(C.byref(a), None) == DFW_EWORKSPACE
    a, keep = _valid(hip_lib, cap=255)
    a.cap = 256                                                      # a second sort pass needs its second record buffer
    keep["run_off"] = np.zeros((2, 257), np.int32)
    a.run_off = keep["run_off"].ctypes.data
    assert hip_lib.dfw_seg_rle(C.byref(a), None) == DFW_EWORKSPACE
    # DFW_ESHAPE: words off their natural alignment
    for field in ("ids", "runs", "run_off", "nruns", "ws"):
        a, keep = _valid(hip_lib)
        setattr(a, field, getattr(a, field) + 2)
        assert hip_lib.dfw_seg_rle(C.byref(a), None) == DFW_ESHAPE, field
    # the order of the house: a null pointer wins over a size that is out of range, that over the workspace
    assert broken(ids=None, H=65536) == DFW_EINVAL
    a, keep = _valid(hip_lib)
    a.H, a.ws_bytes = 70000, 0
    assert hip_lib.dfw_seg_rle(C.byref(a), None) == DFW_ERANGE
    assert all(not v.any() for keep in kept for v in keep.values())  # nothing was written by any of these
    # the buffer rule of the object stages: every output and the workspace against every input and each other
    check_overlap_rule(lambda a: hip_lib.dfw_seg_rle(C.byref(a), None), lambda: _valid(hip_lib), dict(ids=(4 * 2 * 5 * 7, 4)),
                       dict(runs=(2 * 6 * 8, 4), run_off=(2 * 5 * 4, 4), nruns=(2 * 8, 4),
                            ws=(hip_lib.dfw_seg_rle_workspace_bytes(2, 5, 7, 4, 6, 1), 4)))
    assert hip_lib.dfw_version() >= 122


def test_ops_pass_the_allocation_scan():
    """ops.seg_rle / seg_rle_workspace allocate nothing: test_launch_guard_cpu's scan of ops.py neither sees them nor
    fails."""
    import test_launch_guard_cpu as scan
    seen = scan._allocating_functions(os.path.join(ROOT, "diffews_amd", "ops.py"))
    assert "seg_rle" not in seen and "seg_rle_workspace" not in seen
    scan.test_every_allocation_of_the_wrappers_is_reachable_and_declared()


def test_wrappers_refuse_wrong_arguments_without_a_device(hip_lib):
    from diffews_amd import objects, ops
    with pytest.raises(ValueError):
        ops.seg_rle_workspace(1, 5, 7, 4, 4, "diagonal")
    with pytest.raises(ValueError):
        objects.object_runs(np.zeros((5, 7), np.int32))              # an id map without max_components
    with pytest.raises(ValueError):
        objects.RunBuffers(1, 5, 7, max_components=0, device="cpu")
