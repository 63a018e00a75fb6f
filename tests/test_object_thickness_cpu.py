"""CPU tests of the Euclidean side of the boundary stage: tests/edt_ref.py's two-pass form against the definition (a
per-pixel search), against scipy where it is installed, against the chessboard reference and on shapes whose answer is
known by hand; the C ABI of the fields appended to dfw_seg_boundary_args and dfw_seg_boundary_counts_args (mirrors, sizeof,
offsetof, the unchanged workspace query, every new refusal and every old one on a valid Euclidean call, on host memory --
validation precedes any launch); and the argument checks of the objects layer that need no device.  All integers: every
comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary_ref as br
import edt_ref as er
from seg_args_cases import check_overlap_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ESHAPE, DFW_ERANGE, DFW_EWORKSPACE = -1, -2, -3, -4


# ------------------------------------------------------------------------------------------------ the reference

def _maps(shape, rs):
    H, W = shape
    yield "constant", np.full((H, W), 3, np.int32)
    yield "empty", np.zeros((H, W), np.int32)
    for trial in range(4):                                                 # several values; 255; above 255; negative
        yield f"random {trial}", rs.randint(0, 4, (H, W)).astype(np.int32) * np.array([1, 257, -3, 85])[trial]
    yield "two touching values", (1 + (np.add.outer(np.arange(H), 2 * np.arange(W)) > (H + W) // 2)).astype(np.int32) * 255
    big = np.kron(rs.randint(0, 3, ((H + 3) // 4, (W + 3) // 4)), np.ones((4, 4), np.int64))[:H, :W]
    yield "blocks", big.astype(np.int32)


SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (5, 7), (12, 13)]


@pytest.mark.parametrize("shape", SHAPES)
def test_two_pass_form_equals_the_definition(shape):
    rs = np.random.RandomState(100 * shape[0] + shape[1])
    for name, m in _maps(shape, rs):
        want = er.d2_search(m)
        got = er.d2_two_pass(m)
        assert np.array_equal(got, want), (name, shape)
        assert np.array_equal(want == 0, m == 0)
        for dmax in (1, 2, 5, 40):
            capped = er.dist2_ref(m, dmax)
            assert capped.dtype == np.uint16 and np.array_equal(capped, np.minimum(want, (dmax + 1) ** 2)), (name, shape, dmax)
            assert np.array_equal(er.dist2_ref(m[None], dmax)[0], capped)


@pytest.mark.parametrize("shape", SHAPES)
def test_equals_scipy_per_value(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(7 * shape[0] + shape[1])
    for name, m in _maps(shape, rs):
        got = er.d2_two_pass(m)
        for v in np.unique(m):
            if v == 0:
                continue
            mask = np.pad(m == v, 1, constant_values=False)                # outside the image differs
            edt2 = np.rint(ndi.distance_transform_edt(mask)[1:-1, 1:-1] ** 2).astype(np.int64)
            assert np.array_equal(got[m == v], edt2[m == v]), (name, shape, int(v))


@pytest.mark.parametrize("shape", SHAPES)
def test_properties_against_the_chessboard_reference(shape):
    H, W = shape
    rs = np.random.RandomState(31 * H + W)
    for name, m in _maps(shape, rs):
        d2 = er.d2_two_pass(m)
        dc = br.dist_ref(m, 40).astype(np.int64)                           # uncapped: no distance here exceeds 7
        assert int(dc.max()) <= 7
        assert (dc * dc <= d2).all() and (d2 <= 2 * dc * dc).all(), name
        p = np.full((H + 2, W + 2), np.iinfo(np.int64).min, np.int64)      # a value no map holds: outside differs
        p[1:-1, 1:-1] = m
        c = p[1:-1, 1:-1]
        near = (p[:-2, 1:-1] != c) | (p[2:, 1:-1] != c) | (p[1:-1, :-2] != c) | (p[1:-1, 2:] != c)
        assert np.array_equal(d2 == 1, near & (m != 0)), name
        for cap in (1, 2, 3, 6):                                           # capping h changes no capped result
            assert np.array_equal(er.d2_two_pass(m, cap), np.minimum(d2, cap * cap)), (name, cap)


def _peak(m, k, dmax=40):
    """(r2, (y, x), capped) of object k of the int map m, through the reference's table."""
    ids = np.asarray(m, np.int32)[None]
    cap = int(ids.max())
    peaks = er.peaks_ref(ids, er.dist2_ref(ids, dmax), cap)
    return er.decode_peak(peaks[0, k - 1], ids.shape[2], dmax)


def test_a_diamond_where_the_chessboard_answer_is_wrong():
    r, c = 6, 7
    yy, xx = np.mgrid[:15, :15]
    m = (np.abs(yy - c) + np.abs(xx - c) <= r).astype(np.int32)
    # the nearest background pixels of the centre lie at |dy| + |dx| = 7: (3, 4) away, distance 5 -- the chessboard says 4
    assert er.d2_search(m)[c, c] == 25 and br.dist_ref(m, 40)[c, c] == 4
    assert _peak(m, 1) == (25, (c, c), False)
    assert _peak(m, 1, dmax=4) == (25, (c, c), True) and _peak(m, 1, dmax=3)[0] == 16


def test_an_l_whose_peak_is_not_its_box_centre():
    m = np.zeros((14, 14), np.int32)
    m[1:13, 1:5] = 2
    m[9:13, 1:13] = 2
    assert m[7, 7] == 0 and m[6, 6] == 0                                   # the box is rows and columns 1..12
    # at the junction: the inner corner's background pixel (8, 5) is (2, 2) away, the outside 3 rows / columns
    d2 = er.d2_search(m)
    assert d2[10, 3] == 8 and int(d2.max()) == 8 and (d2 == 8).sum() == 1
    assert _peak(m, 2) == (8, (10, 3), False)
    assert _peak(m, 1) == (0, None, False)                                 # an id with no pixel


def test_a_ring_whose_centroid_is_background():
    m = np.zeros((13, 13), np.int32)
    m[1:12, 1:12] = 1
    m[4:9, 4:9] = 0
    ys, xs = np.nonzero(m)
    assert (int(ys.mean()), int(xs.mean())) == (6, 6) and m[6, 6] == 0
    r2, pos, capped = _peak(m, 1)
    assert (r2, pos, capped) == (4, (2, 2), False) and m[pos] == 1         # three pixels thick all round


def test_two_equal_peaks_the_smaller_position_wins():
    m = np.zeros((5, 16), np.int32)
    m[1:4, 1:4] = 1
    m[1:4, 6:15] = 1                                                       # id 1 in two pieces, id 2 absent, ids above the cap ignored
    m[2, 4:6] = 3
    d2 = er.d2_search(m)
    assert d2[2, 2] == 4 and (d2 == 4).sum() == 8 and int(d2[m == 1].max()) == 4
    ids = m[None]
    peaks = er.peaks_ref(ids, er.dist2_ref(ids, 5), 2)
    assert peaks.shape == (1, 2) and peaks[0, 1] == 0
    assert er.decode_peak(peaks[0, 0], 16, 5) == (4, (2, 2), False)
    assert peaks[0, 0] == er.peak_key(4, 2, 2, 16) == (4 << 32) | (0xFFFFFFFF - 34)


def test_worked_example_of_the_header():
    m = np.full((3, 3), 7, np.int32)
    assert er.dist2_ref(m, 2).tolist() == [[1, 1, 1], [1, 4, 1], [1, 1, 1]]
    peaks = er.peaks_ref(m[None], er.dist2_ref(m[None], 2), 7)
    assert peaks[0].tolist() == [0] * 6 + [(4 << 32) | (0xFFFFFFFF - 4)]
    assert er.band_ref(m, er.dist2_ref(m, 2), 1).tolist() == [[7, 7, 7], [7, 0, 7], [7, 7, 7]]


# ------------------------------------------------------------------------------------------------ the C ABI

def test_struct_mirrors_sizeof_offsetof_and_version(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    import test_object_boundaries_cpu as tb
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    fields = tb._fields(hdr, "dfw_seg_boundary_args")
    assert fields[-3:] == ["metric", "peaks", "cap"] and fields == [f[0] for f in L.SegBoundaryArgs._fields_]
    cfields = tb._fields(hdr, "dfw_seg_boundary_counts_args")
    assert cfields[-1] == "dist_elem" and cfields == [f[0] for f in L.SegBoundaryCountsArgs._fields_]
    A, Cn = L.SegBoundaryArgs, L.SegBoundaryCountsArgs
    old = [("map", A), ("ws_bytes", A), ("d", A), ("counts", Cn), ("nlabels", Cn)]
    new = [("metric", A), ("peaks", A), ("cap", A), ("dist_elem", Cn)]
    names = {A: "dfw_seg_boundary_args", Cn: "dfw_seg_boundary_counts_args"}
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "diffews_hip.h"\nint main(){printf("%zu %zu", '
                   'sizeof(dfw_seg_boundary_args), sizeof(dfw_seg_boundary_counts_args));\n'
                   + "".join(f'printf(" %zu", offsetof({names[s]}, {f}));\n' for f, s in old + new) + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(A), C.sizeof(Cn)] + [getattr(s, f).offset for f, s in old + new]
    assert A.metric.offset == A.d.offset + 4 and Cn.dist_elem.offset == Cn.nlabels.offset + 4   # appended, nothing moved
    assert hip_lib.dfw_version() >= 124


def test_the_workspace_query_is_what_it_was(hip_lib):
    """One byte a pixel rounded up to 16, for every argument tuple of test_object_boundaries_cpu's query test: h is all the
    state the Euclidean pass needs."""
    q = hip_lib.dfw_seg_boundary_workspace_bytes
    for B in (1, 2, 3, 65535):
        for H, W in ((1, 1), (1, 37), (37, 1), (16, 64), (17, 65), (4096, 4096), (65535, 16384), (32768, 32768)):
            for elem in (1, 4):
                assert q(B, H, W, elem) == (B * H * W + 15) // 16 * 16, (B, H, W, elem)
    for bad in ((0, 4, 4, 1), (-1, 4, 4, 1), (1, 0, 4, 1), (1, 4, -2, 4), (65536, 1, 1, 1), (1, 65536, 1, 1), (1, 1, 65536, 4),
                (1, 65535, 32768, 1), (1, 32768, 32769, 4), (1, 4, 4, 0), (1, 4, 4, 2), (1, 4, 4, 8)):
        assert q(*bad) == 0, bad


B_, H_, W_, CAP_ = 2, 5, 7, 6


def _valid(lib, elem=4, dmax=3, d=2):
    """A fully valid Euclidean dfw_seg_boundary call with peaks on host memory (never launched: every test breaks one thing)."""
    from diffews_amd import _lib as L
    ws_bytes = lib.dfw_seg_boundary_workspace_bytes(B_, H_, W_, elem)
    assert ws_bytes > 0
    keep = dict(map=np.zeros((B_, H_, W_), np.int32), dist=np.zeros((B_, H_, W_ + 1), np.uint16), band=np.zeros((B_, H_, W_), np.int32),
                ws=np.zeros(ws_bytes // 8 + 2, np.int64), peaks=np.zeros((B_, CAP_ + 1), np.int64))
    a = L.SegBoundaryArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.ws_bytes, a.elem, a.B, a.H, a.W, a.dmax, a.d, a.metric, a.cap = ws_bytes, elem, B_, H_, W_, dmax, d, 1, CAP_
    return a, keep


def test_every_refusal_of_a_euclidean_call_comes_from_the_host(hip_lib):
    kept = []

    def broken(**kw):
        a, keep = _valid(hip_lib)
        kept.append(keep)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.dfw_seg_boundary(C.byref(a), None)

    # the new ones
    for v in (2, -1, 3, 1 << 20):
        assert broken(metric=v) == DFW_EINVAL, v
        assert broken(metric=v, peaks=None) == DFW_EINVAL, v
    assert broken(metric=0) == DFW_EINVAL                                  # peaks want the Euclidean metric
    for v in (0, -1):
        assert broken(cap=v) == DFW_EINVAL, v
    a, keep = _valid(hip_lib, elem=1)                                      # ... and an id map
    assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_EINVAL
    assert broken(B=65535, cap=32769) == DFW_ERANGE                        # B * cap = 2^31 + 32767; the workspace comes later
    assert broken(B=65535, cap=32768) == DFW_EWORKSPACE                    # 2^31 - 32768 is allowed
    assert broken(peaks=None, cap=-5, ws_bytes=0) == DFW_EWORKSPACE        # without peaks cap is not looked at
    for shift in (1, 2, 4):
        a, keep = _valid(hip_lib)
        a.peaks += shift
        assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_ESHAPE, shift
    a, keep = _valid(hip_lib)
    a.dist += 1                                                            # uint16: aligned to 2
    assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_ESHAPE
    # dist is 2 * B * H * W bytes in the table: a buffer on its second half is an overlap
    for out, shift in (("band", 0), ("ws", 0), ("peaks", 0)):
        a, keep = _valid(hip_lib)
        setattr(a, out, a.dist + (B_ * H_ * W_ + 1 + 7) // 8 * 8 + shift)
        assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_EINVAL, out
    # the order: EINVAL of the new fields before ERANGE, ERANGE of B * cap before the workspace
    assert broken(metric=2, H=65536) == DFW_EINVAL
    assert broken(cap=0, H=65536) == DFW_EINVAL
    assert broken(d=0, metric=2) == DFW_EINVAL
    assert broken(H=65536, B=65535, cap=32769) == DFW_ERANGE
    assert broken(B=0, cap=1 << 30) == DFW_EINVAL

    # the old ones, unchanged on a valid Euclidean call
    assert hip_lib.dfw_seg_boundary(None, None) == DFW_EINVAL
    for field in ("map", "dist", "ws"):
        assert broken(**{field: None}) == DFW_EINVAL, field
    for v in (0, 2, 3, 8, -1):
        assert broken(elem=v) == DFW_EINVAL, v
    for v in (0, -1, 255, 1000):
        assert broken(dmax=v, d=1) == DFW_EINVAL, v
    for v in (0, -1, 4, 255):
        assert broken(d=v) == DFW_EINVAL, v
    for field in ("B", "H", "W"):
        for v in (0, -1):
            assert broken(**{field: v}) == DFW_EINVAL, field
    assert broken(H=65536, W=1) == DFW_ERANGE
    assert broken(H=1, W=65536) == DFW_ERANGE
    assert broken(H=65535, W=32768) == DFW_ERANGE
    assert broken(B=65536) == DFW_ERANGE
    a, keep = _valid(hip_lib)
    a.ws_bytes -= 1
    assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_EWORKSPACE
    assert broken(ws_bytes=0) == DFW_EWORKSPACE
    assert broken(B=3) == DFW_EWORKSPACE
    for field, shift in (("map", 2), ("map", 1), ("band", 2), ("ws", 2), ("ws", 1)):
        a, keep = _valid(hip_lib)
        setattr(a, field, getattr(a, field) + shift)
        assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_ESHAPE, (field, shift)
    assert broken(map=None, H=65536) == DFW_EINVAL
    assert broken(H=65536, dmax=0) == DFW_EINVAL
    assert broken(H=65536, elem=2) == DFW_EINVAL
    assert broken(H=65536, ws_bytes=0) == DFW_ERANGE
    a, keep = _valid(hip_lib)
    a.dist, a.ws_bytes = a.map, 0
    assert hip_lib.dfw_seg_boundary(C.byref(a), None) == DFW_EWORKSPACE
    assert broken(band=None, d=0, ws_bytes=0) == DFW_EWORKSPACE
    assert broken(band=None, d=99, H=65536) == DFW_ERANGE
    n = B_ * H_ * W_
    check_overlap_rule(lambda a: hip_lib.dfw_seg_boundary(C.byref(a), None), lambda: _valid(hip_lib), dict(map=(4 * n, 4)),
                       dict(dist=(2 * n, 2), band=(4 * n, 4), ws=(hip_lib.dfw_seg_boundary_workspace_bytes(B_, H_, W_, 4), 4),
                            peaks=(8 * B_ * CAP_, 8)))


def _valid_counts(dist_elem=2):
    from diffews_amd import _lib as L
    dt = np.uint16 if dist_elem == 2 else np.uint8
    keep = dict(pred=np.zeros((B_, H_, W_ + 1), np.uint8), pdist=np.zeros((B_, H_, W_ + 1), dt), gt=np.zeros((B_, H_, W_ + 1), np.uint8),
                gdist=np.zeros((B_, H_, W_ + 1), dt), counts=np.zeros((B_, 2, 5), np.int64))
    a = L.SegBoundaryCountsArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.B, a.H, a.W, a.d, a.nlabels, a.dist_elem = B_, H_, W_, 2, 3, dist_elem
    return a, keep


def test_every_refusal_of_counts_with_squared_maps_comes_from_the_host(hip_lib):
    kept = []

    def broken(**kw):
        a, keep = _valid_counts()
        kept.append(keep)
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.dfw_seg_boundary_counts(C.byref(a), None)

    for v in (3, 4, -1, 16):
        assert broken(dist_elem=v) == DFW_EINVAL, v
    assert broken(dist_elem=3, H=65536) == DFW_EINVAL                      # before the sizes' DFW_ERANGE
    for field in ("pdist", "gdist"):                                       # uint16: aligned to 2, and twice the bytes
        a, keep = _valid_counts()
        setattr(a, field, getattr(a, field) + 1)
        assert hip_lib.dfw_seg_boundary_counts(C.byref(a), None) == DFW_ESHAPE, field
        a, keep = _valid_counts()
        a.counts = getattr(a, field) + (2 * B_ * H_ * W_ - 1) // 8 * 8
        assert hip_lib.dfw_seg_boundary_counts(C.byref(a), None) == DFW_EINVAL, field
    # the old ones, unchanged
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
    assert broken(B=65536) == DFW_ERANGE
    for shift in (1, 2, 4):
        a, keep = _valid_counts()
        a.counts += shift
        assert hip_lib.dfw_seg_boundary_counts(C.byref(a), None) == DFW_ESHAPE, shift
    n = B_ * H_ * W_
    for de in (2, 1):
        check_overlap_rule(lambda a: hip_lib.dfw_seg_boundary_counts(C.byref(a), None), lambda: _valid_counts(de),
                           dict(pred=(n, 1), pdist=(de * n, de), gt=(n, 1), gdist=(de * n, de)), dict(counts=(B_ * 2 * 4 * 8, 8)))


# ------------------------------------------------------------------------------------------------ the objects layer

def test_thickness_to_host_decodes_the_table_and_checks_its_argument():
    from diffews_amd import objects
    rs = np.random.RandomState(9)
    ids = np.kron(rs.randint(0, 5, (2, 3, 4)), np.ones((1, 4, 5), np.int64)).astype(np.int32)
    dmax, cap = 1, 6
    peaks = er.peaks_ref(ids, er.dist2_ref(ids, dmax), cap)
    n = np.array([[4, 4], [9, 9]], np.int32)                               # the second count is above the table
    t = dict(dist2=None, peaks=torch.from_numpy(peaks), n=torch.from_numpy(n), dmax=dmax, shape=ids.shape[1:])
    host = objects.thickness_to_host(t)
    assert [len(h) for h in host] == [4, cap]
    for b in range(2):
        assert host[b] == [er.decode_peak(k, ids.shape[2], dmax) for k in peaks[b, :len(host[b])]]
    assert any(r[2] for h in host for r in h) and host[1][5] == (0, None, False)
    one = objects.thickness_to_host(dict(t, peaks=t["peaks"][0], n=t["n"][0]))
    assert one == host[0]
    assert objects.thickness_to_host({k: [v[0], v[1]] if isinstance(v, torch.Tensor) else [v, v] for k, v in t.items()}) == host
    for bad in (None, {}, dict(peaks=t["peaks"]), dict(t, peaks=t["peaks"].int()), dict(t, n=t["n"][:1])):
        with pytest.raises(ValueError):
            objects.thickness_to_host(bad)


def test_object_cores_and_object_thickness_check_their_arguments(hip_lib):
    from diffews_amd import objects
    z = torch.zeros(4, 4, dtype=torch.int32)
    o = dict(ids=z, labels=z.to(torch.uint8), stats=torch.zeros(3, 8, dtype=torch.int32), n=torch.zeros(2, dtype=torch.int32))
    for radius in (-1, 255, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="radius"):
            objects.object_cores(o, radius)
    with pytest.raises(ValueError):
        objects.object_cores(z, 1)
    with pytest.raises(ValueError):
        objects.object_cores({"ids": z}, 1)
    with pytest.raises(ValueError, match="buffers"):
        objects.object_cores(o, 1, buffers=None)
    with pytest.raises(ValueError):
        objects.object_thickness(z)
    with pytest.raises(ValueError):
        objects.object_thickness(o)                                        # host tensors
    with pytest.raises(ValueError, match="254"):
        objects.object_thickness(dict(o, ids=_FakeIds()), dmax=255)
    for kw in (dict(metric="manhattan"), dict(metric="euclidean", max_components=0), dict(max_components=4),
               dict(dtype=torch.uint8, metric="euclidean", max_components=4)):
        with pytest.raises(ValueError):
            objects.BoundaryBuffers(1, 8, 8, 3, **{"dtype": torch.int32, "device": "cpu", **kw})
    with pytest.raises(ValueError, match="metric"):
        objects.boundary_bands(z, metric="manhattan")
    b = objects.BoundaryBuffers(2, 8, 9, 3, torch.int32, "cpu", "euclidean", 5)
    assert b.dist.dtype == torch.uint16 and b.dist.shape == (2, 8, 9) and b.peaks.shape == (2, 5) and b.peaks.dtype == torch.int64
    assert objects.BoundaryBuffers(2, 8, 9, 3, device="cpu").dist.dtype == torch.uint8


class _FakeIds:
    is_cuda, dtype, shape = True, torch.int32, (1, 8, 8)

    def dim(self):
        return 3


def test_ops_still_pass_the_allocation_scan():
    import test_launch_guard_cpu as scan
    seen = scan._allocating_functions(os.path.join(ROOT, "diffews_amd", "ops.py"))
    assert "seg_boundary" not in seen and "seg_boundary_counts" not in seen
    scan.test_every_allocation_of_the_wrappers_is_reachable_and_declared()
