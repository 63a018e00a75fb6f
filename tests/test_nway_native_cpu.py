"""CPU tests of N-way labels and counts at native size: the binding against the header and the compiler,
dfw_seg_labels_native's host-side validation (no launch, no GPU), and the CPU reference (tests/nway_native_ref.py) pinned on
the input the GPU tests rely on and tied, for N = 1, to the binary native reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import native_ref as nr
import nway_native_ref as nn
import nway_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE, ERANGE, EWORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    from diffews_amd import build, _lib
    build.build()
    return _lib.lib()


def test_labels_native_struct_matches_header_and_compiler(tmp_path):
    """SegLabelsNativeArgs mirrors dfw_seg_labels_native_args field for field and in size; the symbol is bound."""
    import subprocess
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    cname, cls = "dfw_seg_labels_native_args", L.SegLabelsNativeArgs
    body = re.search(r"typedef struct \{([^{}]*)\}\s*" + cname + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.strip().replace("*", " ").replace(",", " ").split()
        names += [p for p in parts if p not in ("const", "void", "float", "int32_t", "int64_t", "size_t", "uint8_t", "uint32_t")]
    assert names == [f[0] for f in cls._fields_]
    for need in ("N", "tmp_cls_stride", "u8_cls_stride", "labels", "labels_bytes", "out_u8", "mx", "counts", "class_ids"):
        assert need in names, need
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\nint main(){printf("%zu %zu", sizeof(' + cname +
                   '), sizeof(dfw_native_item));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [C.sizeof(cls), C.sizeof(L.NativeItem)]
    assert "dfw_seg_labels_native" in L.SYMBOLS


def _valid_args(L, N=3, sizes=((37, 83), (64, 64)), src=(64, 64), with_gt=True, with_u8=True):
    """A fully valid dfw_seg_labels_native call on host memory (never launched: every test below breaks one thing)."""
    from diffews_amd.input_pipeline import NativeTargets
    gts = [np.zeros(s, np.uint8) for s in sizes] if with_gt else None
    t = NativeTargets(src, sizes, gt=gts, device=None)
    B = len(sizes)
    tmp_n = N * t.tmp_bytes + (0 if with_u8 else N * t.u8_bytes)
    keep = dict(t=t, seg=np.zeros((N, B, 3) + tuple(src), np.uint8), tmp=np.zeros(tmp_n, np.uint8),
                u8=np.zeros(N * t.u8_bytes, np.uint8), labels=np.zeros(t.pred_bytes, np.uint8),
                mx=np.zeros(N * B, np.uint32), counts=np.zeros((B, 2, N + 1), np.int64), ids=np.arange(N, dtype=np.int32))
    a = L.SegLabelsNativeArgs()
    a.seg_u8, a.N, a.B, a.Hs, a.Ws = keep["seg"].ctypes.data, N, B, src[0], src[1]
    a.items = a.items_host = C.addressof(t.items)
    a.weights, a.weights_bytes = t.host.ctypes.data, t.host.nbytes
    a.gt, a.gt_bytes = (t.host.ctypes.data, t.host.nbytes) if with_gt else (None, 0)
    a.tmp, a.tmp_bytes, a.tmp_res_off = keep["tmp"].ctypes.data, tmp_n, N * t.tmp_bytes
    a.tmp_cls_stride, a.u8_cls_stride = t.tmp_bytes, t.u8_bytes
    if with_u8:
        a.out_u8, a.out_u8_bytes = keep["u8"].ctypes.data, N * t.u8_bytes
    a.labels, a.labels_bytes = keep["labels"].ctypes.data, t.pred_bytes
    a.mx, a.counts = keep["mx"].ctypes.data, keep["counts"].ctypes.data if with_gt else None
    a.class_ids = keep["ids"].ctypes.data
    a.r_threshold, a.threshold, a.batch_max = 0.25, 0.0, 0
    return a, keep


def test_seg_labels_native_validates_on_the_host_before_any_launch(lib):
    """Every return code of the header's contract, on host memory with no GPU: a call that got past the validation would
    launch and fail differently (or crash), so each assertion also shows that nothing was launched."""
    from diffews_amd import _lib as L
    call = lambda a: lib.dfw_seg_labels_native(C.byref(a), None)
    assert lib.dfw_seg_labels_native(None, None) == EINVAL
    for field in ("seg_u8", "items", "items_host", "weights", "tmp", "labels"):
        a, keep = _valid_args(L)
        setattr(a, field, None)
        assert call(a) == EINVAL, field
    for bad in (0, -1, 255):
        a, keep = _valid_args(L)
        a.N = bad                                       # N outside 1..254
        assert call(a) == EINVAL, bad
    a, keep = _valid_args(L)
    a.gt = None                                         # counts without a ground truth
    assert call(a) == EINVAL
    a, keep = _valid_args(L)
    a.mx = None                                         # dynamic threshold without the maxima
    assert call(a) == EINVAL
    a, keep = _valid_args(L)
    a.r_threshold = 0.0                                 # neither thresholding flag
    assert call(a) == EINVAL
    for field in ("B", "Hs", "Ws"):
        a, keep = _valid_args(L)
        setattr(a, field, 0)
        assert call(a) == EINVAL, field
    for field in ("h", "w"):
        for bad in (0, -3):
            a, keep = _valid_args(L)
            setattr(keep["t"].items[1], field, bad)
            assert call(a) == EINVAL, field
    a, keep = _valid_args(L)
    keep["t"].items[0].gt_elem = 2
    assert call(a) == EINVAL
    for field in ("xk", "yk"):
        a, keep = _valid_args(L)
        setattr(keep["t"].items[0], field, getattr(keep["t"].items[0], field) + 2)
        assert call(a) == ESHAPE, field
    a, keep = _valid_args(L)
    a.Ws = 128                                          # the table's x weights were made for Ws = 64: other ksize
    assert call(a) == ESHAPE
    a, keep = _valid_args(L)
    keep["t"].items[0].yc_off += 2                      # misaligned int32 weights
    assert call(a) == ESHAPE
    for field in ("h", "w"):
        a, keep = _valid_args(L)
        setattr(keep["t"].items[1], field, 65536)
        assert call(a) == ERANGE, field
    for field in ("Hs", "Ws", "B"):
        a, keep = _valid_args(L)
        setattr(a, field, 65536)
        assert call(a) == ERANGE, field
    a, keep = _valid_args(L, N=254)
    a.B = 259                                           # 254 * 259 = 65786 > 65535, each factor in range
    assert call(a) == ERANGE
    for with_u8, fields in ((True, ("tmp_bytes", "out_u8_bytes", "labels_bytes", "gt_bytes")),
                            (False, ("tmp_bytes", "tmp_res_off", "labels_bytes"))):
        for field in fields:
            a, keep = _valid_args(L, with_u8=with_u8)
            setattr(a, field, getattr(a, field) - 16)   # the last class' last image no longer fits
            assert call(a) == EWORKSPACE, (with_u8, field)
    a, keep = _valid_args(L, with_u8=False)
    a.tmp_res_off = a.tmp_bytes + 16                    # the staged bytes start past the scratch
    assert call(a) == EWORKSPACE
    for field in ("tmp_cls_stride", "u8_cls_stride"):
        a, keep = _valid_args(L)
        setattr(a, field, getattr(a, field) - 16)       # smaller than one class plane's extent: classes would overlap
        assert call(a) == EWORKSPACE, field
        a, keep = _valid_args(L)
        setattr(a, field, getattr(a, field) + 16)       # the last class leaves the buffer
        assert call(a) == EWORKSPACE, field
        a, keep = _valid_args(L, N=1)
        setattr(a, field, 0)                            # a stride holds one plane even when no second class uses it
        assert call(a) == EWORKSPACE, field
    a, keep = _valid_args(L)
    last = keep["t"].items[1]
    a.weights_bytes = last.yc_off + 4 * last.h * last.yk - 1    # one byte short of the last image's y weights
    assert call(a) == EWORKSPACE
    a, keep = _valid_args(L)
    keep["t"].items[1].u8_off = -16
    assert call(a) == EWORKSPACE
    assert lib.dfw_version() >= 106


def test_discriminating_input_discriminates():
    """The input of the GPU tests separates the rule from its plausible misreadings, computed here with Pillow and torch:
    maxima taken before the resize, the batch maximum, labels made at the processing size and resized, a tie given to the
    higher class."""
    x = nn.discriminating_input()
    assert tuple(x.shape) == (4, 2, 3) + nn.DISC_SRC
    r = nn.nway_native_ref(x, nn.DISC_SIZES)
    assert r["mx"].tolist() == [[225, 255], [137, 199], [93, 215], [225, 255]]
    src_mx = nway_ref.maxima(x)
    assert src_mx.tolist() == [[200, 230], [120, 180], [93, 217], [200, 230]]
    res = nn.resized(x, nn.DISC_SIZES)
    thr_src = nn.thresholds(src_mx)
    before = nn.labels_of([res[c][0] for c in range(4)], thr_src[:, 0])
    assert int((before != r["labels"][0]).sum()) == 14
    bm = nn.nway_native_ref(x, nn.DISC_SIZES, batch_max=True)
    assert int((bm["labels"][0] != r["labels"][0]).sum()) == 292
    small = nway_ref.labels(x)                                          # the rule at 32 x 32 ...
    diff = []
    for i, hw in enumerate(nn.DISC_SIZES):                              # ... and the label map resized (nearest)
        up = torch.nn.functional.interpolate(small[i][None, None].float(), size=hw, mode="nearest")[0, 0].to(torch.uint8)
        diff.append(int((up != r["labels"][i]).sum()))
    assert diff == [112, 41]
    for lab in r["labels"]:
        assert not bool((lab == 4).any()) and bool((lab == 1).any())    # class 3 copies class 0: the tie goes to class 0
    assert torch.bincount(r["labels"][0].flatten().long(), minlength=5).tolist() == [510, 352, 545, 643, 0]


def test_one_class_is_the_binary_native_reference():
    """N = 1, 0/1/255 masks, ignore_value 255: labels and counts are native_ref's pred and counts in the three modes."""
    g = torch.Generator().manual_seed(8)
    sizes = [(41, 50), (23, 37), (32, 32)]
    seg = (torch.rand(3, 3, 32, 32, generator=g) * 256).to(torch.uint8)
    seg[0] = nr.overshoot_image()[0]
    seg[1] //= 3
    rs = np.random.RandomState(2)
    gts = []
    for h, w in sizes:
        m = (rs.rand(h, w) > 0.5).astype(np.uint8)
        m[rs.rand(h, w) < 0.07] = 255
        gts.append(m)
    for r_thr, thr, bmax in ((0.25, 0.0, False), (0.25, 0.0, True), (0.0, 0.5, False)):
        want = nr.native_ref(seg, sizes, gts, 1, 255, r_thr, thr, bmax)
        got = nn.nway_native_ref(seg[None], sizes, gts, None, 255, r_thr, thr, bmax)
        assert got["mx"][0].tolist() == want["mx"]
        for i in range(len(sizes)):
            assert torch.equal(got["labels"][i], want["pred"][i]), (r_thr, thr, bmax, i)
            assert torch.equal(got["seg_u8"][i][0], want["seg_u8"][i])
        assert torch.equal(got["counts"].view(len(sizes), 4), want["counts"]), (r_thr, thr, bmax)


def test_reference_ground_truth_mapping():
    """Ids -> labels: the ignore value first, then either the id itself (outside 0..N dropped) or the class-id table (lowest
    class on a duplicate id, everything else background, an id above 255 included)."""
    ids = np.array([[0, 1, 2, 3, 255, 7, 300, -1]], np.int64)
    assert nn.target_map(ids, 2, None, 255).tolist() == [[0, 1, 2, 255, 255, 255, 255, 255]]
    assert nn.target_map(ids, 2, None, -1).tolist() == [[0, 1, 2, 255, 255, 255, 255, 255]]
    assert nn.target_map(ids, 3, [7, 300, 7], 255).tolist() == [[0, 0, 0, 0, 255, 1, 2, 0]]
    assert nn.target_map(ids, 3, [255, 0, 3], -1).tolist() == [[2, 0, 0, 3, 1, 0, 0, 0]]
