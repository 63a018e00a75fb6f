"""CPU tests of the native-size stage: the library's bicubic weights against Pillow itself, the bilinear weights unchanged,
the CPU reference (tests/native_ref.py) tied to the S x S path's definition, the overshoot input the GPU tests rely on,
dfw_seg_native's host-side validation (no launch, no GPU) and the NativeTargets staging layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import native_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BILINEAR, BICUBIC = 0, 1
EINVAL, ESHAPE, ERANGE, EWORKSPACE = -1, -2, -3, -4
PB = 22

# (Hs, Ws) -> (h, w)
PAIRS = [((64, 64), (37, 83)), ((64, 64), (128, 96)), ((64, 64), (64, 50)), ((64, 64), (23, 64)), ((64, 64), (9, 200)),
         ((64, 64), (1, 1)), ((64, 64), (64, 64)), ((40, 72), (333, 500))]


@pytest.fixture(scope="module")
def lib():
    from diffews_amd import build, _lib
    build.build()
    return _lib.lib()


def _coeffs(lib, n_in, n_out, filt):
    k = lib.dfw_resample_ksize_ex(n_in, n_out, filt)
    b = np.zeros((n_out, 2), np.int32)
    w = np.zeros((n_out, k), np.int32)
    assert lib.dfw_resample_coeffs_ex(n_in, n_out, filt, b.ctypes.data, w.ctypes.data) == 0
    return b, w, k


def _pass(a, b, w):
    """Fixed-point pass along axis 1 of uint8 [R, n]: Pillow's ImagingResampleHorizontal_8bpc."""
    out = np.zeros((a.shape[0], b.shape[0]), np.uint8)
    for xx in range(b.shape[0]):
        x0, n = int(b[xx, 0]), int(b[xx, 1])
        acc = (1 << (PB - 1)) + (a[:, x0:x0 + n].astype(np.int64) * w[xx, :n].astype(np.int64)).sum(1)
        out[:, xx] = np.clip(acc >> PB, 0, 255)
    return out


def _resize(lib, a, h, w):
    """Horizontal then vertical pass with a uint8 intermediate, every axis through the library's weights (the identity
    included: no special case)."""
    xb, xw, _ = _coeffs(lib, a.shape[1], w, BICUBIC)
    yb, yw, _ = _coeffs(lib, a.shape[0], h, BICUBIC)
    t = _pass(a, xb, xw)
    return _pass(np.ascontiguousarray(t.T), yb, yw).T


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in PAIRS])
def test_bicubic_weights_reproduce_pillow(lib, src, dst):
    rs = np.random.RandomState(src[0] * 1000 + dst[1])
    for kind in ("random", "binary"):
        a = (rs.rand(*src) * 256).astype(np.uint8) if kind == "random" else ((rs.rand(*src) > 0.6) * 255).astype(np.uint8)
        got = _resize(lib, a, *dst)
        for ref in (Image.fromarray(a).resize((dst[1], dst[0])), Image.fromarray(a).resize((dst[1], dst[0]), Image.BICUBIC)):
            assert np.array_equal(got, np.asarray(ref)), (kind, src, dst, int((got != np.asarray(ref)).sum()))


def test_bilinear_unchanged_and_ksize_known_answers(lib):
    for n_in, n_out in [(64, 64), (640, 512), (427, 512), (100, 512), (1, 7), (7, 1), (512, 37), (333, 64), (64, 333)]:
        k = lib.dfw_resample_ksize(n_in, n_out)
        assert lib.dfw_resample_ksize_ex(n_in, n_out, BILINEAR) == k
        b0 = np.zeros((n_out, 2), np.int32)
        w0 = np.zeros((n_out, k), np.int32)
        assert lib.dfw_resample_coeffs(n_in, n_out, b0.ctypes.data, w0.ctypes.data) == 0
        b1, w1, _ = _coeffs(lib, n_in, n_out, BILINEAR)
        assert np.array_equal(b0, b1) and np.array_equal(w0, w1), (n_in, n_out)
    assert lib.dfw_resample_ksize_ex(64, 128, BICUBIC) == 5
    assert lib.dfw_resample_ksize_ex(64, 23, BICUBIC) == 13
    assert lib.dfw_resample_ksize_ex(64, 64, 2) == 0 and lib.dfw_resample_ksize_ex(0, 64, BICUBIC) == 0
    dummy = np.zeros(16, np.int32)
    assert lib.dfw_resample_coeffs_ex(4, 1, 2, dummy.ctypes.data, dummy.ctypes.data) == EINVAL
    assert lib.dfw_version() >= 105


def test_reference_at_processing_size_is_the_current_definition():
    """h = w = S, 0/1/255 ground truth: native_ref == the launcher expressions on seg_u8 itself (what seg_postprocess is
    tested against), for the three thresholding modes."""
    from oracle.metrics import classify_prediction
    S, b = 64, 3
    g = torch.Generator().manual_seed(5)
    seg = (torch.rand(b, 3, S, S, generator=g) * 256).to(torch.uint8)
    seg[1] //= 3
    gt = (torch.rand(b, S, S, generator=g) > 0.5).to(torch.uint8)
    gt[torch.rand(b, S, S, generator=g) < 0.05] = 255
    for r_thr, thr, bmax in ((0.25, 0.0, False), (0.25, 0.0, True), (0.0, 0.5, False)):
        ref = nr.native_ref(seg, [(S, S)] * b, [x.numpy() for x in gt], 1, 255, r_thr, thr, bmax)
        x = seg.to(torch.float32).div(255)                       # to_tensor
        for i in range(b):
            assert torch.equal(ref["seg_u8"][i], seg[i])
            if r_thr > 0:
                pred = x[i].mean(dim=0) > (x.max() if bmax else x[i].max()) * r_thr
            else:
                pred = x[i].mean(dim=0) > thr
            inter, union = classify_prediction(pred.to(torch.uint8)[None], (gt[i] == 1).to(torch.uint8)[None],
                                               (gt[i] == 255).to(torch.uint8)[None])
            assert torch.equal(ref["pred"][i], pred.to(torch.uint8))
            assert ref["counts"][i].tolist() == [int(v) for v in torch.cat([inter[:, 0], union[:, 0]])]


def test_overshoot_input_separates_the_two_maximum_rules():
    a = nr.overshoot_image()
    assert tuple(a.shape[-2:]) == nr.OVERSHOOT_SRC and sorted(set(a.flatten().tolist())) == [0, 200]
    r = nr.resize_u8(a[0], *nr.OVERSHOOT_SIZE)
    assert int(r.max()) == 225
    x = nr.to_tensor(r.permute(1, 2, 0).numpy())
    after = nr.predict(x, 0.25, 0.0)
    before = nr.predict(x, 0.25, 0.0, mx=torch.tensor(200, dtype=torch.float32).div(255))
    assert int((after != before).sum()) >= 1
    assert torch.equal(nr.native_ref(a, [nr.OVERSHOOT_SIZE])["pred"][0], after.to(torch.uint8))


def _valid_args(L, sizes=((37, 83), (64, 64)), src=(64, 64), with_gt=True):
    """A fully valid dfw_seg_native call on host memory (never launched: every test below breaks one thing)."""
    from diffews_amd.input_pipeline import NativeTargets
    gts = [np.zeros(s, np.uint8) for s in sizes] if with_gt else None
    t = NativeTargets(src, sizes, gt=gts, device=None)
    keep = dict(t=t, seg=np.zeros((len(sizes), 3) + tuple(src), np.uint8), tmp=np.zeros(t.tmp_bytes, np.uint8),
                u8=np.zeros(t.u8_bytes, np.uint8), pred=np.zeros(t.pred_bytes, np.uint8),
                mx=np.zeros(len(sizes), np.uint32), counts=np.zeros((len(sizes), 4), np.int64))
    a = L.SegNativeArgs()
    a.seg_u8, a.B, a.Hs, a.Ws = keep["seg"].ctypes.data, len(sizes), src[0], src[1]
    a.items = a.items_host = C.addressof(t.items)
    a.weights, a.weights_bytes = t.host.ctypes.data, t.host.nbytes
    a.gt, a.gt_bytes = (t.host.ctypes.data, t.host.nbytes) if with_gt else (None, 0)
    a.tmp, a.tmp_bytes, a.tmp_res_off = keep["tmp"].ctypes.data, t.tmp_bytes, t.tmp_bytes
    a.out_u8, a.out_u8_bytes = keep["u8"].ctypes.data, t.u8_bytes
    a.pred, a.pred_bytes = keep["pred"].ctypes.data, t.pred_bytes
    a.mx, a.counts = keep["mx"].ctypes.data, keep["counts"].ctypes.data if with_gt else None
    a.r_threshold, a.threshold, a.batch_max = 0.25, 0.0, 0
    return a, keep


def test_seg_native_validates_on_the_host_before_any_launch(lib):
    from diffews_amd import _lib as L
    call = lambda a: lib.dfw_seg_native(C.byref(a), None)
    assert lib.dfw_seg_native(None, None) == EINVAL
    for field in ("seg_u8", "items", "items_host", "weights", "tmp"):
        a, keep = _valid_args(L)
        setattr(a, field, None)
        assert call(a) == EINVAL, field
    a, keep = _valid_args(L)
    a.gt = None                                         # counts without a ground truth
    assert call(a) == EINVAL
    a, keep = _valid_args(L)
    a.mx = None                                         # dynamic threshold without the maxima
    assert call(a) == EINVAL
    a, keep = _valid_args(L)
    a.r_threshold = 0.0                                 # neither thresholding flag
    assert call(a) == EINVAL
    a, keep = _valid_args(L, with_gt=False)
    a.out_u8 = a.pred = a.mx = None                     # nothing to produce
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
    for field in ("tmp_bytes", "out_u8_bytes", "pred_bytes", "gt_bytes"):
        a, keep = _valid_args(L)
        setattr(a, field, getattr(a, field) - 16)       # the last image no longer fits (sizes end within 15 bytes of it)
        assert call(a) == EWORKSPACE, field
    a, keep = _valid_args(L)
    last = keep["t"].items[1]
    a.weights_bytes = last.yc_off + 4 * last.h * last.yk - 1    # one byte short of the last image's y weights
    assert call(a) == EWORKSPACE
    a, keep = _valid_args(L)
    keep["t"].items[1].u8_off = -16
    assert call(a) == EWORKSPACE


def test_native_structs_match_header_and_compiler(tmp_path):
    """NativeItem / SegNativeArgs mirror dfw_native_item / dfw_seg_native_args field for field and in size."""
    import subprocess
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    pairs = (("dfw_native_item", L.NativeItem), ("dfw_seg_native_args", L.SegNativeArgs))
    for cname, cls in pairs:
        body = re.search(r"typedef struct \{([^{}]*)\}\s*" + cname + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            parts = decl.strip().replace("*", " ").replace(",", " ").split()
            names += [p for p in parts if p not in ("const", "void", "float", "int32_t", "int64_t", "size_t", "uint8_t", "uint32_t")]
        assert names == [f[0] for f in cls._fields_], cname
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", sizeof({n}));' for n, _ in pairs) + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [C.sizeof(c) for _, c in pairs]


def test_native_targets_staging_layout():
    """Mixed batch (odd sizes, uint8 and int32 ground truth, guards): every offset 16-byte aligned, no two regions of one
    buffer overlap, the staged bytes are the table / weights / ground truth; bad sizes and shapes are rejected."""
    from diffews_amd import _lib as L
    from diffews_amd.input_pipeline import NativeTargets, resample_coeffs
    sizes = [(97, 131), (23, 37), (64, 50), (64, 64), (1, 7)]
    rs = np.random.RandomState(3)
    gts = [rs.randint(0, 9, s).astype(np.uint8 if i % 2 else np.int64) for i, s in enumerate(sizes)]
    Hs, Ws, guard = 40, 72, 64
    t = NativeTargets((Hs, Ws), sizes, gt=gts, class_value=[7, 1, 2, 3, 4], ignore_value=255, device=None, guard=guard)
    assert t.b == 5 and t.dev is None and t.host.nbytes == t.total and t.has_gt
    staged, tmp, u8, pr = [(0, C.sizeof(t.items))], [], [], []
    for it, (h, w), g, cv in zip(t.items, sizes, gts, [7, 1, 2, 3, 4]):
        assert (it.h, it.w, it.class_value, it.ignore_value) == (h, w, cv, 255)
        assert it.xk == L.lib().dfw_resample_ksize_ex(Ws, w, BICUBIC) and it.yk == L.lib().dfw_resample_ksize_ex(Hs, h, BICUBIC)
        assert it.gt_elem == (1 if g.dtype == np.uint8 else 4)
        staged += [(it.xb_off, 8 * w), (it.xc_off, 4 * w * it.xk), (it.yb_off, 8 * h), (it.yc_off, 4 * h * it.yk),
                   (it.gt_off, h * w * it.gt_elem)]
        tmp.append((it.tmp_off, 3 * Hs * w + guard))
        u8.append((it.u8_off, 3 * h * w + guard))
        pr.append((it.pred_off, h * w + guard))
        xb, xw, _ = resample_coeffs(Ws, w, BICUBIC)
        yb, yw, _ = resample_coeffs(Hs, h, BICUBIC)
        for off, arr in ((it.xb_off, xb), (it.xc_off, xw), (it.yb_off, yb), (it.yc_off, yw),
                         (it.gt_off, g if g.dtype == np.uint8 else g.astype(np.int32))):
            assert bytes(t.host[off:off + arr.nbytes]) == arr.tobytes()
    assert bytes(t.host[:C.sizeof(t.items)]) == bytes(t.items)
    for regions, cap in ((staged, t.total), (tmp, t.tmp_bytes), (u8, t.u8_bytes), (pr, t.pred_bytes)):
        assert all(o % 16 == 0 and o >= 0 for o, _ in regions)
        regions = sorted(regions)
        assert all(o0 + n0 <= o1 for (o0, n0), (o1, _) in zip(regions, regions[1:]))
        assert regions[-1][0] + regions[-1][1] <= cap
    for bad in ([(0, 5)], [(5, 0)], [(4, -1)], []):
        with pytest.raises(ValueError):
            NativeTargets((64, 64), bad, device=None)
    with pytest.raises(ValueError, match="shape"):
        NativeTargets((64, 64), [(5, 6)], gt=[np.zeros((6, 5), np.uint8)], device=None)
    with pytest.raises(ValueError):
        NativeTargets((64, 64), [(5, 6), (5, 6)], gt=[np.zeros((5, 6), np.uint8)], device=None)
