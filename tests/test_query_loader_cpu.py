"""CPU tests of the batched input transform and the query stream loader: the three new structs against the header and the
compiler, dfw_inputs_to_tensor's host-side validation (no launch, no GPU), the staging layout of
DeviceImageTransform.batch and of a QueryLoader batch in their host-only mode, and a numpy emulation of the two device
tables run over the staged bytes against Pillow and torch themselves (exact)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import query_loader_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE, ERANGE, EWORKSPACE = -1, -2, -3, -4
PB = 22


@pytest.fixture(scope="module")
def lib():
    from diffews_amd import build, _lib
    build.build()
    return _lib.lib()


def test_input_structs_match_header_and_compiler(lib, tmp_path):
    from diffews_amd import _lib as L
    assert lib.dfw_version() >= 107
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    pairs = (("dfw_input_image_item", L.InputImageItem), ("dfw_input_mask_item", L.InputMaskItem),
             ("dfw_inputs_args", L.InputsArgs))
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
    assert "dfw_inputs_to_tensor" in L.SYMBOLS


# ------------------------------------------------------------------------------------------------ validation

def _valid_args(images=True, masks=True):
    """A fully valid dfw_inputs_to_tensor call on host memory (never launched: every test below breaks one thing).
    Two images (9 x 13, 20 x 7) and three maps: uint8 -> +-1 and 0/1, int32 -> 0/1 only, uint8 -> +-1 only."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    rs = np.random.RandomState(1)
    ims = [rs.randint(0, 256, (9, 13, 3)).astype(np.uint8), rs.randint(0, 256, (20, 7, 3)).astype(np.uint8)] if images else []
    mks = [rs.randint(0, 4, (9, 13)).astype(np.uint8), rs.randint(0, 4, (20, 7)).astype(np.int32),
           rs.randint(0, 4, (5, 6)).astype(np.uint8)] if masks else []
    lay = DeviceImageTransform((16, 24), device=None).batch(ims, mks, [1, 2, 3][:len(mks)], want_pm1=[True, False, True][:len(mks)],
                                                            want_bin=[True, True, False][:len(mks)])
    keep = dict(lay=lay, tmp=np.zeros(max(lay.tmp_bytes, 16), np.uint8), dst=np.zeros(max(lay.dst_bytes, 16), np.uint8),
                pm1=np.zeros(max(lay.pm1_bytes, 16), np.uint8), bin=np.zeros(max(lay.bin_bytes, 16), np.uint8),
                lut=np.zeros(256, np.float32))
    pair = lambda k, n: (keep[k].ctypes.data, n)
    a = lay.args(lay.host.ctypes.data, lay.total, keep["lut"].ctypes.data, pair("tmp", lay.tmp_bytes), pair("dst", lay.dst_bytes),
                 pair("pm1", lay.pm1_bytes), pair("bin", lay.bin_bytes))
    return a, keep


def test_inputs_to_tensor_validates_on_the_host_before_any_launch(lib):
    call = lambda a: lib.dfw_inputs_to_tensor(C.byref(a), None)
    img = lambda keep, i: keep["lay"].img_items[i]
    msk = lambda keep, j: keep["lay"].mask_items[j]
    # ---- DFW_EINVAL
    assert lib.dfw_inputs_to_tensor(None, None) == EINVAL
    for field in ("image_items", "image_items_host", "mask_items", "mask_items_host", "staged", "tmp", "dst", "lut", "pm1", "bin"):
        a, keep = _valid_args()
        setattr(a, field, None)
        assert call(a) == EINVAL, field
    for field in ("out_h", "out_w"):
        for bad in (0, -2):
            a, keep = _valid_args()
            setattr(a, field, bad)
            assert call(a) == EINVAL, field
    a, keep = _valid_args()
    a.n_img = a.n_mask = 0                                # nothing to do
    assert call(a) == EINVAL
    for field in ("n_img", "n_mask"):
        a, keep = _valid_args()
        setattr(a, field, -1)
        assert call(a) == EINVAL, field
    for field in ("H", "W"):
        for bad in (0, -3):
            a, keep = _valid_args()
            setattr(img(keep, 1), field, bad)
            assert call(a) == EINVAL, ("image", field)
            a, keep = _valid_args()
            setattr(msk(keep, 2), field, bad)
            assert call(a) == EINVAL, ("mask", field)
    for bad in (0, 2, 8):
        a, keep = _valid_args()
        msk(keep, 0).elem = bad
        assert call(a) == EINVAL, bad
    a, keep = _valid_args()
    msk(keep, 1).bin_off = -1                             # the int32 map had 0/1 only: now neither destination
    assert call(a) == EINVAL
    # ---- DFW_ESHAPE
    for field in ("xk", "yk"):
        a, keep = _valid_args()
        setattr(img(keep, 0), field, getattr(img(keep, 0), field) + 1)
        assert call(a) == ESHAPE, field
    a, keep = _valid_args()
    a.out_w = 3                                           # the x weights were made for out_w = 24: other ksize
    assert call(a) == ESHAPE
    for field in ("xb_off", "xc_off", "yb_off", "yc_off", "dst_off"):
        a, keep = _valid_args()
        setattr(img(keep, 1), field, getattr(img(keep, 1), field) + 2)
        assert call(a) == ESHAPE, field
    a, keep = _valid_args()
    msk(keep, 1).src_off += 2                             # int32 ids
    assert call(a) == ESHAPE
    a, keep = _valid_args()
    msk(keep, 0).pm1_off += 2
    assert call(a) == ESHAPE
    a, keep = _valid_args()
    msk(keep, 0).src_off += 1                             # uint8 ids need no alignment: only the extent is checked
    a.staged_bytes = msk(keep, 0).src_off + 9 * 13 - 1
    assert call(a) == EWORKSPACE
    # ---- DFW_ERANGE
    a, keep = _valid_args()
    img(keep, 0).H = 65536
    assert call(a) == ERANGE
    for field in ("out_h", "n_img", "n_mask"):
        a, keep = _valid_args()
        setattr(a, field, 65536)
        assert call(a) == ERANGE, field
    # ---- DFW_EWORKSPACE
    a, keep = _valid_args()
    last = img(keep, 1)
    a.tmp_bytes = last.tmp_off + 3 * last.H * a.out_w - 1             # the last image's tmp extent overruns by one byte
    assert call(a) == EWORKSPACE
    a, keep = _valid_args()
    plane = 4 * a.out_h * a.out_w
    img(keep, 1).dst_off = a.dst_bytes - 3 * plane + 4                # two planes fit, the last one leaves dst
    assert call(a) == EWORKSPACE
    a, keep = _valid_args()
    img(keep, 1).dst_off = a.dst_bytes - 2 * plane                    # the whole last plane lies outside
    assert call(a) == EWORKSPACE
    a, keep = _valid_args()
    a.staged_bytes = msk(keep, 2).src_off + 5 * 6 - 1                 # one byte short of the last map's ids
    assert call(a) == EWORKSPACE
    a, keep = _valid_args()
    a.staged_bytes = img(keep, 1).yc_off + 4 * a.out_h * img(keep, 1).yk - 1     # ... of the last image's y weights
    assert call(a) == EWORKSPACE
    for field in ("dst_bytes", "pm1_bytes", "bin_bytes"):             # dense outputs: the last item ends with its buffer
        a, keep = _valid_args()
        setattr(a, field, getattr(a, field) - 1)
        assert call(a) == EWORKSPACE, field
    for field in ("src_off", "xb_off", "xc_off", "yb_off", "yc_off", "tmp_off", "dst_off"):
        a, keep = _valid_args()
        setattr(img(keep, 0), field, -16)
        assert call(a) == EWORKSPACE, field
        a, keep = _valid_args()
        setattr(img(keep, 0), field, 1 << 40)
        assert call(a) == EWORKSPACE, field
    for j, field in ((0, "src_off"), (0, "pm1_off"), (1, "bin_off")):
        a, keep = _valid_args()
        setattr(msk(keep, j), field, -16)
        assert call(a) == EWORKSPACE, field
    a, keep = _valid_args()
    msk(keep, 2).pm1_off = a.pm1_bytes - 3 * plane + 4
    assert call(a) == EWORKSPACE
    # the images-only and masks-only calls need only their own pointers, and are checked like the full one
    a, keep = _valid_args(masks=False)
    assert a.n_mask == 0 and not a.pm1_bytes and not a.bin_bytes
    a.mask_items = a.mask_items_host = a.pm1 = a.bin = None
    a.tmp_bytes = img(keep, 1).tmp_off + 3 * img(keep, 1).H * a.out_w - 1
    assert call(a) == EWORKSPACE
    a, keep = _valid_args(images=False)
    assert a.n_img == 0
    a.image_items = a.image_items_host = a.tmp = a.dst = a.lut = None
    a.bin_bytes -= 1
    assert call(a) == EWORKSPACE


# ------------------------------------------------------------------------------------------------ layout

def _regions_ok(regions, cap):
    assert all(o % 16 == 0 and o >= 0 for o, _ in regions), regions
    regions = sorted(regions)
    assert all(o0 + n0 <= o1 for (o0, n0), (o1, _) in zip(regions, regions[1:])), regions
    assert regions[-1][0] + regions[-1][1] <= cap


def _check_layout(lay, images, masks, guard):
    """Every offset 16-byte aligned, the regions of each buffer pairwise disjoint and inside it, tmp regions 3 * H * out_w,
    the staged bytes are the tables / images / weights / ids."""
    from diffews_amd import _lib as L
    from diffews_amd.input_pipeline import resample_coeffs
    oh, ow = lay.out_hw
    assert lay.n_img == len(images) and lay.host.nbytes >= lay.total
    staged = [(lay.img_table_off, C.sizeof(L.InputImageItem) * lay.n_img)]
    if lay.n_mask:
        staged.append((lay.mask_table_off, C.sizeof(L.InputMaskItem) * lay.n_mask))
    tmp, dst, pm1, bn = [], [], [], []
    for it, im in zip(lay.img_items, images):
        H, W = im.shape[:2]
        assert (it.H, it.W) == (H, W)
        assert it.xk == L.lib().dfw_resample_ksize(W, ow) and it.yk == L.lib().dfw_resample_ksize(H, oh)
        xb, xw, _ = resample_coeffs(W, ow)
        yb, yw, _ = resample_coeffs(H, oh)
        for off, arr in ((it.src_off, im), (it.xb_off, xb), (it.xc_off, xw), (it.yb_off, yb), (it.yc_off, yw)):
            staged.append((off, arr.nbytes))
            assert bytes(lay.host[off:off + arr.nbytes]) == arr.tobytes()
        tmp.append((it.tmp_off, 3 * H * ow + guard))
        dst.append((it.dst_off, 12 * oh * ow + guard))
    assert len(lay.mask_src) == len(masks)
    for (off, elem), m in zip(lay.mask_src, masks):
        m = m if m.dtype == np.uint8 else m.astype(np.int32)
        assert elem == m.dtype.itemsize
        staged.append((off, m.nbytes))
        assert bytes(lay.host[off:off + m.nbytes]) == m.tobytes()
    for it in lay.mask_items[:lay.n_mask]:
        assert (it.src_off, it.elem) in lay.mask_src
        if it.pm1_off != -1:
            pm1.append((it.pm1_off, 12 * oh * ow + guard))
        if it.bin_off != -1:
            bn.append((it.bin_off, oh * ow + guard))
    n = C.sizeof(L.InputImageItem) * lay.n_img
    assert bytes(lay.host[:n]) == bytes(lay.img_items)[:n]
    n = C.sizeof(L.InputMaskItem) * lay.n_mask
    assert bytes(lay.host[lay.mask_table_off:lay.mask_table_off + n]) == bytes(lay.mask_items)[:n]
    for regions, cap in ((staged, lay.total), (tmp, lay.tmp_bytes), (dst, lay.dst_bytes), (pm1, lay.pm1_bytes), (bn, lay.bin_bytes)):
        if regions:
            _regions_ok(regions, cap)
    return len(pm1), len(bn)


@pytest.mark.parametrize("out_hw", qr.OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("guard", [0, 64])
def test_batch_host_layout(lib, out_hw, guard):
    from diffews_amd.input_pipeline import DeviceImageTransform
    d = qr.ragged(out_hw)
    tf = DeviceImageTransform(out_hw if out_hw[0] != out_hw[1] else out_hw[0], device=None)
    assert (tf.out_h, tf.out_w) == out_hw
    lay = tf.batch(d["images"], d["masks"], d["mask_class"], d["want_pm1"], d["want_bin"], guard=guard)
    n_pm1, n_bin = _check_layout(lay, d["images"], d["masks"], guard)
    assert lay.n_mask == len(d["masks"]) and n_pm1 == sum(d["want_pm1"]) and n_bin == sum(d["want_bin"])
    for it, cv in zip(lay.mask_items, d["mask_class"]):
        assert it.class_value == cv
    with pytest.raises(ValueError):
        tf.batch(d["images"], d["masks"], d["mask_class"][:-1])
    with pytest.raises(ValueError):
        tf.batch([np.zeros((4, 4), np.uint8)])


def _queries(n, with_gt=True, seed=5):
    rs = np.random.RandomState(seed)
    sizes = [(48, 64), (80, 56), (64, 64), (23, 37), (97, 131)]
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        q = dict(query_img=rs.randint(0, 256, (h, w, 3)).astype(np.uint8), cls=[3, 7][i % 2])
        if with_gt:
            q["gt"] = rs.choice([0, 3, 7, 255], size=(h, w)).astype(np.uint8 if i % 2 == 0 else np.int64)
        out.append(q)
    return out


@pytest.mark.parametrize("class_value", [None, 7, "callable"])
def test_query_loader_host_layout(lib, class_value):
    """A QueryLoader batch in host-only mode: InputBatch's layout, and `native` reads the ground truth IN PLACE -- its gt
    offsets are the staged map bytes; without class_value the maps are staged only (no mask item, no mask launch)."""
    from diffews_amd.input_pipeline import QueryLoader
    qs = _queries(5)
    cv = (lambda q: q["cls"]) if class_value == "callable" else class_value
    ld = QueryLoader(qs, 64, 5, device=None, class_value=cv, ignore_value=255)
    lay, native = ld.host_batch(qs)
    images, gts = [q["query_img"] for q in qs], [q["gt"] for q in qs]
    _check_layout(lay, images, gts, 0)
    assert lay.n_mask == (0 if class_value is None else 5)
    assert native.b == 5 and native.has_gt and native.sizes == [g.shape for g in gts] and native.src_hw == (64, 64)
    want_cls = {None: [1] * 5, 7: [7] * 5, "callable": [q["cls"] for q in qs]}[class_value]
    for it, (off, elem), g, c in zip(native.items, lay.mask_src, gts, want_cls):
        assert (it.gt_off, it.gt_elem) == (off, elem) and it.gt_off % 16 == 0
        assert (it.class_value, it.ignore_value) == (c, 255)
        g = g if g.dtype == np.uint8 else g.astype(np.int32)
        assert bytes(lay.host[it.gt_off:it.gt_off + it.h * it.w * it.gt_elem]) == g.tobytes()
    for it, c in zip(lay.mask_items[:lay.n_mask], want_cls):
        assert it.class_value == c and it.pm1_off == -1 and it.bin_off % 16 == 0
    # no ground truth: sizes only
    lay, native = QueryLoader([], 64, 3, device=None).host_batch(_queries(3, with_gt=False))
    assert lay.n_mask == 0 and lay.mask_src == [] and not native.has_gt and native.b == 3
    mixed = _queries(2)
    del mixed[1]["gt"]
    with pytest.raises(ValueError, match="gt"):
        ld.host_batch(mixed)
    bad = _queries(1)
    bad[0]["gt"] = bad[0]["gt"][:-1]
    with pytest.raises(ValueError, match="size"):
        ld.host_batch(bad)


# ------------------------------------------------------------------------------------------------ numpy emulation

def _emulate(lay, lut):
    """What the three launches compute, in numpy, from NOTHING but the staged bytes: the tables are read back from the
    buffer, every image and map through the offsets of its item."""
    from diffews_amd import _lib as L
    host, (oh, ow) = lay.host, lay.out_hw
    i32 = lambda off, n: np.frombuffer(host, np.int32, n, off)
    items = (L.InputImageItem * max(lay.n_img, 1)).from_buffer_copy(bytes(host[:C.sizeof(L.InputImageItem) * max(lay.n_img, 1)]))
    images = []
    for it in items[:lay.n_img]:
        src = np.frombuffer(host, np.uint8, it.H * it.W * 3, it.src_off).reshape(it.H, it.W, 3).astype(np.int64)
        xb, xc = i32(it.xb_off, 2 * ow).reshape(ow, 2), i32(it.xc_off, ow * it.xk).reshape(ow, it.xk).astype(np.int64)
        yb, yc = i32(it.yb_off, 2 * oh).reshape(oh, 2), i32(it.yc_off, oh * it.yk).reshape(oh, it.yk).astype(np.int64)
        tmp = np.zeros((it.H, ow, 3), np.int64)
        for xo in range(ow):
            x0, n = int(xb[xo, 0]), int(xb[xo, 1])
            acc = (1 << (PB - 1)) + (src[:, x0:x0 + n] * xc[xo, :n, None]).sum(1)
            tmp[:, xo] = np.clip(acc >> PB, 0, 255)
        out = np.zeros((oh, ow, 3), np.int64)
        for yo in range(oh):
            y0, n = int(yb[yo, 0]), int(yb[yo, 1])
            acc = (1 << (PB - 1)) + (tmp[y0:y0 + n] * yc[yo, :n, None, None]).sum(0)
            out[yo] = np.clip(acc >> PB, 0, 255)
        images.append(lut[torch.from_numpy(out).permute(2, 0, 1)])
    raw = bytes(host[lay.mask_table_off:lay.mask_table_off + C.sizeof(L.InputMaskItem) * max(lay.n_mask, 1)])
    mitems = (L.InputMaskItem * max(lay.n_mask, 1)).from_buffer_copy(raw)
    pm1, bn = {}, {}
    for it in mitems[:lay.n_mask]:
        ids = np.frombuffer(host, np.uint8 if it.elem == 1 else np.int32, it.H * it.W, it.src_off).reshape(it.H, it.W)
        sy, sx = np.float32(it.H) / np.float32(oh), np.float32(it.W) / np.float32(ow)
        iy = np.minimum(np.floor(np.arange(oh, dtype=np.float32) * sy).astype(np.int64), it.H - 1)
        ix = np.minimum(np.floor(np.arange(ow, dtype=np.float32) * sx).astype(np.int64), it.W - 1)
        on = ids[iy][:, ix].astype(np.int64) == it.class_value
        if it.pm1_off != -1:
            pm1[it.pm1_off] = np.where(on, np.float32(1), np.float32(-1))[None].repeat(3, 0)
        if it.bin_off != -1:
            bn[it.bin_off] = on.astype(np.uint8)
    return images, pm1, bn


@pytest.mark.parametrize("out_hw", qr.OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tables_over_staged_bytes_reproduce_pillow_and_torch(lib, out_hw):
    from diffews_amd.input_pipeline import DeviceImageTransform
    d = qr.ragged(out_hw)
    tf = DeviceImageTransform(out_hw, device=None)
    lay = tf.batch(d["images"], d["masks"], d["mask_class"], d["want_pm1"], d["want_bin"])
    images, pm1, bn = _emulate(lay, tf.lut)
    for i, (got, ref) in enumerate(zip(images, d["ref_images"])):
        assert torch.equal(got, ref), (i, d["images"][i].shape)
    n_pm1 = n_bin = 0
    for j, ref in enumerate(d["ref_masks"]):
        if d["want_pm1"][j]:
            assert np.array_equal(pm1[n_pm1 * lay.pm1_stride], (ref[None].repeat(3, 1, 1) * 2 - 1).numpy()), j
            n_pm1 += 1
        if d["want_bin"][j]:
            assert np.array_equal(bn[n_bin * lay.bin_stride], ref.to(torch.uint8).numpy()), j
            n_bin += 1
    assert n_pm1 == len(pm1) and n_bin == len(bn)
