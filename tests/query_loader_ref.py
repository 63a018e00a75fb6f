"""Shared by tests/test_query_loader_cpu.py and tests/test_query_loader_gpu.py: the ragged batch both run, and its expected
tensors from the code the reference runs on the host -- PIL.Image.resize(BILINEAR) + ToTensor + Normalize
(evaluation_util/data/dataset.py:36-40) and F.interpolate(nearest) on the binarised class map (coco.py:42,46).  Computed
once per output size and never written.  Also the per-item C entry points (dfw_image_to_tensor / dfw_mask_to_tensor),
which the package itself no longer calls, through ctypes."""
import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

OUT_SIZES = [(64, 64), (48, 300)]       # the second: not square, more than one 256-thread block wide
CLASS_VALUES = (3, 7)


def source_sizes(out_hw):
    """Up- and down-scaling on each axis, the identity, fewer rows than the batch's tallest image, sizes below one block."""
    return [(1, 1), (2, 3), (37, 41), (97, 131), (333, 500), (700, 20), tuple(out_hw)]


def host_image(img_u8, out_hw):
    res = np.asarray(Image.fromarray(img_u8, "RGB").resize((out_hw[1], out_hw[0]), Image.BILINEAR))
    t = torch.from_numpy(res.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return (t - 0.5) / 0.5


def host_mask(ids, value, out_hw):
    """float 0/1 [out_h, out_w]: (ids == value) nearest-resized by ATen."""
    m = (torch.from_numpy(np.asarray(ids).astype(np.int64)) == int(value)).float()
    return F.interpolate(m[None, None], tuple(out_hw), mode="nearest")[0, 0]


@functools.lru_cache(maxsize=None)
def ragged(out_hw):
    """dict(images, masks, mask_class, want_pm1, want_bin, ref_images, ref_masks) for one output size: one image and one
    class-id map per source size; maps alternate uint8 / int32, the two class values, and cycle through +-1 only, 0/1
    only, both."""
    rs = np.random.RandomState(out_hw[0] * 1000 + out_hw[1])
    sizes = source_sizes(out_hw)
    images = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    masks = [rs.choice([0, 3, 3, 7, 9], size=(h, w)).astype(np.uint8 if j % 2 == 0 else np.int32)
             for j, (h, w) in enumerate(sizes)]
    mask_class = [CLASS_VALUES[(j // 2) % 2] for j in range(len(sizes))]
    want_pm1 = [j % 3 != 1 for j in range(len(sizes))]
    want_bin = [j % 3 != 0 for j in range(len(sizes))]
    return dict(images=images, masks=masks, mask_class=mask_class, want_pm1=want_pm1, want_bin=want_bin,
                ref_images=[host_image(im, out_hw) for im in images],
                ref_masks=[host_mask(m, c, out_hw) for m, c in zip(masks, mask_class)])


def _stage_one(arrays, device):
    """One pinned buffer holding `arrays` at 16-byte aligned offsets, one H2D copy -> (device tensor, addresses)."""
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total = (total + a.nbytes + 15) // 16 * 16
    host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
    for o, a in zip(offs, arrays):
        host.numpy()[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    dev = host.to(device, non_blocking=True)
    return dev, [dev.data_ptr() + o for o in offs]


def per_item_image(img_u8, out_hw, lut):
    """dfw_image_to_tensor for one uint8 [H, W, 3] image -> fp32 [3, out_h, out_w] on lut's device."""
    from diffews_amd import _lib as L
    from diffews_amd.input_pipeline import resample_coeffs
    (H, W), (oh, ow) = img_u8.shape[:2], out_hw
    xb, xw, xk = resample_coeffs(W, ow)
    yb, yw, yk = resample_coeffs(H, oh)
    dev, p = _stage_one([np.ascontiguousarray(img_u8), xb, xw, yb, yw], lut.device)
    tmp = torch.empty(H * ow * 3, dtype=torch.uint8, device=lut.device)
    dst = torch.empty(3, oh, ow, dtype=torch.float32, device=lut.device)
    a = L.ImageArgs()
    a.src, a.H, a.W, a.out_h, a.out_w = p[0], H, W, oh, ow
    a.xbounds, a.xcoef, a.xk, a.ybounds, a.ycoef, a.yk = p[1], p[2], xk, p[3], p[4], yk
    a.tmp, a.dst, a.lut = tmp.data_ptr(), dst.data_ptr(), lut.data_ptr()
    L.check(L.lib().dfw_image_to_tensor(C.byref(a), torch.cuda.current_stream(lut.device).cuda_stream), "dfw_image_to_tensor")
    return dst


def per_item_mask(ids, value, out_hw, device, want_pm1=True, want_bin=True):
    """dfw_mask_to_tensor for one uint8 / int32 class-id map -> (fp32 [3, out_h, out_w] in +-1 or None, uint8
    [out_h, out_w] in 0/1 or None)."""
    from diffews_amd import _lib as L
    assert ids.dtype in (np.uint8, np.int32)
    (H, W), (oh, ow) = ids.shape, out_hw
    dev, p = _stage_one([np.ascontiguousarray(ids)], device)
    pm1 = torch.empty(3, oh, ow, dtype=torch.float32, device=device) if want_pm1 else None
    bn = torch.empty(oh, ow, dtype=torch.uint8, device=device) if want_bin else None
    ptr = lambda t: None if t is None else t.data_ptr()
    L.check(L.lib().dfw_mask_to_tensor(p[0], ids.dtype.itemsize, H, W, int(value), oh, ow, ptr(pm1), ptr(bn),
                                       torch.cuda.current_stream(device).cuda_stream), "dfw_mask_to_tensor")
    return pm1, bn
