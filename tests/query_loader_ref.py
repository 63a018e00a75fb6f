"""Shared by tests/test_query_loader_cpu.py and tests/test_query_loader_gpu.py: the ragged batch both run, and its expected
tensors from the code the reference runs on the host -- PIL.Image.resize(BILINEAR) + ToTensor + Normalize
(evaluation_util/data/dataset.py:36-40) and F.interpolate(nearest) on the binarised class map (coco.py:42,46).  Computed
once per output size and never written."""
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
