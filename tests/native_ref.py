"""CPU reference of the native-size stage (ops.seg_native): what the reference does on the host under
--use_original_imgsize, restated with Pillow and torch themselves.

Per image: `Image.fromarray(hwc).resize((w, h))` with the default filter (marigold_pipeline_rgb_latent_noise.py:539), then
the launcher's expressions (main_oss.py:128-137) -- to_tensor, `max() * r_threshold` or the fixed threshold,
`mean(dim=1) > thr` -- then oracle.metrics.classify_prediction (evaluation.py:12-39) on the native ground truth, with the
foreground `id == class_value` (coco.py:74-75) and the ignore map `id == ignore_value` (pascal.py query_ignore_idx).
"""
import numpy as np
import torch
from PIL import Image

from oracle.metrics import classify_prediction


def to_tensor(img):
    """torchvision.transforms.functional.to_tensor of an RGB uint8 PIL image / HWC array: CHW, float32, / 255."""
    return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def resize_u8(seg_u8_i, h, w):
    """uint8 [3, Hs, Ws] tensor -> uint8 [3, h, w], through Pillow as the reference's pipeline does."""
    hwc = np.ascontiguousarray(seg_u8_i.permute(1, 2, 0).numpy())
    out = np.asarray(Image.fromarray(hwc).resize((w, h)))
    return torch.from_numpy(out.copy()).permute(2, 0, 1).contiguous()


def predict(x, r_threshold, threshold, mx=None):
    """Launcher expressions on x = to_tensor(resized) [3, h, w]; mx overrides x.max() (the batch's maximum)."""
    if r_threshold > 0:
        m = x.max() if mx is None else mx
        return x.mean(dim=0) > m * r_threshold
    return x.mean(dim=0) > threshold


def counts_of(pred, gt, class_value=1, ignore_value=-1):
    """pred bool [h, w], gt integer [h, w] -> int64 [4] = inter0, inter1, union0, union1."""
    gt = torch.as_tensor(np.asarray(gt).astype(np.int64))
    fg = (gt == class_value).to(torch.uint8)
    ign = (gt == ignore_value).to(torch.uint8) if ignore_value >= 0 else None
    inter, union = classify_prediction(pred.to(torch.uint8)[None], fg[None], None if ign is None else ign[None])
    return torch.cat([inter[:, 0], union[:, 0]]).to(torch.int64)


def native_ref(seg_u8, sizes, gts=None, class_values=1, ignore_value=-1, r_threshold=0.25, threshold=0.0, batch_max=False):
    """seg_u8 uint8 [b, 3, Hs, Ws] (CPU) -> dict(seg_u8=[uint8 [3,h,w]], pred=[uint8 [h,w]], counts=int64 [b,4] | None,
    mx=[int])."""
    seg_u8 = seg_u8.cpu()
    b = seg_u8.shape[0]
    cls = [class_values] * b if np.isscalar(class_values) else list(class_values)
    res = [resize_u8(seg_u8[i], h, w) for i, (h, w) in enumerate(sizes)]
    xs = [to_tensor(r.permute(1, 2, 0).numpy()) for r in res]
    bm = torch.stack([x.max() for x in xs]).max() if batch_max else None
    preds = [predict(x, r_threshold, threshold, bm) for x in xs]
    counts = None
    if gts is not None:
        counts = torch.stack([counts_of(p, g, c, ignore_value) for p, g, c in zip(preds, gts, cls)])
    return dict(seg_u8=res, pred=[p.to(torch.uint8) for p in preds], counts=counts, mx=[int(r.max()) for r in res])


OVERSHOOT_SRC, OVERSHOOT_SIZE = (32, 32), (41, 50)


def overshoot_image():
    """uint8 [1, 3, 32, 32]: a 0/200 block whose bicubic resize to 41 x 50 overshoots to 225, placed so that thresholding at
    0.25 x the RESIZED maximum and at 0.25 x the maximum BEFORE the resize give different masks
    (test_native_cpu.test_overshoot_input_separates_the_two_maximum_rules asserts both)."""
    a = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    a[:, :, 2:13, 5:20] = 200
    return a
