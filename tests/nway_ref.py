"""Pure-torch reference of the N-way label rule (ops.seg_labels / dfw_seg_labels), on the host, in the kernel's own fp32
expressions -- integer input, one IEEE operation per step, so the comparison with the device is exact.

Input: seg_u8 uint8 [N, B, 3, H, W], the quantised decoded masks of N classes for B query images.
  score_c  = ((u0 / 255 + u1 / 255) + u2 / 255) / 3          fp32, per pixel and class (seg_postprocess' mean)
  thr_c    = (m / 255) * r_threshold   when r_threshold > 0, m = max of class c, image b (batch_max: over class c's B images)
           = threshold                  otherwise
  fg_c     = score_c > thr_c
  label    = 0 when no class is foreground, else 1 + c of the foreground class of the largest score, lowest c on a tie
With gt uint8 [B, H, W] (0..N; 255 and every value above N dropped): counts int64 [B, 2, N+1], row 0 the pixels with
label == gt == l, row 1 pred_l + gt_l - inter_l.
"""
import torch

F32 = torch.float32


def scores(seg_u8):
    """uint8 [N, B, 3, H, W] -> fp32 [N, B, H, W]."""
    lut = torch.arange(256, dtype=F32) / torch.tensor(255.0, dtype=F32)
    u = lut[seg_u8.cpu().long()]
    return ((u[:, :, 0] + u[:, :, 1]) + u[:, :, 2]) / torch.tensor(3.0, dtype=F32)


def maxima(seg_u8):
    """Per class and image maximum byte, int32 [N, B]: what seg_postprocess leaves in its scratch."""
    N, B = seg_u8.shape[:2]
    return seg_u8.cpu().reshape(N, B, -1).amax(-1).to(torch.int32)


def thresholds(seg_u8, r_threshold=0.25, threshold=0.0, batch_max=False):
    """fp32 [N, B]."""
    N, B = seg_u8.shape[:2]
    if not r_threshold > 0:
        return torch.full((N, B), float(threshold), dtype=F32)
    m = maxima(seg_u8)
    if batch_max:
        m = m.amax(1, keepdim=True).expand(N, B)
    return (m.to(F32) / torch.tensor(255.0, dtype=F32)) * torch.tensor(float(r_threshold), dtype=F32)


def foreground(seg_u8, r_threshold=0.25, threshold=0.0, batch_max=False):
    """bool [N, B, H, W]: the binary prediction of every class (seg_postprocess' `pred`)."""
    return scores(seg_u8) > thresholds(seg_u8, r_threshold, threshold, batch_max)[:, :, None, None]


def labels(seg_u8, r_threshold=0.25, threshold=0.0, batch_max=False):
    """uint8 [B, H, W]."""
    sc = scores(seg_u8)
    fg = sc > thresholds(seg_u8, r_threshold, threshold, batch_max)[:, :, None, None]
    best = torch.full(sc.shape[1:], -1.0, dtype=F32)
    lab = torch.zeros(sc.shape[1:], dtype=torch.uint8)
    for c in range(sc.shape[0]):                      # ascending, strictly larger takes over: lowest c wins a tie
        take = fg[c] & (sc[c] > best)
        best = torch.where(take, sc[c], best)
        lab = torch.where(take, torch.full_like(lab, c + 1), lab)
    return lab


def counts(lab, gt, N):
    """labels uint8 [B, H, W], gt uint8 [B, H, W] -> int64 [B, 2, N+1]."""
    lab, gt = lab.cpu().long(), gt.cpu().long()
    B = lab.shape[0]
    out = torch.zeros(B, 2, N + 1, dtype=torch.int64)
    for b in range(B):
        keep = gt[b] <= N
        l, g = lab[b][keep], gt[b][keep]
        pred = torch.bincount(l, minlength=N + 1)
        gth = torch.bincount(g, minlength=N + 1)
        inter = torch.bincount(l[l == g], minlength=N + 1)
        out[b, 0], out[b, 1] = inter, pred + gth - inter
    return out


def seg_labels(seg_u8, gt=None, r_threshold=0.25, threshold=0.0, batch_max=False):
    """(labels uint8 [B, H, W], counts int64 [B, 2, N+1] or None)."""
    lab = labels(seg_u8, r_threshold, threshold, batch_max)
    return lab, (None if gt is None else counts(lab, gt, seg_u8.shape[0]))
