"""Host reference of tiled segmentation (input_pipeline.TilePlan, ops.tiles_cut / ops.tiles_merge), in Python / numpy int64,
written from the definitions and not from the kernel: the kernel GATHERS per output pixel, this SCATTERS every window into
two int64 accumulators and divides once, so the two share no indexing.

Per axis of length L with tile length S and minimum overlap v:  L == S -> one window at 0, otherwise
n = 1 + ceil((L - S) / (S - v)) windows at o_i = (i * (L - S)) // (n - 1).  Windows are numbered row-major.
Weight of pixel (dy, dx) of a th x tw window: min(dy + 1, th - dy, ramp) * min(dx + 1, tw - dx, ramp).
Merged byte: with A = sum w * u and W = sum w over the windows that cover the pixel, (2 A + W) // (2 W): round half up.
"""
import numpy as np


def origins(L, S, overlap):
    """First pixel of every window of one axis."""
    assert L >= S >= 1 and 0 <= overlap <= S // 2
    if L == S:
        return [0]
    step = S - overlap
    n = 1 + (L - S + step - 1) // step
    return [(i * (L - S)) // (n - 1) for i in range(n)]


def axis_weights(S, ramp):
    """int64 [S]: min(d + 1, S - d, ramp)."""
    d = np.arange(S, dtype=np.int64)
    return np.minimum(np.minimum(d + 1, S - d), ramp)


def weights(tile, ramp):
    """int64 [th, tw]."""
    return axis_weights(tile[0], ramp)[:, None] * axis_weights(tile[1], ramp)[None, :]


def windows(ys, xs):
    """[(y, x)] of the windows in their numbering, t = iy * nx + ix."""
    return [(y, x) for y in ys for x in xs]


def cut(img, ys, xs, tile):
    """img [..., h, w] (planar) -> [T, ..., th, tw]: the crops, copied."""
    th, tw = tile
    return np.stack([img[..., y:y + th, x:x + tw] for y, x in windows(ys, xs)])


def merge(win, img_hw, ys, xs, ramp):
    """win uint8 [N, T, 3, th, tw] -> (uint8 [N, 3, h, w], int64 [N] maxima of the merged bytes)."""
    win = np.asarray(win)
    N, T, C, th, tw = win.shape
    h, w = img_hw
    where = windows(ys, xs)
    assert T == len(where)
    wt = weights((th, tw), ramp)
    A = np.zeros((N, C, h, w), np.int64)
    W = np.zeros((h, w), np.int64)
    for t, (y, x) in enumerate(where):
        A[:, :, y:y + th, x:x + tw] += wt * win[:, t].astype(np.int64)
        W[y:y + th, x:x + tw] += wt
    assert (W > 0).all(), "a pixel no window covers"
    out = (2 * A + W) // (2 * W)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8), out.reshape(N, -1).max(1)
