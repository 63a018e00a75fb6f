"""Host-side wrappers of the two calls that split touching objects: the nearest seed inside the object (dfw_seg_components
with `seeds`, a stage of its own on that entry point) and connected components of equal (byte, key) pairs
(dfw_seg_components with `keys`).

They are the wrappers of ops.py in every respect -- caller-owned buffers only, every tensor through ops._Args, no `assert`,
no allocation, the device rule last and the stream asked for behind it -- and live in a module of their own because the
refusal table of ops.py / ops_bwd.py (tests/op_args_cases.py) names every tensor parameter of those two files; this module
has a table of its own (tests/split_args_cases.py) under the same discipline.
"""
import ctypes as C

import torch

from . import _lib as L
from .ops import _Args, _stream


def seg_nearest_workspace(B, H, W):
    """Bytes of seg_nearest's workspace for [B, H, W] maps, 5 a pixel; 0 for sizes the call refuses."""
    return int(L.lib().dfw_seg_nearest_workspace_bytes(int(B), int(H), int(W)))


def seg_nearest(map, seeds, nearest, dist, ws, reach, passes=1):
    """The nearest seed inside the object, on caller-owned buffers only (objects.SplitBuffers holds a set).  map int32
    [B, H, W], values compared for equality only, 0 = background; seeds int32 [B, H, W], every non-zero value a seed.  A
    candidate of a pixel p = (y, x) with v = map[p] != 0 is a seed q = (y + dy, x + dx) with dy^2 + dx^2 <= reach^2 that an
    L path on v joins to p: down or up column x from row y to row y + dy, then along that row to x + dx.  Writes nearest
    int32 [B, H, W], the value of the candidate with the smallest (dy^2 + dx^2, value) and 0 where there is none (and on
    background), and dist uint16 [B, H, W]: 0 on a seed and on background, the winner's dy^2 + dx^2, (reach + 1)^2 without
    a candidate.  passes (1..8) repeats the pass with seeds := nearest in place; a pixel that holds a value keeps it and
    its dist, so each pass carries every label round one more bend.  1 <= reach <= 254.  ws: a uint8 buffer of at least
    seg_nearest_workspace(B, H, W) bytes, which needs no initialisation.  2 * passes launches, no host synchronisation, no
    memset node, no atomics: the call can be captured.  Returns None."""
    own = _Args("seg_nearest")
    own("map", map, torch.int32, dim=3)
    B, H, W = map.shape
    a = L.SegComponentsArgs()
    a.map, a.seeds = map.data_ptr(), own("seeds", seeds, torch.int32, (B, H, W))
    a.nearest, a.dist = own("nearest", nearest, torch.int32, (B, H, W)), own("dist", dist, torch.uint16, (B, H, W))
    a.ws, a.ws_bytes = own("ws", ws, torch.uint8), ws.numel()
    a.B, a.H, a.W, a.reach, a.passes = B, H, W, int(reach), int(passes)
    own.device()
    L.check(L.lib().dfw_seg_components(C.byref(a), _stream()), "dfw_seg_components")


def seg_components_keyed(labels, keys, ids, n, ws, filtered=None, stats=None, gt=None, counts=None, connectivity=8, min_area=0,
                         nlabels=None):
    """ops.seg_components with a second plane: keys int32 [B, H, W], compared for equality only (0 and negative values are
    keys like any other).  Two neighbouring pixels join when their label bytes are equal and non-zero AND their keys are
    equal; everything else -- ids numbered by first pixel, n, filtered, stats (the label column is the byte), counts, ws
    (ops.seg_components_workspace), the number of launches -- is that call's.  Returns None."""
    own = _Args("seg_components_keyed")
    own("labels", labels, torch.uint8, dim=3)
    B, H, W = labels.shape
    a = L.SegComponentsArgs()
    a.labels, a.keys = labels.data_ptr(), own("keys", keys, torch.int32, (B, H, W))
    a.ids, a.n = own("ids", ids, torch.int32, (B, H, W)), own("n", n, torch.int32, (B, 2))
    a.ws, a.ws_bytes = own("ws", ws, torch.uint8), ws.numel()
    if filtered is not None:
        a.filtered = own("filtered", filtered, torch.uint8, (B, H, W))
    if stats is not None:
        own.need(stats.dim() == 3, "stats must be int32 [B, cap, 8]")
        a.stats, a.cap = own("stats", stats, torch.int32, (B, stats.shape[1], 8)), stats.shape[1]
    own.need(counts is None or gt is not None, "counts need a ground truth")
    if gt is not None:
        own.need(nlabels is not None, "a ground truth needs nlabels, the number of classes")
        a.gt, a.nlabels = own("gt", gt, torch.uint8, (B, H, W)), int(nlabels)
        if counts is not None:
            a.counts = own("counts", counts, torch.int64, (B, 2, int(nlabels) + 1))
    a.B, a.H, a.W, a.connectivity, a.min_area = B, H, W, int(connectivity), int(min_area)
    own.device()
    L.check(L.lib().dfw_seg_components(C.byref(a), _stream()), "dfw_seg_components")
