"""Objects of a label map, on the device: connected components with per-object class, area and box, an optional
minimum-area filter, and the filtered labels re-counted against a ground truth (ops.seg_components).

Every segmentation route ends in a label map -- `labels` of segment_classes / segment_candidates / segment_tiled, `pred`
of the binary routes, `r["native"]["labels"]` / `["pred"]` at the queries' own sizes -- and label_objects turns it into
"which objects, how many, how big, where" without bringing the map to the host.  Nothing here synchronises except
objects_to_host, which copies the two small tables (n and stats) once.
"""
import torch

from . import ops


class ComponentBuffers:
    """Everything one label_objects call of a shape writes, allocated once: ids int32 [B, H, W], labels uint8 [B, H, W]
    (the filtered map), n int32 [B, 2], stats int32 [B, max_components, 8], the workspace, and -- made on first use for a
    number of classes -- counts int64 [B, 2, nlabels + 1].  A later call with the same buffers overwrites them."""

    def __init__(self, B, H, W, max_components=1024, device="cuda"):
        self.shape, self.max_components, self.device = (int(B), int(H), int(W)), int(max_components), torch.device(device)
        if self.max_components < 1:
            raise ValueError("max_components must be at least 1")
        dev = self.device
        self.ids = torch.empty(self.shape, dtype=torch.int32, device=dev)
        self.device = self.ids.device                                  # "cuda" resolved to the current device
        self.labels = torch.empty(self.shape, dtype=torch.uint8, device=dev)
        self.n = torch.empty(B, 2, dtype=torch.int32, device=dev)
        self.stats = torch.empty(B, self.max_components, 8, dtype=torch.int32, device=dev)
        self.ws = torch.empty(ops.seg_components_workspace(B, H, W), dtype=torch.uint8, device=dev)
        self._counts = {}

    def counts(self, nlabels):
        c = self._counts.get(nlabels)
        if c is None:
            c = self._counts[nlabels] = torch.empty(self.shape[0], 2, nlabels + 1, dtype=torch.int64, device=self.device)
        return c


def _one(labels, gt, connectivity, min_area, max_components, nlabels, buffers):
    squeeze = labels.dim() == 2
    if squeeze:
        labels, gt = labels[None], None if gt is None else gt[None]
    if labels.dim() != 3 or labels.dtype != torch.uint8 or not labels.is_cuda:
        raise ValueError("label_objects takes a uint8 device tensor [H, W] or [B, H, W], or a list of [h, w] maps")
    labels = labels.contiguous()
    B, H, W = labels.shape
    if buffers is None:
        buffers = ComponentBuffers(B, H, W, max_components, labels.device)
    elif buffers.shape != (B, H, W) or buffers.device != labels.device:
        raise ValueError(f"buffers were made for {buffers.shape} on {buffers.device}, the labels are {(B, H, W)} on {labels.device}")
    counts = None
    if gt is not None:
        if nlabels is None:
            raise ValueError("label_objects: a ground truth needs nlabels, the number of classes")
        if gt.dtype != torch.uint8 or gt.shape != labels.shape:
            raise ValueError("label_objects: gt must be uint8 and shaped like the labels")
        gt, counts = gt.contiguous(), buffers.counts(int(nlabels))
    ops.seg_components(labels, buffers.ids, buffers.n, buffers.ws, filtered=buffers.labels, stats=buffers.stats, gt=gt,
                       counts=counts, connectivity=connectivity, min_area=min_area, nlabels=nlabels)
    r = dict(ids=buffers.ids, labels=buffers.labels, n=buffers.n, stats=buffers.stats, counts=counts)
    if squeeze:
        r = {k: (None if v is None else v[0]) for k, v in r.items()}
    return r


def label_objects(labels, gt=None, connectivity=8, min_area=0, max_components=1024, nlabels=None, buffers=None):
    """Connected components of a label map.  labels: a uint8 device tensor [H, W] or [B, H, W] (0 = background; pixels of
    the same non-zero byte joined over `connectivity` = 4 | 8 neighbours are one object; different bytes never merge), or a
    LIST of [h_i, w_i] maps of different sizes, as the native-size routes return them.  An object with fewer than min_area
    pixels is removed.  gt (optional, with nlabels = the number of classes): uint8, shaped like the labels, 0..nlabels, 255
    and anything above nlabels ignored.

    Returns dict(ids, labels, n, stats, counts), all on the device:
      ids     int32, 0 = background or removed, else 1..n in row-major order of each object's first pixel, per image
      labels  uint8, the input without the removed objects -- what metrics.nway_iou's counts below describe
      n       int32 [.., 2] = (objects kept, objects found before the filter)
      stats   int32 [.., max_components, 8] = (label, area, y0, x0, y1, x1 half-open, first pixel y * W + x, 0) of object
              id in row id - 1, zero rows behind; when n[.., 0] > max_components only this table is cut short
      counts  int64 [.., 2, nlabels + 1] (intersections, unions) of the FILTERED labels against gt, or None
    A [H, W] input gives the same without the batch axis.  A list is handled with ONE CALL PER ITEM -- ragged sizes do not
    share a launch -- and every value of the result is then a list; `gt` is a list too and `buffers` a list of
    ComponentBuffers or None.  buffers: a ComponentBuffers of this shape, reused call after call (the result then aliases
    it); without it fresh buffers are allocated.  A fixed number of launches per call and no host synchronisation."""
    if isinstance(labels, (list, tuple)):
        gts = gt if gt is not None else [None] * len(labels)
        bufs = buffers if buffers is not None else [None] * len(labels)
        if len(gts) != len(labels) or len(bufs) != len(labels):
            raise ValueError("label_objects: one gt / buffers entry per label map")
        per = [_one(l, g, connectivity, min_area, max_components, nlabels, b) for l, g, b in zip(labels, gts, bufs)]
        return {k: [p[k] for p in per] for k in ("ids", "labels", "n", "stats", "counts")}
    return _one(labels, gt, connectivity, min_area, max_components, nlabels, buffers)


def objects_to_host(r):
    """label_objects' result -> (objects, truncated) on the host, with ONE synchronising copy of n and stats (per item
    for a list result).  objects: per image a list of (label, area, (y0, x0, y1, x1), first_pixel), in id order;
    truncated: True when an image holds more objects than the stats table has rows (the list then ends at the table's
    last row; ids, labels and counts on the device are complete all the same).  A [H, W] result gives one image's list."""
    if isinstance(r["n"], (list, tuple)):
        per = [objects_to_host({k: v[i] for k, v in r.items()}) for i in range(len(r["n"]))]
        return [p[0] for p in per], any(p[1] for p in per)
    n, stats = r["n"], r["stats"]
    single = n.dim() == 1
    if single:
        n, stats = n[None], stats[None]
    B, cap = stats.shape[:2]
    both = torch.cat([n.reshape(-1), stats.reshape(-1)]).cpu()       # the one copy
    n, stats = both[:2 * B].view(B, 2).tolist(), both[2 * B:].view(B, cap, 8).tolist()
    objs = [[(s[0], s[1], (s[2], s[3], s[4], s[5]), s[6]) for s in stats[b][:min(n[b][0], cap)]] for b in range(B)]
    truncated = any(n[b][0] > cap for b in range(B))
    return (objs[0] if single else objs), truncated
