"""Objects of a label map, on the device: connected components with per-object class, area and box, an optional
minimum-area filter, and the filtered labels re-counted against a ground truth (ops.seg_components).

Every segmentation route ends in a label map -- `labels` of segment_classes / segment_candidates / segment_tiled, `pred`
of the binary routes, `r["native"]["labels"]` / `["pred"]` at the queries' own sizes -- and label_objects turns it into
"which objects, how many, how big, where" without bringing the map to the host.  Nothing here synchronises except
objects_to_host, which copies the two small tables (n and stats) once, and runs_to_host.

object_runs adds each object's SHAPE: the run-length encoding of the id map (ops.seg_rle), in row or column (COCO) order,
still on the device; runs_to_host / runs_to_coco / runs_to_mask bring it to the host and into the usual forms.
"""
import numpy as np
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


# ------------------------------------------------------------------------------------------------ run-length encodings

class RunBuffers:
    """Everything one object_runs call of a shape writes, allocated once: runs int32 [B, max_runs, 2], run_off int32
    [B, max_components + 1], nruns int32 [B, 2] and the workspace.  max_runs defaults to min(H * W, 1 << 20) rows per
    image -- 8 MB at the most, a choice and not a measurement: a scene of a few thousand compact objects at 4096 x 4096
    stays far below it, a map of single pixels overflows it and object_runs reports that as found > kept."""

    def __init__(self, B, H, W, max_components=1024, max_runs=None, order="column", device="cuda"):
        self.shape, self.max_components, self.order = (int(B), int(H), int(W)), int(max_components), order
        self.max_runs = min(int(H) * int(W), 1 << 20) if max_runs is None else int(max_runs)
        if self.max_components < 1 or self.max_runs < 1:
            raise ValueError("max_components and max_runs must be at least 1")
        nbytes = ops.seg_rle_workspace(B, H, W, self.max_components, self.max_runs, order)   # refuses a bad order
        dev = torch.device(device)
        self.runs = torch.empty(B, self.max_runs, 2, dtype=torch.int32, device=dev)
        self.device = self.runs.device
        self.run_off = torch.empty(B, self.max_components + 1, dtype=torch.int32, device=dev)
        self.nruns = torch.empty(B, 2, dtype=torch.int32, device=dev)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _runs_one(ids, cap, order, max_runs, buffers):
    squeeze = ids.dim() == 2
    if squeeze:
        ids = ids[None]
    if ids.dim() != 3 or ids.dtype != torch.int32 or not ids.is_cuda:
        raise ValueError("object_runs takes an int32 device tensor [H, W] or [B, H, W], or a list of [h, w] maps")
    ids = ids.contiguous()
    B, H, W = ids.shape
    if buffers is None:
        buffers = RunBuffers(B, H, W, cap, max_runs, order, ids.device)
    elif (buffers.shape != (B, H, W) or buffers.device != ids.device or buffers.max_components != cap
          or buffers.order != order or (max_runs is not None and buffers.max_runs != int(max_runs))):
        raise ValueError(f"buffers were made for {buffers.shape}, {buffers.max_components} objects, {buffers.max_runs} runs, "
                         f"order {buffers.order!r} on {buffers.device}; the ids are {(B, H, W)} with {cap} objects, order "
                         f"{order!r} on {ids.device}")
    ops.seg_rle(ids, buffers.runs, buffers.run_off, buffers.nruns, buffers.ws, cap, order)
    r = dict(runs=buffers.runs, run_off=buffers.run_off, nruns=buffers.nruns, order=order, shape=(H, W))
    if squeeze:
        r.update(runs=r["runs"][0], run_off=r["run_off"][0], nruns=r["nruns"][0])
    return r


def object_runs(o, order="column", max_runs=None, buffers=None, max_components=None):
    """The run-length encoding of every object of an id map.  o: a label_objects result -- the ids are o["ids"] and the
    objects encoded are 1..cap, cap = the rows of o["stats"] -- or an int32 device tensor [H, W] / [B, H, W] of ids (or a
    list of [h_i, w_i] maps) together with max_components=.  order: "column" (position x * H + y, COCO's) or "row"
    (y * W + x); a run is a maximal interval of positions of one object and does not stop at a line's end.

    Returns dict(runs, run_off, nruns, order, shape), the tensors on the device:
      nruns    int32 [.., 2] = (runs kept, runs found); kept = min(found, max_runs), the first runs in ascending start
      runs     int32 [.., max_runs, 2] = (start, length), grouped by object ascending and ascending in start within an
               object; rows from kept on hold whatever the buffer held
      run_off  int32 [.., cap + 1]: object k's runs are rows run_off[k-1] .. run_off[k]
      shape    (H, W) of the map
    A list is handled with ONE CALL PER ITEM and every value of the result is then a list, as in label_objects; `buffers` is
    then a list of RunBuffers or None.  buffers: a RunBuffers of this shape, object count and order, reused call after call
    (the result aliases it); max_runs: rows per image for fresh buffers (RunBuffers' default otherwise).  A fixed number of
    launches per call and no host synchronisation."""
    if isinstance(o, dict):
        if max_components is not None:
            raise ValueError("object_runs: max_components comes from the result's stats table")
        ids, stats = o["ids"], o["stats"]
        caps = [s.shape[-2] for s in stats] if isinstance(stats, (list, tuple)) else stats.shape[-2]
    else:
        if max_components is None:
            raise ValueError("object_runs: an id tensor needs max_components, the highest id to encode")
        ids = o
        caps = [int(max_components)] * len(ids) if isinstance(ids, (list, tuple)) else int(max_components)
    if isinstance(ids, (list, tuple)):
        bufs = buffers if buffers is not None else [None] * len(ids)
        if len(bufs) != len(ids):
            raise ValueError("object_runs: one buffers entry per id map")
        per = [_runs_one(i, c, order, max_runs, b) for i, c, b in zip(ids, caps, bufs)]
        return {k: [p[k] for p in per] for k in ("runs", "run_off", "nruns", "order", "shape")}
    return _runs_one(ids, caps, order, max_runs, buffers)


def runs_to_host(rr):
    """object_runs' result -> (per image a list over the objects 1..min(n, cap) of int32 numpy arrays [k, 2] = (start,
    length) in ascending start, truncated) with TWO synchronising copies (per item for a list result): the small tables
    nruns and run_off first, then runs[:kept] of every image and nothing behind it.  n = the highest object with a run.
    truncated: found > kept somewhere -- the buffers had fewer rows than the image has runs, and the lists hold only the
    runs that start first.  A [H, W] result gives one image's list."""
    if isinstance(rr["nruns"], (list, tuple)):
        per = [runs_to_host({k: v[i] for k, v in rr.items()}) for i in range(len(rr["nruns"]))]
        return [p[0] for p in per], any(p[1] for p in per)
    nruns, run_off, runs = rr["nruns"], rr["run_off"], rr["runs"]
    single = nruns.dim() == 1
    if single:
        nruns, run_off, runs = nruns[None], run_off[None], runs[None]
    B, cap = run_off.shape[0], run_off.shape[1] - 1
    both = torch.cat([nruns.reshape(-1), run_off.reshape(-1)]).cpu().numpy()       # copy one: the tables
    nruns, run_off = both[:2 * B].reshape(B, 2), both[2 * B:].reshape(B, cap + 1)
    kept = nruns[:, 0].tolist()
    flat = torch.cat([runs[b, :kept[b]].reshape(-1) for b in range(B)]).cpu().numpy().reshape(-1, 2)   # copy two
    out, at = [], 0
    for b in range(B):
        rows, off = flat[at:at + kept[b]], run_off[b]
        at += kept[b]
        n = int(np.searchsorted(off, kept[b], side="left")) if kept[b] else 0   # the first k with run_off[k] == kept
        out.append([rows[off[k - 1]:off[k]] for k in range(1, min(n, cap) + 1)])
    truncated = bool((nruns[:, 1] > nruns[:, 0]).any())
    return (out[0] if single else out), truncated


def runs_to_coco(runs_k, h, w, order="column"):
    """One object's runs [k, 2] (column order, ascending start) -> {"size": [h, w], "counts": [...]}, the uncompressed COCO
    RLE: alternating lengths of zeros and ones over the column-major positions, zeros first.  Runs in row order are
    refused: COCO has no such form."""
    if order != "column":
        raise ValueError("a COCO RLE runs down the columns: encode with order='column'")
    counts, at = [], 0
    for s, l in np.asarray(runs_k, dtype=np.int64).reshape(-1, 2).tolist():
        counts += [s - at, l]
        at = s + l
    if at < h * w:
        counts.append(h * w - at)
    return {"size": [int(h), int(w)], "counts": counts}


def runs_to_mask(runs_k, h, w, order):
    """One object's runs [k, 2] -> numpy bool [h, w]."""
    if order not in ("row", "column"):
        raise ValueError(f"order must be 'row' or 'column', not {order!r}")
    r = np.asarray(runs_k, dtype=np.int64).reshape(-1, 2)
    edge = np.zeros(h * w + 1, np.int64)
    np.add.at(edge, r[:, 0], 1)
    np.add.at(edge, r[:, 0] + r[:, 1], -1)
    flat = np.cumsum(edge[:-1]) > 0
    return flat.reshape(h, w) if order == "row" else flat.reshape(w, h).T.copy()
