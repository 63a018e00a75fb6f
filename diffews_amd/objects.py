"""Objects of a label map, on the device: connected components with per-object class, area and box, an optional
minimum-area filter, and the filtered labels re-counted against a ground truth (ops.seg_components).

Every segmentation route ends in a label map -- `labels` of segment_classes / segment_candidates / segment_tiled, `pred`
of the binary routes, `r["native"]["labels"]` / `["pred"]` at the queries' own sizes -- and label_objects turns it into
"which objects, how many, how big, where" without bringing the map to the host.  Nothing here synchronises except
objects_to_host, which copies the two small tables (n and stats) once, runs_to_host and matches_to_host.

object_runs adds each object's SHAPE: the run-length encoding of the id map (ops.seg_rle), in row or column (COCO) order,
still on the device; runs_to_host / runs_to_coco / runs_to_mask bring it to the host and into the usual forms.

match_objects says whether the objects are RIGHT: the objects of a prediction against those of a ground truth (ops.seg_match)
-- the shared pixels of every pair, the areas, a one-to-one matching on IoU and (TP, FP, FN, sum of IoU) per class, which
metrics.panoptic_quality turns into PQ, SQ and RQ; matches_to_host brings the tables to the host.
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


# ------------------------------------------------------------------------------------------------ object matching

class MatchBuffers:
    """Everything one match_objects call of a shape writes, allocated once: pairs int32 [B, max_pairs, 3], pair_off int32
    [B, cap_p + 2], area int32 [B, cap_p + cap_g + 2], match int32 [B, cap_p, 3], gmatch int32 [B, cap_g], pq int64
    [B, nlabels + 1, 4], n int32 [B, 4] and the workspace.  max_records defaults to min(H * W, 1 << 20) records per image
    and max_pairs to min(max_records, 1 << 18) rows -- choices and not measurements: a scene of a few thousand compact
    objects at 4096 x 4096 stays far below both, maps of single pixels overflow them, and match_objects reports that as
    n[.., 0] < n[.., 1] or n[.., 2] < n[.., 3]."""

    def __init__(self, B, H, W, cap_p, cap_g, nlabels, max_records=None, max_pairs=None, device="cuda"):
        self.shape, self.cap_p, self.cap_g, self.nlabels = (int(B), int(H), int(W)), int(cap_p), int(cap_g), int(nlabels)
        self.max_records = min(int(H) * int(W), 1 << 20) if max_records is None else int(max_records)
        self.max_pairs = min(self.max_records, 1 << 18) if max_pairs is None else int(max_pairs)
        if min(self.cap_p, self.cap_g, self.nlabels, self.max_records, self.max_pairs) < 1:
            raise ValueError("cap_p, cap_g, nlabels, max_records and max_pairs must be at least 1")
        nbytes = ops.seg_match_workspace(B, H, W, self.cap_p, self.cap_g, self.max_records, self.max_pairs)
        if nbytes == 0:
            raise ValueError(f"seg_match refuses these sizes: {self.shape}, caps {self.cap_p} x {self.cap_g}, "
                             f"{self.max_records} records, {self.max_pairs} pairs")
        dev, i32 = torch.device(device), torch.int32
        self.pairs = torch.empty(B, self.max_pairs, 3, dtype=i32, device=dev)
        self.device = self.pairs.device
        self.pair_off = torch.empty(B, self.cap_p + 2, dtype=i32, device=dev)
        self.area = torch.empty(B, self.cap_p + self.cap_g + 2, dtype=i32, device=dev)
        self.match = torch.empty(B, self.cap_p, 3, dtype=i32, device=dev)
        self.gmatch = torch.empty(B, self.cap_g, dtype=i32, device=dev)
        self.pq = torch.empty(B, self.nlabels + 1, 4, dtype=torch.int64, device=dev)
        self.n = torch.empty(B, 4, dtype=i32, device=dev)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)


_MATCH_KEYS = ("pairs", "pair_off", "area", "match", "gmatch", "pq", "n")


def _side(o, what):
    """A label_objects result or an (ids, stats-or-None[, cap]) tuple -> (ids, stats, cap); lists stay lists."""
    if isinstance(o, dict):
        ids, stats = o["ids"], o["stats"]
        if stats is None:
            raise ValueError(f"match_objects: the {what} result holds no stats table; pass (ids, None, cap)")
        cap = [s.shape[-2] for s in stats] if isinstance(stats, (list, tuple)) else stats.shape[-2]
        return ids, stats, cap
    if not isinstance(o, (list, tuple)) or len(o) not in (2, 3):
        raise ValueError(f"match_objects: {what} must be a label_objects result or a tuple (ids, stats or None[, cap])")
    ids, stats = o[0], o[1]
    many = isinstance(ids, (list, tuple))
    if len(o) == 3:
        cap = [int(o[2])] * len(ids) if many else int(o[2])
    elif stats is None:
        raise ValueError(f"match_objects: {what} ids without a stats table need an explicit cap: (ids, None, cap)")
    else:
        cap = [s.shape[-2] for s in stats] if many else stats.shape[-2]
    if many and stats is None:
        stats = [None] * len(ids)
    return ids, stats, cap


def _match_one(pids, pstats, cap_p, gids, gstats, cap_g, skip, iou, nlabels, buffers):
    squeeze = pids.dim() == 2
    if squeeze:
        lift = lambda t: None if t is None else t[None]  # noqa: E731
        pids, gids, pstats, gstats, skip = pids[None], lift(gids), lift(pstats), lift(gstats), lift(skip)
    if pids.dim() != 3 or pids.dtype != torch.int32 or not pids.is_cuda:
        raise ValueError("match_objects takes int32 device id maps [H, W] or [B, H, W], or lists of [h, w] maps")
    if gids is None or gids.dtype != torch.int32 or gids.shape != pids.shape:
        raise ValueError("match_objects: the ground truth's ids must be int32 and shaped like the prediction's")
    if skip is not None and (skip.dtype != torch.uint8 or skip.shape != pids.shape):
        raise ValueError("match_objects: skip must be uint8 and shaped like the ids")
    B, H, W = pids.shape
    if buffers is None:
        if nlabels is None:
            raise ValueError("match_objects needs nlabels, the number of classes (or buffers made for it)")
        buffers = MatchBuffers(B, H, W, cap_p, cap_g, nlabels, device=pids.device)
    elif (buffers.shape != (B, H, W) or buffers.device != pids.device or (buffers.cap_p, buffers.cap_g) != (cap_p, cap_g)
          or (nlabels is not None and buffers.nlabels != int(nlabels))):
        raise ValueError(f"buffers were made for {buffers.shape}, caps {buffers.cap_p} x {buffers.cap_g}, {buffers.nlabels} "
                         f"classes on {buffers.device}; the ids are {(B, H, W)} with caps {cap_p} x {cap_g}"
                         f"{'' if nlabels is None else f', {nlabels} classes'} on {pids.device}")
    cont = lambda t: None if t is None else t.contiguous()  # noqa: E731
    ops.seg_match(pids.contiguous(), gids.contiguous(), buffers.pairs, buffers.pair_off, buffers.area, buffers.match,
                  buffers.gmatch, buffers.pq, buffers.n, buffers.ws, buffers.max_records, pstats=cont(pstats),
                  gstats=cont(gstats), skip=cont(skip), iou=iou)
    r = {k: getattr(buffers, k) for k in _MATCH_KEYS}
    if squeeze:
        r = {k: v[0] for k, v in r.items()}
    return r


def match_objects(o_pred, o_gt, skip=None, iou=(1, 2), nlabels=None, buffers=None):
    """The objects of a prediction matched one-to-one to those of a ground truth, and the panoptic-quality counts per
    class.  o_pred, o_gt: two label_objects results -- the ids are o["ids"], the classes column 0 of o["stats"], the caps
    its rows -- or tuples (ids, stats) / (ids, None, cap): int32 device ids [H, W] / [B, H, W] (or lists of [h_i, w_i]
    maps); without a stats table every object of that side has class 1.  Ids outside 1..cap count as background.  skip
    (optional): uint8, shaped like the ids; a pixel whose byte is 255 is not counted -- pass the ground-truth label map and
    its ignore value does the rest.  iou = (num, den): objects of one class in 1..nlabels match when inter * den > num *
    union in integers, strictly; num / den must be at least 1/2, so every object has at most one partner.

    Returns dict(pairs, pair_off, area, match, gmatch, pq, n), all on the device:
      n         int32 [.., 4] = (pairs kept, pairs found, records kept, records found); a record is a maximal interval of
                positions y * W + x with one (p, g) other than (0, 0).  kept < found: the buffers were too small, and every
                table below describes only the first records / the first pairs
      pairs     int32 [.., max_pairs, 3] = (p, g, inter) of every pair that shares a counted pixel, p = 0 or g = 0 for
                background, ascending in (p, g); rows from kept on hold whatever the buffer held
      pair_off  int32 [.., cap_p + 2]: the rows of p are pair_off[p] .. pair_off[p + 1]; the last entry is kept
      area      int32 [.., cap_p + cap_g + 2]: the counted pixels of p = 0..cap_p, then of g = 0..cap_g
      match     int32 [.., cap_p, 3] = (g, inter, union) of object p's partner in row p - 1, zeros without one
      gmatch    int32 [.., cap_g]: the partner p of object g, or 0
      pq        int64 [.., nlabels + 1, 4] = (TP, FP, FN, S) per class, S = the sum of floor(inter * 2^32 / union) over the
                TPs; an object without a counted pixel is neither FP nor FN; metrics.panoptic_quality reads this table
    A [H, W] input gives the same without the batch axis.  A list is handled with ONE CALL PER ITEM and every value of the
    result is then a list, as in label_objects; `skip` is a list too and `buffers` a list of MatchBuffers or None.
    buffers: a MatchBuffers of this shape, caps and class count, reused call after call (the result aliases it); without
    it fresh buffers of MatchBuffers' default sizes are allocated, which needs nlabels.  A fixed number of launches per
    call and no host synchronisation."""
    pids, pstats, cap_p = _side(o_pred, "prediction")
    gids, gstats, cap_g = _side(o_gt, "ground truth")
    if isinstance(pids, (list, tuple)):
        k = len(pids)
        if not isinstance(gids, (list, tuple)) or len(gids) != k:
            raise ValueError("match_objects: one ground-truth id map per predicted id map")
        skips = skip if skip is not None else [None] * k
        bufs = buffers if buffers is not None else [None] * k
        if len(skips) != k or len(bufs) != k:
            raise ValueError("match_objects: one skip / buffers entry per id map")
        per = [_match_one(pids[i], pstats[i], cap_p[i], gids[i], gstats[i], cap_g[i], skips[i], iou, nlabels, bufs[i])
               for i in range(k)]
        return {key: [p[key] for p in per] for key in _MATCH_KEYS}
    if isinstance(gids, (list, tuple)):
        raise ValueError("match_objects: one ground-truth id map per predicted id map")
    return _match_one(pids, pstats, cap_p, gids, gstats, cap_g, skip, iou, nlabels, buffers)


def matches_to_host(m):
    """match_objects' result -> (dict of numpy arrays, truncated) with TWO synchronising copies (per item for a list
    result): the tables n, pair_off, area, match, gmatch and pq first, then pairs[:kept] of every image and nothing behind
    it.  The dict holds the tables under their names and pairs as, per image, an int32 array [kept, 3]; truncated: pairs or
    records kept < found somewhere -- the tables then describe only what was kept.  A [H, W] result gives one image's
    arrays."""
    if isinstance(m["n"], (list, tuple)):
        per = [matches_to_host({k: v[i] for k, v in m.items()}) for i in range(len(m["n"]))]
        return {k: [p[0][k] for p in per] for k in _MATCH_KEYS}, any(p[1] for p in per)
    single = m["n"].dim() == 1
    t = {k: (v[None] if single else v) for k, v in m.items()}
    B = t["n"].shape[0]
    names = ("n", "pair_off", "area", "match", "gmatch")
    both = torch.cat([t[k].reshape(-1) for k in names] + [t["pq"].reshape(-1).view(torch.int32)]).cpu().numpy()   # copy one
    out, at = {}, 0
    for k in names:
        out[k] = both[at:at + t[k].numel()].reshape(t[k].shape)
        at += t[k].numel()
    out["pq"] = both[at:].view(np.int64).reshape(t["pq"].shape)
    kept = out["n"][:, 0].tolist()
    flat = torch.cat([t["pairs"][b, :kept[b]].reshape(-1) for b in range(B)]).cpu().numpy().reshape(-1, 3)   # copy two
    offs = np.concatenate([[0], np.cumsum(kept)])
    out["pairs"] = [flat[offs[b]:offs[b + 1]] for b in range(B)]
    truncated = bool((out["n"][:, 0] < out["n"][:, 1]).any() or (out["n"][:, 2] < out["n"][:, 3]).any())
    if single:
        out = {k: v[0] for k, v in out.items()}
    return out, truncated
