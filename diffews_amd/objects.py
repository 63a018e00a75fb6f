"""Objects of a label map, on the device: connected components with per-object class, area and box, an optional
minimum-area filter, and the filtered labels re-counted against a ground truth (ops.seg_components).

Every segmentation route ends in a label map -- `labels` of segment_classes / segment_candidates / segment_tiled, `pred`
of the binary routes, `r["native"]["labels"]` / `["pred"]` at the queries' own sizes -- and label_objects turns it into
"which objects, how many, how big, where" without bringing the map to the host.  Nothing here synchronises except
objects_to_host, which copies the two small tables (n and stats) once, runs_to_host, contours_to_host, matches_to_host,
scores_to_host, detections_to_host and thickness_to_host.

fill_holes is the partner of min_area: the background regions that ONE object encloses, up to max_area pixels, take that
object's id and label (ops.seg_holes), and the result is again a label_objects result, so every stage below takes it.  A
region between two objects, or one with an island of another object inside, is left alone.

object_runs adds each object's SHAPE: the run-length encoding of the id map (ops.seg_rle), in row or column (COCO) order,
still on the device; runs_to_host / runs_to_coco / runs_to_mask bring it to the host and into the usual forms.

object_contours gives each object's OUTLINE: rings of corner points on the pixel lattice (ops.seg_contours), the outer ring
and the hole rings of every object, still on the device; contours_to_host brings them to the host, rings_to_geojson /
rings_to_coco / rings_to_mask put them into the usual forms.

match_objects says whether the objects are RIGHT: the objects of a prediction against those of a ground truth (ops.seg_match)
-- the shared pixels of every pair, the areas, a one-to-one matching on IoU and (TP, FP, FN, sum of IoU) per class, which
metrics.panoptic_quality turns into PQ, SQ and RQ; matches_to_host brings the tables to the host.

object_scores says how SURE the model is of each object: the decoder's uint8 mask planes reduced over the id map
(ops.seg_scores) into (sum, counted pixels, min, max) per object, exact integers; planes_for_classes / planes_for_binary /
planes_for_candidates build the table that says which planes a label of an image reads.  scores_to_host brings the table
to the host, coco_results turns the three host tables into COCO result records, and detections_to_host gathers what
metrics.average_precision ranks.

boundary_bands says how good the CONTOURS are: the capped chessboard distance of every pixel of a label map or an id map
to its own contour (ops.seg_boundary) and the band of pixels within d of it, d = 2 % of the image diagonal by default --
the band of Boundary IoU (Cheng et al., CVPR 2021).  object_boundaries runs it on the labels and the ids of a label_objects
result; boundary_counts counts two label bands against each other per class, in the counts layout metrics.nway_iou /
metrics.boundary_iou read.  Per-object Boundary IoU needs no stage of its own: the band of an id map is an id map, so
    pb, gb = object_boundaries(o_pred), object_boundaries(o_gt)
    m = match_objects((pb["ids"]["band"], o_pred["stats"]), (gb["ids"]["band"], o_gt["stats"]), skip=gt_labels, nlabels=N)
gives in m["pairs"] the shared band pixels of every (pred, gt) pair, in m["area"] the band areas, and in m["match"] / m["pq"]
the matching and the panoptic counts at Boundary IoU above `iou`.

object_thickness says how THICK an object is and where its MIDDLE lies: the squared Euclidean distance of every pixel of
the id map to its own contour (ops.seg_boundary with metric="euclidean", which boundary_bands and object_boundaries take as
well) and, per object, the largest of them with its first position -- radius and centre of the largest inscribed circle, a
label point inside the object and the measure a min-thickness rule needs; thickness_to_host brings the table to the host.
object_cores labels the pixels farther than a radius from the contour again: touching objects of one class fall apart.

split_objects grows those cores back into full INSTANCES: every object pixel takes the core that an L path inside its
object reaches first (nearest_seeds, ops_split.seg_nearest), and the object's labels are labelled again with that core as
a second key (label_objects(..., keys=), ops_split.seg_components_keyed).  The result is a label_objects result -- every
stage above takes it as it stands -- that also says which object each instance came from.
"""
import numpy as np
import torch

from . import ops, ops_split


# ------------------------------------------------------------------------------------------------ what the stages share

def _per_item(call, k, optional, message, keys):
    """The list dispatch of every stage: each of `optional` is a list of k per-item arguments or None (k times None then;
    any other length is ValueError(message)); call(i, *entries of item i) runs once per item, and the per-item dicts
    become one dict of lists over `keys`."""
    cols = [c if c is not None else [None] * k for c in optional]
    if any(len(c) != k for c in cols):
        raise ValueError(message)
    per = [call(i, *(c[i] for c in cols)) for i in range(k)]
    return {key: [p[key] for p in per] for key in keys}


def _lift(squeeze, *ts):
    """[H, W] inputs as batches of one when squeeze is set; None stays None."""
    return tuple(t[None] if squeeze and t is not None else t for t in ts)


def _unlift(squeeze, r):
    """... and the result without that batch axis again: every tensor of r loses it, everything else stays."""
    return {k: (v[0] if squeeze and isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _rows(stats):
    """cap, the rows of a stats table -- per item for a list."""
    return [s.shape[-2] for s in stats] if isinstance(stats, (list, tuple)) else stats.shape[-2]


def _ids_caps(o, max_components, who, verb):
    """A label_objects result, or an id tensor (or list of them) with max_components -> (ids, cap); cap per item for a
    list."""
    if isinstance(o, dict):
        if max_components is not None:
            raise ValueError(f"{who}: max_components comes from the result's stats table")
        return o["ids"], _rows(o["stats"])
    if max_components is None:
        raise ValueError(f"{who}: an id tensor needs max_components, the highest id to {verb}")
    return o, [int(max_components)] * len(o) if isinstance(o, (list, tuple)) else int(max_components)


def _cached_counts(self, nlabels):
    """The counts method of ComponentBuffers and HoleBuffers: int64 [B, 2, nlabels + 1], made on first use for a number of
    classes and kept."""
    c = self._counts.get(nlabels)
    if c is None:
        c = self._counts[nlabels] = torch.empty(self.shape[0], 2, nlabels + 1, dtype=torch.int64, device=self.device)
    return c


def _to_host(tensors):
    """int32 / int64 device tensors -> numpy arrays of the same shapes and dtypes with ONE synchronising copy: flattened
    and concatenated on the device (an int64 table as pairs of int32), copied, split again."""
    parts = [t.reshape(-1).view(torch.int32) if t.dtype == torch.int64 else t.reshape(-1) for t in tensors]
    flat = torch.cat(parts).cpu().numpy()
    cut = np.cumsum([0] + [p.numel() for p in parts])
    return [(flat[cut[i]:cut[i + 1]].view(np.int64) if t.dtype == torch.int64 else flat[cut[i]:cut[i + 1]]).reshape(t.shape)
            for i, t in enumerate(tensors)]


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

    counts = _cached_counts


def _one(labels, gt, connectivity, min_area, max_components, nlabels, buffers, keys=None):
    squeeze = labels.dim() == 2
    labels, gt, keys = _lift(squeeze, labels, gt, keys)
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
    if keys is not None:
        if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int32 or keys.shape != labels.shape:
            raise ValueError("label_objects: keys must be an int32 tensor shaped like the labels")
        ops_split.seg_components_keyed(labels, keys.contiguous(), buffers.ids, buffers.n, buffers.ws, filtered=buffers.labels,
                                       stats=buffers.stats, gt=gt, counts=counts, connectivity=connectivity, min_area=min_area,
                                       nlabels=nlabels)
    else:
        ops.seg_components(labels, buffers.ids, buffers.n, buffers.ws, filtered=buffers.labels, stats=buffers.stats, gt=gt,
                           counts=counts, connectivity=connectivity, min_area=min_area, nlabels=nlabels)
    return _unlift(squeeze, dict(ids=buffers.ids, labels=buffers.labels, n=buffers.n, stats=buffers.stats, counts=counts))


def label_objects(labels, gt=None, connectivity=8, min_area=0, max_components=1024, nlabels=None, buffers=None, keys=None):
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
    it); without it fresh buffers are allocated.  A fixed number of launches per call and no host synchronisation.

    keys (optional): an int32 tensor shaped like the labels (a list for a list), compared for equality only.  Two
    neighbouring pixels then join only when their keys are equal as well; 0 and negative values are keys like any other,
    and a pixel is an object pixel by its byte alone.  Everything else is unchanged, stats' label column included."""
    if isinstance(labels, (list, tuple)):
        return _per_item(lambda i, g, b, k: _one(labels[i], g, connectivity, min_area, max_components, nlabels, b, k),
                         len(labels), (gt, buffers, keys), "label_objects: one gt / buffers / keys entry per label map",
                         ("ids", "labels", "n", "stats", "counts"))
    return _one(labels, gt, connectivity, min_area, max_components, nlabels, buffers, keys)


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
    n, stats = (a.tolist() for a in _to_host([n, stats]))            # the one copy
    objs = [[(s[0], s[1], (s[2], s[3], s[4], s[5]), s[6]) for s in stats[b][:min(n[b][0], cap)]] for b in range(B)]
    truncated = any(n[b][0] > cap for b in range(B))
    return (objs[0] if single else objs), truncated


# ------------------------------------------------------------------------------------------------ holes

class HoleBuffers:
    """Everything one fill_holes call of a shape writes, allocated once: ids int32 [B, H, W], labels uint8 [B, H, W],
    holes int32 [B, 2], stats int32 [B, max_components, 8], the workspace, and -- made on first use for a number of
    classes -- counts int64 [B, 2, nlabels + 1].  max_components is that of the label_objects result the calls take.  A
    later call with the same buffers overwrites them."""

    def __init__(self, B, H, W, max_components=1024, device="cuda"):
        self.shape, self.max_components = (int(B), int(H), int(W)), int(max_components)
        if self.max_components < 1:
            raise ValueError("max_components must be at least 1")
        nbytes = ops.seg_holes_workspace(*self.shape)
        if nbytes == 0:
            raise ValueError(f"seg_holes refuses these sizes: {self.shape}")
        dev = torch.device(device)
        self.ids = torch.empty(self.shape, dtype=torch.int32, device=dev)
        self.device = self.ids.device                                  # "cuda" resolved to the current device
        self.labels = torch.empty(self.shape, dtype=torch.uint8, device=dev)
        self.holes = torch.empty(self.shape[0], 2, dtype=torch.int32, device=dev)
        self.stats = torch.empty(self.shape[0], self.max_components, 8, dtype=torch.int32, device=dev)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._counts = {}

    counts = _cached_counts


def _holes_one(o, max_area, connectivity, gt, nlabels, buffers):
    if connectivity not in (4, 8):
        raise ValueError(f"fill_holes: connectivity must be 4 or 8, not {connectivity!r}")
    if max_area is not None and not 0 <= int(max_area) <= 2 ** 31 - 1:
        raise ValueError(f"fill_holes: max_area must lie in 0..2^31 - 1 (None: no limit), got {max_area}")
    ids, labels, n, stats = o["ids"], o["labels"], o["n"], o["stats"]
    squeeze = ids.dim() == 2
    ids, labels, stats, gt = _lift(squeeze, ids, labels, stats, gt)
    if ids.dim() != 3 or ids.dtype != torch.int32 or not ids.is_cuda or labels.dtype != torch.uint8 or labels.shape != ids.shape:
        raise ValueError("fill_holes takes a label_objects result: ids int32 and labels uint8 on the device, [H, W] or "
                         "[B, H, W], or lists of [h, w] maps")
    B, H, W = ids.shape
    if stats.dim() != 3 or stats.dtype != torch.int32 or stats.shape[0] != B or stats.shape[2] != 8:
        raise ValueError("fill_holes: stats must be the int32 [.., max_components, 8] table of the label_objects result")
    cap = stats.shape[1]
    if buffers is None:
        buffers = HoleBuffers(B, H, W, cap, ids.device)
    elif buffers.shape != (B, H, W) or buffers.device != ids.device or buffers.max_components != cap:
        raise ValueError(f"buffers were made for {buffers.shape} with {buffers.max_components} components on {buffers.device}, "
                         f"the objects are {(B, H, W)} with {cap} on {ids.device}")
    counts = None
    if gt is not None:
        if nlabels is None:
            raise ValueError("fill_holes: a ground truth needs nlabels, the number of classes")
        if gt.dtype != torch.uint8 or gt.shape != ids.shape:
            raise ValueError("fill_holes: gt must be uint8 and shaped like the labels")
        gt, counts = gt.contiguous(), buffers.counts(int(nlabels))
    ops.seg_holes(labels.contiguous(), ids.contiguous(), buffers.ids, buffers.labels, buffers.holes, buffers.ws,
                  stats=stats.contiguous(), stats_out=buffers.stats, gt=gt, counts=counts, connectivity=connectivity,
                  max_area=max_area, nlabels=nlabels)
    r = _unlift(squeeze, dict(ids=buffers.ids, labels=buffers.labels, stats=buffers.stats, counts=counts, holes=buffers.holes))
    r["n"] = n
    return r


def fill_holes(o, max_area=None, connectivity=8, gt=None, nlabels=None, buffers=None):
    """Fills the pinholes of the objects of a label_objects result o -- the partner of its min_area, which turns a speck
    inside an object into background, a hole that object_runs, match_objects and boundary_bands would all see.

    A region is a connected component of background pixels (labels == 0) under the DUAL of `connectivity`, which is the
    objects' and must be the one o was made with: 4 neighbours for 8-connected objects, 8 for 4-connected ones.  It is
    enclosed when none of its pixels lies on the first or last row or column.  Its owner is the id of the pixel to the left
    of its first pixel (the smallest y * W + x).  It is FILLED when it is enclosed, the owner is at least 1, every
    non-background pixel in the neighbourhood of its pixels carries the owner's id, and it has at most max_area pixels
    (None: no limit; 0 fills nothing).  NOT filled, on purpose: a region bordered by two objects, whether or not they share
    a class, and a hole with an island of another object inside -- label_objects(min_area=k) removes such islands first.
    gt (optional, with nlabels): as label_objects takes it.

    Returns dict(ids, labels, n, stats, counts, holes), all on the device and itself a label_objects result, which
    objects_to_host, object_runs, match_objects, object_scores, object_boundaries and boundary_counts take unchanged:
      ids, labels  o's maps with every pixel of a filled region set to the owner's id and label byte
      n            o's n, passed through: filling neither adds nor removes an object
      stats        o's stats with column 1 (area) grown by, and column 7 set to, the object's filled pixels; label, box and
                   first pixel do not change.  Re-labelling `labels` with label_objects gives exactly these ids and, with
                   column 7 zeroed, these stats
      counts       int64 [.., 2, nlabels + 1] (intersections, unions) of the filled labels against gt, or None
      holes        int32 [.., 2] = (regions filled, regions enclosed)
    A [H, W] result gives the same without the batch axis.  A list (native-size) result is handled with ONE CALL PER ITEM;
    gt is then a list too and buffers a list of HoleBuffers or None.  buffers: a HoleBuffers of this shape and
    max_components, reused call after call (the result then aliases it).  At most 6 launches per call and no host
    synchronisation."""
    if isinstance(o["ids"], (list, tuple)):
        item = lambda i: {key: o[key][i] for key in ("ids", "labels", "n", "stats")}  # noqa: E731
        return _per_item(lambda i, g, b: _holes_one(item(i), max_area, connectivity, g, nlabels, b), len(o["ids"]),
                         (gt, buffers), "fill_holes: one gt / buffers entry per item",
                         ("ids", "labels", "n", "stats", "counts", "holes"))
    return _holes_one(o, max_area, connectivity, gt, nlabels, buffers)


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
    ids, = _lift(squeeze, ids)
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
    return _unlift(squeeze, dict(runs=buffers.runs, run_off=buffers.run_off, nruns=buffers.nruns, order=order, shape=(H, W)))


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
    ids, caps = _ids_caps(o, max_components, "object_runs", "encode")
    if isinstance(ids, (list, tuple)):
        return _per_item(lambda i, b: _runs_one(ids[i], caps[i], order, max_runs, b), len(ids), (buffers,),
                         "object_runs: one buffers entry per id map", ("runs", "run_off", "nruns", "order", "shape"))
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
    nruns, run_off = _to_host([nruns, run_off])                               # copy one: the tables
    kept = nruns[:, 0].tolist()
    runs = _to_host([runs[b, :kept[b]] for b in range(B)])                    # copy two
    out = []
    for b in range(B):
        rows, off = runs[b], run_off[b]
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


# ------------------------------------------------------------------------------------------------ outlines

class ContourBuffers:
    """Everything one object_contours call of a shape writes, allocated once: verts int32 [B, max_edges, 2], rings int32
    [B, max_edges / 4, 4], ring_off int32 [B, max_components + 1], n int32 [B, 4] and the workspace (4 bytes a pixel and 64
    a row of max_edges).  max_edges defaults to max(4096, H * W // 8) rounded down to a multiple of 4 -- a choice and not a
    measurement: compact objects have far fewer unit edges than that, a map of single pixels has 4 * H * W and
    object_contours reports it as not complete, with the number to size for in n[.., 0].  simplify=True: it also holds
    simp_verts, simp_rings and simp_n, shaped like verts, rings and n, for object_contours(.., tolerance=); the workspace
    is the same."""

    def __init__(self, B, H, W, max_components=1024, max_edges=None, device="cuda", simplify=False):
        self.shape, self.max_components = (int(B), int(H), int(W)), int(max_components)
        self.max_edges = max(4096, int(H) * int(W) // 8) // 4 * 4 if max_edges is None else int(max_edges)
        if self.max_components < 1 or self.max_edges < 4 or self.max_edges % 4:
            raise ValueError("max_components must be at least 1 and max_edges a multiple of 4, at least 4")
        nbytes = ops.seg_contours_workspace(B, H, W, self.max_components, self.max_edges)
        if nbytes == 0:
            raise ValueError(f"seg_contours refuses these sizes: {self.shape}, {self.max_components} objects, {self.max_edges} edges")
        dev, i32 = torch.device(device), torch.int32
        self.verts = torch.empty(B, self.max_edges, 2, dtype=i32, device=dev)
        self.device = self.verts.device
        self.rings = torch.empty(B, self.max_edges // 4, 4, dtype=i32, device=dev)
        self.ring_off = torch.empty(B, self.max_components + 1, dtype=i32, device=dev)
        self.n = torch.empty(B, 4, dtype=i32, device=dev)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.simplify = bool(simplify)
        self.simp_verts = torch.empty_like(self.verts) if simplify else None
        self.simp_rings = torch.empty_like(self.rings) if simplify else None
        self.simp_n = torch.empty_like(self.n) if simplify else None


def _tol4(tolerance):
    """The tolerance in pixels -> quarter pixels, or a ValueError that names the rule; None -> None."""
    if tolerance is None:
        return None
    t = float(tolerance) * 4 if isinstance(tolerance, (int, float)) and not isinstance(tolerance, bool) else -1.0
    if not 0 <= t <= 32768 or t != int(t):
        raise ValueError(f"object_contours: tolerance must be a multiple of 0.25 pixels in 0..8192, not {tolerance!r}")
    return int(t)


_CONTOUR_KEYS = ("verts", "rings", "ring_off", "n")


def _contours_one(ids, cap, connectivity, max_edges, buffers, tol4=None, tolerance=None):
    squeeze = ids.dim() == 2
    ids, = _lift(squeeze, ids)
    if ids.dim() != 3 or ids.dtype != torch.int32 or not ids.is_cuda:
        raise ValueError("object_contours takes an int32 device tensor [H, W] or [B, H, W], or a list of [h, w] maps")
    ids = ids.contiguous()
    B, H, W = ids.shape
    if buffers is None:
        buffers = ContourBuffers(B, H, W, cap, max_edges, ids.device, simplify=tol4 is not None)
    elif tol4 is not None and not buffers.simplify:
        raise ValueError("object_contours: a tolerance needs ContourBuffers(.., simplify=True)")
    elif (buffers.shape != (B, H, W) or buffers.device != ids.device or buffers.max_components != cap
          or (max_edges is not None and buffers.max_edges != int(max_edges))):
        raise ValueError(f"buffers were made for {buffers.shape}, {buffers.max_components} objects, {buffers.max_edges} edges "
                         f"on {buffers.device}; the ids are {(B, H, W)} with {cap} objects on {ids.device}")
    if tol4 is None:
        ops.seg_contours(ids, buffers.verts, buffers.rings, buffers.ring_off, buffers.n, buffers.ws, cap, connectivity)
        return _unlift(squeeze, dict({k: getattr(buffers, k) for k in _CONTOUR_KEYS}, shape=(H, W), connectivity=connectivity))
    ops.seg_contours(ids, buffers.verts, buffers.rings, buffers.ring_off, buffers.n, buffers.ws, cap, connectivity,
                     buffers.simp_verts, buffers.simp_rings, buffers.simp_n, tol4)
    c = _unlift(squeeze, dict({k: getattr(buffers, k) for k in _CONTOUR_KEYS}, shape=(H, W), connectivity=connectivity))
    s = _unlift(squeeze, dict(verts=buffers.simp_verts, rings=buffers.simp_rings, ring_off=buffers.ring_off, n=buffers.simp_n,
                              shape=(H, W), connectivity=connectivity))
    return dict(c, simplified=dict(s, tolerance=tolerance))


def object_contours(o, connectivity=8, max_edges=None, buffers=None, max_components=None, tolerance=None):
    """The outline of every object of an id map as rings of corner points.  o: a label_objects or fill_holes result -- the
    ids are o["ids"] and the objects outlined are 1..cap, cap = the rows of o["stats"] -- or an int32 device tensor [H, W] /
    [B, H, W] of ids (or a list of [h_i, w_i] maps) together with max_components=.  connectivity: 4 | 8, the one the ids
    were made with.

    Pixel (x, y) is the unit square from (x, y) to (x + 1, y + 1), so corners are lattice points 0..W x 0..H.  A ring runs
    clockwise on screen (y down) with the object on its right; its area is the integral of x dy: positive for an outer
    ring, negative for a hole ring.  Only corners are kept (no collinear points), the first being the first corner from the
    ring's smallest edge.  With connectivity 8 a ring may touch itself at a vertex where two pixels meet diagonally.

    Returns dict(verts, rings, ring_off, n, shape, connectivity), the tensors on the device:
      n         int32 [.., 4] = (unit edges found, corners, rings, complete).  complete = 0: the image has more edges than
                max_edges and NOTHING of it was written -- corners and rings are 0, ring_off is zero; size max_edges from
                n[.., 0] and call again
      rings     int32 [.., max_edges / 4, 4] = (id, first, count, area) sorted by id, an object's outer ring first and
                its hole rings behind it; rows from n[.., 2] on hold whatever the buffer held
      ring_off  int32 [.., cap + 1]: object k's rings are rows ring_off[k-1] .. ring_off[k]
      verts     int32 [.., max_edges, 2] = (X, Y): ring r's corners are rows first .. first + count
      shape     (H, W) of the map
    A list is handled with ONE CALL PER ITEM and every value of the result is then a list, as in label_objects; `buffers`
    is then a list of ContourBuffers or None.  buffers: a ContourBuffers of this shape and object count, reused call after
    call (the result aliases it); max_edges: rows per image for fresh buffers (ContourBuffers' default otherwise).  A fixed
    number of launches per call and no host synchronisation.

    tolerance: None, or pixels, a multiple of 0.25 in 0..8192.  The result then gains simplified = dict(verts, rings,
    ring_off, n, shape, connectivity, tolerance), the same rings simplified by Douglas-Peucker in the same call (three more
    launches; reused buffers must be ContourBuffers(.., simplify=True)) and of the same form as the result itself, so
    contours_to_host, rings_to_geojson and rings_to_coco take it unchanged: rings = (id, first, count, area) with the area
    of the ORIGINAL ring, n = (corners in, corners kept, rings, complete), ring_off shared.  Every ring keeps its first
    corner and at least three; tolerance 0 keeps every corner.  Douglas-Peucker preserves no topology: a simplified ring
    may touch or cross itself or a neighbour, and the shared border of two objects is simplified once from each side.
    Without a tolerance the result has exactly the keys above."""
    if connectivity not in (4, 8):
        raise ValueError(f"object_contours: connectivity must be 4 or 8, not {connectivity!r}")
    tol4 = _tol4(tolerance)
    ids, caps = _ids_caps(o, max_components, "object_contours", "outline")
    if isinstance(ids, (list, tuple)):
        keys = _CONTOUR_KEYS + ("shape", "connectivity")
        r = _per_item(lambda i, b: _contours_one(ids[i], caps[i], connectivity, max_edges, b, tol4, tolerance), len(ids),
                      (buffers,), "object_contours: one buffers entry per id map", keys + (("simplified",) if tol4 is not None else ()))
        if tol4 is not None:                                  # a list of dicts -> a dict of lists, like the result itself
            r["simplified"] = {k: [s[k] for s in r["simplified"]] for k in keys + ("tolerance",)}
        return r
    return _contours_one(ids, caps, connectivity, max_edges, buffers, tol4, tolerance)


def contours_to_host(c):
    """object_contours' result -> (per image a list over the objects 1..n of lists of (area, int32 numpy [k, 2] of (X, Y)),
    the outer ring first; incomplete) with TWO synchronising copies (per item for a list result): the tables n, ring_off
    and rings first, then verts[:corners] of every image and nothing behind it.  n = the highest object with a ring.
    incomplete: some image had more edges than max_edges; its list is empty.  A [H, W] result gives one image's list.
    The simplified form, object_contours(.., tolerance=)["simplified"], is taken the same way: its n holds the kept corners
    in column 1, and the areas are those of the original rings."""
    if isinstance(c["n"], (list, tuple)):
        per = [contours_to_host({k: v[i] for k, v in c.items() if isinstance(v, (list, tuple))}) for i in range(len(c["n"]))]
        return [p[0] for p in per], any(p[1] for p in per)
    n, ring_off, rings, verts = c["n"], c["ring_off"], c["rings"], c["verts"]
    single = n.dim() == 1
    if single:
        n, ring_off, rings, verts = n[None], ring_off[None], rings[None], verts[None]
    B, cap = ring_off.shape[0], ring_off.shape[1] - 1
    n, ring_off, rings = _to_host([n, ring_off, rings])                       # copy one: the tables
    verts = _to_host([verts[b, :int(n[b, 1])] for b in range(B)])              # copy two: the corners
    out = []
    for b in range(B):
        pts, off, nr = verts[b], ring_off[b], int(n[b, 2])
        top = int(np.searchsorted(off, nr, side="left")) if nr else 0        # the first k with ring_off[k] == rings
        out.append([[(int(a), pts[f:f + k]) for _, f, k, a in rings[b, off[o - 1]:off[o]].tolist()]
                    for o in range(1, min(top, cap) + 1)])
    incomplete = bool((n[:, 3] == 0).any())
    return (out[0] if single else out), incomplete


def _closed(pts):
    p = np.asarray(pts, dtype=np.int64).reshape(-1, 2).tolist()
    return p + p[:1]


def rings_to_geojson(rings):
    """One object's rings [(area, corners [k, 2])], the outer ring first (as contours_to_host lists them) -> {"type":
    "Polygon", "coordinates": [outer, hole, ..]}, every ring closed (its first point repeated at the end), in pixel-corner
    coordinates [x, y] with y growing downwards.  Orientation: in these coordinates the outer ring runs clockwise as seen
    on screen and the holes counter-clockwise; with y flipped to point up, as a map projection has it, that is
    counter-clockwise outside and clockwise inside, the right-hand rule of RFC 7946."""
    return {"type": "Polygon", "coordinates": [_closed(p) for _, p in rings]}


def rings_to_coco(rings):
    """One object's rings -> its OUTER ring as a flat [x0, y0, x1, y1, ..] list, one polygon of a COCO `segmentation`.
    COCO polygons have no holes: the hole rings are dropped, and the polygon then covers them.  For an exact mask use
    runs_to_coco on object_runs' result."""
    return [v for xy in np.asarray(rings[0][1], dtype=np.int64).reshape(-1, 2).tolist() for v in xy] if rings else []


def rings_to_mask(rings, h, w):
    """One object's rings [(area, corners [k, 2])] -> numpy bool [h, w], for RECTILINEAR rings only (object_contours'
    own; a simplified ring has slanted sides, which this ignores).  Every vertical side of a ring adds, for each row
    it spans, -1 at its column when it heads south (the object lies to its west) and +1 when it heads north; the
    cumulative sum along x is 1 inside and 0 outside."""
    acc = np.zeros((h, w + 1), np.int64)
    for _, pts in rings:
        p = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
        q = np.roll(p, -1, axis=0)
        for (x0, y0), (x1, y1) in zip(p.tolist(), q.tolist()):
            if x0 == x1 and y0 != y1:
                acc[min(y0, y1):max(y0, y1), x0] += -1 if y1 > y0 else 1
    return np.cumsum(acc, axis=1)[:, :w] > 0


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
        return ids, stats, _rows(stats)
    if not isinstance(o, (list, tuple)) or len(o) not in (2, 3):
        raise ValueError(f"match_objects: {what} must be a label_objects result or a tuple (ids, stats or None[, cap])")
    ids, stats = o[0], o[1]
    many = isinstance(ids, (list, tuple))
    if len(o) == 3:
        cap = [int(o[2])] * len(ids) if many else int(o[2])
    elif stats is None:
        raise ValueError(f"match_objects: {what} ids without a stats table need an explicit cap: (ids, None, cap)")
    else:
        cap = _rows(stats)
    if many and stats is None:
        stats = [None] * len(ids)
    return ids, stats, cap


def _match_one(pids, pstats, cap_p, gids, gstats, cap_g, skip, iou, nlabels, buffers):
    squeeze = pids.dim() == 2
    pids, gids, pstats, gstats, skip = _lift(squeeze, pids, gids, pstats, gstats, skip)
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
    return _unlift(squeeze, {k: getattr(buffers, k) for k in _MATCH_KEYS})


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
        return _per_item(lambda i, s, b: _match_one(pids[i], pstats[i], cap_p[i], gids[i], gstats[i], cap_g[i], s, iou,
                                                    nlabels, b),
                         k, (skip, buffers), "match_objects: one skip / buffers entry per id map", _MATCH_KEYS)
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
    names = ("n", "pair_off", "area", "match", "gmatch", "pq")
    out = dict(zip(names, _to_host([t[k] for k in names])))                    # copy one: the tables
    out["pairs"] = _to_host([t["pairs"][b, :int(out["n"][b, 0])] for b in range(B)])   # copy two
    truncated = bool((out["n"][:, 0] < out["n"][:, 1]).any() or (out["n"][:, 2] < out["n"][:, 3]).any())
    if single:
        out = {k: v[0] for k, v in out.items()}
    return out, truncated


# ------------------------------------------------------------------------------------------------ per-object confidence

def planes_for_classes(N, B):
    """The plane table of N-way class-major planes [N, B, 3, H, W] (segment_classes; dense segment_tiled with B = 1): int32
    [B, N + 1], label l of image b reads plane group (l - 1) * B + b; entry 0 is unused (-1)."""
    N, B = int(N), int(B)
    if N < 1 or B < 1:
        raise ValueError("planes_for_classes: N and B must be at least 1")
    t = torch.full((B, N + 1), -1, dtype=torch.int32)
    t[:, 1:] = (torch.arange(N, dtype=torch.int32) * B)[None, :] + torch.arange(B, dtype=torch.int32)[:, None]
    return t


def planes_for_binary(B):
    """The plane table of the binary routes' planes [B, 3, H, W]: int32 [B, 2], label 1 of image b reads plane group b."""
    return planes_for_classes(1, B)


def planes_for_candidates(candidates, nlabels, labels="global"):
    """The plane table of entry-major candidate planes [E, 3, H, W] (segment_candidates), from the lists that call takes:
    `candidates` is one sequence of set indices per query.  Entries are numbered as the route numbers them -- queries in
    order, each list in ascending set index (the route sorts it) -- and entry e of query i is read by label 1 + set index
    (labels="global", the route's "set") or 1 + position in the query's sorted list (labels="local").  Returns int32
    [b, nlabels + 1], -1 for a label the query does not list; a query may have no candidate.  ValueError for a label above
    nlabels, a set named twice by one query or another `labels`."""
    if labels not in ("global", "set", "local"):
        raise ValueError(f"planes_for_candidates: labels is 'global' or 'local', not {labels!r}")
    nlabels = int(nlabels)
    if nlabels < 1:
        raise ValueError("planes_for_candidates: nlabels must be at least 1")
    lists = [sorted(int(c) for c in (cs.tolist() if isinstance(cs, torch.Tensor) else cs)) for cs in candidates]
    t = torch.full((len(lists), nlabels + 1), -1, dtype=torch.int32)
    e = 0
    for i, cs in enumerate(lists):
        if len(set(cs)) != len(cs) or (cs and cs[0] < 0):
            raise ValueError(f"planes_for_candidates: query {i} names a set twice or a negative one ({cs})")
        for pos, c in enumerate(cs):
            lab = 1 + (pos if labels == "local" else c)
            if lab > nlabels:
                raise ValueError(f"planes_for_candidates: query {i} needs label {lab}, the table ends at {nlabels}")
            t[i, lab] = e
            e += 1
    return t


class ScoreBuffers:
    """Everything one object_scores call of a size writes, allocated once: scores int64 [B, cap, 4], the workspace, and the
    plane table twice -- planes_host, a pinned int32 [B, nlabels + 1] mirror, and planes, its device copy.  The shape of
    the maps is not part of it: the buffers depend on B, cap and nlabels only."""

    def __init__(self, B, cap, nlabels, device="cuda"):
        self.B, self.cap, self.nlabels = int(B), int(cap), int(nlabels)
        if min(self.B, self.cap) < 1 or not 1 <= self.nlabels <= 254:
            raise ValueError("ScoreBuffers: B and cap must be at least 1 and nlabels in 1..254")
        nbytes = ops.seg_scores_workspace(self.B, self.cap)
        if nbytes == 0:
            raise ValueError(f"seg_scores refuses these sizes: {self.B} images, {self.cap} objects")
        dev = torch.device(device)
        self.scores = torch.empty(self.B, self.cap, 4, dtype=torch.int64, device=dev)
        self.device = self.scores.device
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.planes = torch.empty(self.B, self.nlabels + 1, dtype=torch.int32, device=dev)
        self.planes_host = torch.empty(self.B, self.nlabels + 1, dtype=torch.int32).pin_memory()
        self._copied = None     # the event behind the last copy out of planes_host

    def stage(self, table):
        """table -> planes_host -> planes, the copy on the current stream.  Only the previous copy out of the mirror is
        waited for, on the host, before the mirror is overwritten; nothing else synchronises."""
        if self._copied is not None:
            self._copied.synchronize()
        self.planes_host.copy_(table)
        self.planes.copy_(self.planes_host, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record(torch.cuda.current_stream(self.device))


def _plane_table(planes, what="planes"):
    t = torch.as_tensor(planes)
    if t.is_cuda or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f"object_scores: {what} must be an integer HOST tensor or a nested list [B, nlabels + 1]")
    return t.to(torch.int32)


def _scores_one(ids, labels, cap, seg_u8, table, buffers):
    squeeze = ids.dim() == 2
    if squeeze:
        ids, labels = ids[None], (labels[None] if labels.dim() == 2 else labels)
    if ids.dim() != 3 or ids.dtype != torch.int32 or not ids.is_cuda:
        raise ValueError("object_scores takes int32 device ids [H, W] or [B, H, W], or a list of [h, w] maps")
    if labels.dtype != torch.uint8 or labels.shape != ids.shape:
        raise ValueError("object_scores: the labels must be uint8 and shaped like the ids")
    B, H, W = ids.shape
    if (not isinstance(seg_u8, torch.Tensor) or seg_u8.dtype != torch.uint8 or seg_u8.dim() < 3
            or tuple(seg_u8.shape[-3:]) != (3, H, W) or not seg_u8.is_contiguous() or seg_u8.device != ids.device):
        raise ValueError(f"object_scores: seg_u8 must be a contiguous uint8 tensor [..., 3, {H}, {W}] on {ids.device}")
    if table.dim() != 2 or table.shape[0] != B or not 2 <= table.shape[1] <= 255:
        raise ValueError(f"object_scores: the plane table must be [B, nlabels + 1] = [{B}, 2..255], got {tuple(table.shape)}")
    nlabels = table.shape[1] - 1
    if buffers is None:
        buffers = ScoreBuffers(B, cap, nlabels, ids.device)
    elif (buffers.B, buffers.cap, buffers.nlabels) != (B, cap, nlabels) or buffers.device != ids.device:
        raise ValueError(f"buffers were made for {buffers.B} images, {buffers.cap} objects, {buffers.nlabels} labels on "
                         f"{buffers.device}; the call has {B} images, {cap} objects, {nlabels} labels on {ids.device}")
    buffers.stage(table)
    ops.seg_scores(ids.contiguous(), labels.contiguous(), seg_u8.view(-1, 3, H, W), buffers.planes, buffers.planes_host,
                   buffers.scores, buffers.ws)
    return _unlift(squeeze, dict(scores=buffers.scores, planes=buffers.planes))


def object_scores(o, seg_u8, planes, buffers=None):
    """How sure the decoder is of every object: its mask planes reduced over the objects of a label map.  o: a label_objects
    result -- its ids, its (filtered) labels and the rows of its stats table (cap) are used.  seg_u8: any contiguous uint8
    device tensor whose last three axes are [3, H, W], viewed as P plane groups [P, 3, H, W].  planes: an int32 host tensor
    or nested list [B, nlabels + 1], the plane group that label l of image b reads, -1 for none (planes_for_classes /
    planes_for_binary / planes_for_candidates build it); it is staged in a pinned mirror and a device copy held by the
    buffers, and copied again on every call.

    A pixel is counted when its id lies in 1..cap, its label l in 1..nlabels and planes[b][l] in 0..P-1; its value is the
    sum of the three bytes of that plane group at the pixel, 0..765.  Returns dict(scores, planes) on the device: scores
    int64 [.., cap, 4] = (sum, counted pixels, min, max) of object id in row id - 1 -- zeros for an object without a
    counted pixel -- and planes, the device table the call read.  A [H, W] result gives the same without the batch axis.
    A list result (native sizes) is handled with ONE CALL PER ITEM: seg_u8 is then a list of [.., 3, h_i, w_i] tensors,
    planes one [1, nlabels + 1] table for every item or a list of them, buffers a list of ScoreBuffers or None, and every
    value of the result is a list.  buffers: a ScoreBuffers of this B, cap and nlabels, reused call after call (the result
    aliases it).  Three launches and one small copy per call, no host synchronisation."""
    ids, labels, stats = o["ids"], o["labels"], o["stats"]
    if isinstance(ids, (list, tuple)):
        k = len(ids)
        if not isinstance(seg_u8, (list, tuple)) or len(seg_u8) != k:
            raise ValueError("object_scores: one seg_u8 tensor per id map")
        if isinstance(planes, (list, tuple)) and len(planes) == k and all(_plane_table(p).dim() == 2 for p in planes):
            tabs = [_plane_table(p) for p in planes]
        else:
            tabs = [_plane_table(planes)] * k
        return _per_item(lambda i, b: _scores_one(ids[i], labels[i], stats[i].shape[-2], seg_u8[i], tabs[i], b), k,
                         (buffers,), "object_scores: one buffers entry per id map", ("scores", "planes"))
    return _scores_one(ids, labels, stats.shape[-2], seg_u8, _plane_table(planes), buffers)


def scores_to_host(s):
    """object_scores' result -> dict(sum, n, min, max, mean) of numpy arrays [B, cap] ([cap] for a [H, W] result; a list of
    such dicts for a list result), with ONE synchronising copy (per item for a list result).  sum, n, min and max are the
    int64 columns of the table; mean = sum / (765 * n) as float64, the object's confidence in 0..1, and 0 where n == 0."""
    if isinstance(s["scores"], (list, tuple)):
        return [scores_to_host({"scores": t}) for t in s["scores"]]
    t = s["scores"].cpu().numpy()                                    # the one copy
    out = dict(sum=t[..., 0], n=t[..., 1], min=t[..., 2], max=t[..., 3])
    out["mean"] = _mean_score(out["sum"], out["n"])
    return out


def _mean_score(total, n):
    total, n = np.asarray(total, dtype=np.int64), np.asarray(n, dtype=np.int64)
    return np.where(n > 0, total.astype(np.float64) / np.maximum(765 * n, 1).astype(np.float64), 0.0)


def coco_results(o_host, runs_host, scores_host, image_id, category_ids, h, w):
    """COCO result records of ONE image from its three host tables: o_host, the image's list from objects_to_host;
    runs_host, the image's list from runs_to_host (column order); scores_host, the image's dict from scores_to_host.
    Returns, for the objects 1..min(n, cap) in id order, a list of {"image_id", "category_id" = category_ids[label - 1],
    "segmentation" = runs_to_coco(runs, h, w), "bbox" = [x, y, width, height] from the half-open box, "area", "score" = the
    mean above}.  Host only: no copy of its own."""
    out = []
    for k, (label, area, (y0, x0, y1, x1), _first) in enumerate(o_host):
        runs = runs_host[k] if k < len(runs_host) else np.zeros((0, 2), np.int32)
        total, n = int(scores_host["sum"][k]), int(scores_host["n"][k])
        out.append({"image_id": image_id, "category_id": category_ids[label - 1],
                    "segmentation": runs_to_coco(runs, h, w), "bbox": [int(x0), int(y0), int(x1 - x0), int(y1 - y0)],
                    "area": int(area), "score": float(_mean_score(total, n))})
    return out


def detections_to_host(o, s, m):
    """What metrics.average_precision ranks, from a label_objects result o, its object_scores s and its match_objects m
    against the ground truth, with ONE synchronising copy (per item for list results) of n, column 0 of stats, scores, and
    m's match, area and pq.  m must have been made with iou=(1, 2): its match table then holds every partner above 1/2, so
    every stricter threshold is decided from (inter, union) alone.

    Returns (dets, npos).  dets: per image an int64 array [k, 5] = (class, sum, n, inter, union) of every object p in id
    order that has n > 0 counted score pixels and a counted pixel in m (area[p] > 0), inter and union 0 without a partner;
    one array for a [H, W] result, a list over the images otherwise.  npos: int64 [nlabels + 1] = TP + FN of m's pq, summed
    over the images: the ground-truth objects of every class."""
    if isinstance(o["n"], (list, tuple)):
        per = [detections_to_host({k: v[i] for k, v in o.items()}, {k: v[i] for k, v in s.items()},
                                  {k: v[i] for k, v in m.items()}) for i in range(len(o["n"]))]
        return [p[0] for p in per], np.sum([p[1] for p in per], axis=0)
    single = o["n"].dim() == 1
    n, stats, scores, match, area, pq = _lift(single, o["n"], o["stats"], s["scores"], m["match"], m["area"], m["pq"])
    B, cap = stats.shape[:2]
    if scores.shape[:2] != (B, cap) or match.shape[:2] != (B, cap):
        raise ValueError("detections_to_host: o, s and m must describe the same images and the same number of objects")
    n, cls, match, area, scores, pq = _to_host([n, stats[:, :, 0], match, area[:, 1:cap + 1], scores, pq])   # the one copy
    dets = []
    for b in range(B):
        k = min(int(n[b, 0]), cap)
        keep = (scores[b, :k, 1] > 0) & (area[b, :k] > 0)
        paired = match[b, :k, 0] > 0
        rows = np.stack([cls[b, :k].astype(np.int64), scores[b, :k, 0], scores[b, :k, 1],
                         np.where(paired, match[b, :k, 1], 0).astype(np.int64),
                         np.where(paired, match[b, :k, 2], 0).astype(np.int64)], axis=1)
        dets.append(rows[keep])
    npos = (pq[:, :, 0] + pq[:, :, 2]).sum(axis=0)
    return (dets[0] if single else dets), npos


# ------------------------------------------------------------------------------------------------ boundary bands

_BOUNDARY_DMAX = 254
_BOUNDARY_METRICS = ("chessboard", "euclidean")


class BoundaryBuffers:
    """Everything one boundary_bands call of a shape writes, allocated once: dist uint8 [B, H, W], band [B, H, W] of the
    map's dtype (torch.uint8 for label maps, torch.int32 for id maps) and the workspace.  dmax is the search radius of the
    calls that use the buffers without naming one.  metric="euclidean": dist is uint16 and holds squared distances;
    max_components (with it, for int32 id maps): peaks int64 [B, max_components], what object_thickness writes."""

    def __init__(self, B, H, W, dmax, dtype=torch.uint8, device="cuda", metric="chessboard", max_components=None):
        self.shape, self.dmax, self.dtype, self.metric = (int(B), int(H), int(W)), int(dmax), dtype, metric
        if dtype not in (torch.uint8, torch.int32):
            raise ValueError("BoundaryBuffers: dtype must be torch.uint8 (label maps) or torch.int32 (id maps)")
        if not 1 <= self.dmax <= _BOUNDARY_DMAX:
            raise ValueError(f"BoundaryBuffers: dmax must lie in 1..{_BOUNDARY_DMAX}, got {self.dmax}")
        if metric not in _BOUNDARY_METRICS:
            raise ValueError(f"BoundaryBuffers: metric must be one of {_BOUNDARY_METRICS}, got {metric!r}")
        self.max_components = None if max_components is None else int(max_components)
        if self.max_components is not None and (metric != "euclidean" or dtype != torch.int32 or self.max_components < 1):
            raise ValueError("BoundaryBuffers: max_components (>= 1) goes with metric='euclidean' and torch.int32")
        nbytes = ops.seg_boundary_workspace(*self.shape, 1 if dtype == torch.uint8 else 4)
        if nbytes == 0:
            raise ValueError(f"seg_boundary refuses these sizes: {self.shape}")
        dev = torch.device(device)
        self.dist = torch.empty(self.shape, dtype=torch.uint16 if metric == "euclidean" else torch.uint8, device=dev)
        self.device = self.dist.device
        self.band = torch.empty(self.shape, dtype=dtype, device=dev)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.peaks = None
        if self.max_components is not None:
            self.peaks = torch.empty(self.shape[0], self.max_components, dtype=torch.int64, device=dev)


def _bands_one(m, d, ratio, dmax, buffers, metric="chessboard"):
    if metric not in _BOUNDARY_METRICS:
        raise ValueError(f"boundary_bands: metric must be one of {_BOUNDARY_METRICS}, got {metric!r}")
    squeeze = m.dim() == 2
    m, = _lift(squeeze, m)
    if m.dim() != 3 or m.dtype not in (torch.uint8, torch.int32) or not m.is_cuda:
        raise ValueError("boundary_bands takes a uint8 or int32 device tensor [H, W] or [B, H, W], or a list of [h, w] maps")
    B, H, W = m.shape
    if d is None:
        from .metrics import boundary_width
        d = boundary_width(H, W, ratio)
    d = int(d)
    if dmax is None:
        dmax = d if buffers is None else buffers.dmax
    dmax = int(dmax)
    if d > _BOUNDARY_DMAX or dmax > _BOUNDARY_DMAX:
        raise ValueError(f"boundary_bands: a band of {max(d, dmax)} pixels is above the limit of {_BOUNDARY_DMAX} (dist is a "
                         f"byte): at ratio 0.02 that is an image diagonal of about 12 700 pixels")
    if d < 1 or dmax < d:
        raise ValueError(f"boundary_bands: the width must lie in 1..dmax, got d = {d}, dmax = {dmax}")
    if buffers is None:
        buffers = BoundaryBuffers(B, H, W, dmax, m.dtype, m.device, metric)
    elif buffers.shape != (B, H, W) or buffers.device != m.device or buffers.dtype != m.dtype:
        raise ValueError(f"buffers were made for {buffers.shape} of {buffers.dtype} on {buffers.device}, the map is "
                         f"{(B, H, W)} of {m.dtype} on {m.device}")
    elif buffers.metric != metric:
        raise ValueError(f"buffers were made for the {buffers.metric} metric, the call asks for {metric}")
    if metric == "chessboard":
        ops.seg_boundary(m.contiguous(), buffers.dist, buffers.ws, dmax, band=buffers.band, d=d)
        return _unlift(squeeze, dict(dist=buffers.dist, band=buffers.band, d=d, dmax=dmax))
    ops.seg_boundary(m.contiguous(), buffers.dist, buffers.ws, dmax, band=buffers.band, d=d, metric=metric)
    return _unlift(squeeze, dict(dist2=buffers.dist, band=buffers.band, d=d, dmax=dmax, metric=metric))


def boundary_bands(m, d=None, ratio=0.02, dmax=None, buffers=None, metric="chessboard"):
    """Distance to the contour and the boundary band of a label map or an id map.  m: a uint8 or int32 device tensor [H, W]
    or [B, H, W] (0 = background; every other value, 255 and negative ints included, is an object value, compared for
    equality only), or a LIST of [h_i, w_i] maps.  d: the band's width in pixels, by default metrics.boundary_width(H, W,
    ratio) = 2 % of the image diagonal; dmax: the search radius, d by default (or the buffers' dmax), at most 254 -- a
    larger d is a ValueError.

    Returns dict(dist, band, d, dmax) on the device: dist uint8, 0 on background, else min(D, dmax + 1) with D the
    chessboard distance to the nearest position outside the image or of another value (1 on the contour), so one dist
    answers every width up to dmax; band, of m's dtype, the value where 1 <= dist <= d and 0 elsewhere -- for the mask of
    one value exactly mask - eroded of the published mask_to_boundary.  A [H, W] input gives the same without the batch
    axis.  A list is handled with ONE CALL PER ITEM, d comes from each item's own size, and every value of the result is a
    list; buffers is then a list of BoundaryBuffers or None.  buffers: a BoundaryBuffers of this shape and dtype, reused
    call after call (the result aliases it).  Two launches per call and no host synchronisation.

    metric="euclidean" measures the true distance: the result is dict(dist2, band, d, dmax, metric) with dist2 uint16, 0 on
    background, else min(D2, (dmax + 1)^2), D2 the smallest dy^2 + dx^2 to a position outside the image or of another value,
    and band the value where 1 <= dist2 <= d^2 -- a 45-degree edge is sqrt(2) times farther away than the chessboard
    distance says.  The buffers are then BoundaryBuffers(..., metric="euclidean")."""
    if isinstance(m, (list, tuple)):
        ds = d if isinstance(d, (list, tuple)) else [d] * len(m)
        keys = ("dist", "band", "d", "dmax") if metric == "chessboard" else ("dist2", "band", "d", "dmax", "metric")
        return _per_item(lambda i, di, b: _bands_one(m[i], di, ratio, dmax, b, metric), len(m), (ds, buffers),
                         "boundary_bands: one d / buffers entry per map", keys)
    return _bands_one(m, d, ratio, dmax, buffers, metric)


def object_boundaries(o, d=None, ratio=0.02, dmax=None, buffers=None, metric="chessboard"):
    """boundary_bands of both maps of a label_objects result o: its (filtered) labels, whose band feeds boundary_counts,
    and its ids, whose band is an id map that match_objects takes (per-object Boundary IoU, see the module docstring).
    buffers: dict(labels=BoundaryBuffers of uint8, ids=BoundaryBuffers of int32) -- of lists of them for a list result --
    or None.  Returns dict(labels, ids, d): two boundary_bands results and the width they share (a list for a list).
    metric: boundary_bands' -- with "euclidean" both results hold dist2 and name the metric."""
    buffers = buffers or {}
    lab = boundary_bands(o["labels"], d, ratio, dmax, buffers.get("labels"), metric)
    ids = boundary_bands(o["ids"], lab["d"], ratio, dmax, buffers.get("ids"), metric)
    return dict(labels=lab, ids=ids, d=lab["d"])


def _bcounts_one(bp, bg, pred, gt, nlabels, d, counts):
    squeeze = pred.dim() == 2
    if ("dist2" in bp) != ("dist2" in bg):
        raise ValueError("boundary_counts: both dist maps must be of one metric")
    key = "dist2" if "dist2" in bp else "dist"
    pdist, gdist = bp[key], bg[key]
    if squeeze:
        pred, gt, pdist, gdist = pred[None], (gt[None] if gt.dim() == 2 else gt), pdist[None], gdist[None]
    if pred.dim() != 3 or pred.dtype != torch.uint8 or not pred.is_cuda:
        raise ValueError("boundary_counts takes uint8 device label maps [H, W] or [B, H, W], or lists of [h, w] maps")
    if gt.dtype != torch.uint8 or gt.shape != pred.shape:
        raise ValueError("boundary_counts: gt must be uint8 and shaped like pred")
    if pdist.shape != pred.shape or gdist.shape != pred.shape:
        raise ValueError("boundary_counts: the dist maps must be shaped like pred")
    nlabels = int(nlabels)
    if not 1 <= nlabels <= 254:
        raise ValueError("boundary_counts: nlabels must lie in 1..254")
    d = int(bp["d"] if d is None else d)
    if d < 1 or d > min(bp.get("dmax", d), bg.get("dmax", d)):
        raise ValueError(f"boundary_counts: d = {d} is outside 1..dmax of the dist maps")
    B = pred.shape[0]
    if counts is None:
        counts = torch.empty(B, 2, nlabels + 1, dtype=torch.int64, device=pred.device)
    elif squeeze and counts.dim() == 2:
        counts = counts[None]
    ops.seg_boundary_counts(pred.contiguous(), pdist.contiguous(), gt.contiguous(), gdist.contiguous(), counts, d)
    return counts[0] if squeeze else counts


def boundary_counts(bp, bg, pred, gt, nlabels, d=None, counts=None):
    """Per-class counts of the boundary band of a prediction against that of a ground truth.  bp, bg: boundary_bands
    results of the two uint8 label maps pred and gt (device tensors [H, W] / [B, H, W], or lists of [h_i, w_i] maps; the
    four then are lists, handled with one call per item).  d: the width, bp's by default; any width up to the dmax both
    dist maps were made with.  A pixel with gt > nlabels (255 included) is dropped; otherwise it counts for its predicted
    class when it lies in the prediction's band and for its true class when it lies in the ground truth's band, for bin 0
    otherwise.  The ground truth's distance was taken on the map as given: 255 is a value like any other there, so a class
    pixel beside an ignore region lies in the band -- the published method has no ignore label, and treating the unknown
    as "other" needs no second rule.

    bp and bg may both be results of metric="euclidean": the band is then 1 <= dist2 <= d^2.

    Returns counts int64 [.., 2, nlabels + 1] = (intersections, unions) on the device, the layout of label_objects'
    counts: metrics.boundary_iou(counts) is Boundary IoU per class and its mean.  counts (optional): the buffer to write,
    reused call after call.  Two launches per call and no host synchronisation."""
    if isinstance(pred, (list, tuple)):
        k = len(pred)
        cs = counts if counts is not None else [None] * k
        ds = d if isinstance(d, (list, tuple)) else [d] * k
        if not isinstance(gt, (list, tuple)) or len(gt) != k or len(bp["band"]) != k or len(bg["band"]) != k or len(cs) != k:
            raise ValueError("boundary_counts: one gt, one dist pair and one counts entry per predicted map")
        item = lambda r, i: {key: v[i] for key, v in r.items()}  # noqa: E731
        return [_bcounts_one(item(bp, i), item(bg, i), pred[i], gt[i], nlabels, ds[i], cs[i]) for i in range(k)]
    return _bcounts_one(bp, bg, pred, gt, nlabels, d, counts)


# ------------------------------------------------------------------------------------------------ thickness and cores

def _thickness_one(ids, n, cap, dmax, buffers):
    squeeze = ids.dim() == 2
    ids, n = _lift(squeeze, ids, n)
    if ids.dim() != 3 or ids.dtype != torch.int32 or not ids.is_cuda:
        raise ValueError("object_thickness takes the int32 device ids [H, W] or [B, H, W] of a label_objects or fill_holes result")
    B, H, W = ids.shape
    if dmax is None:
        dmax = _BOUNDARY_DMAX if buffers is None else buffers.dmax
    dmax = int(dmax)
    if not 1 <= dmax <= _BOUNDARY_DMAX:
        raise ValueError(f"object_thickness: dmax must lie in 1..{_BOUNDARY_DMAX}, got {dmax}")
    if buffers is None:
        buffers = BoundaryBuffers(B, H, W, dmax, torch.int32, ids.device, "euclidean", cap)
    elif (buffers.shape != (B, H, W) or buffers.device != ids.device or buffers.dtype != torch.int32
          or buffers.metric != "euclidean" or buffers.max_components != cap):
        raise ValueError(f"object_thickness: the buffers must be BoundaryBuffers({B}, {H}, {W}, dmax, torch.int32, "
                         f"metric='euclidean', max_components={cap}) on {ids.device}")
    ops.seg_boundary(ids.contiguous(), buffers.dist, buffers.ws, dmax, metric="euclidean", peaks=buffers.peaks)
    return _unlift(squeeze, dict(dist2=buffers.dist, peaks=buffers.peaks, n=n, dmax=dmax, shape=(H, W)))


def object_thickness(o, dmax=None, buffers=None):
    """How THICK every object is and where its MIDDLE lies: the largest inscribed circle of every object of a label_objects
    or fill_holes result o, from the Euclidean distance of its ids to their own contour (ops.seg_boundary with
    metric="euclidean" and peaks).  dmax: the largest radius told apart, 1..254, by default 254 (or the buffers'); the
    column walk costs O(min(distance, dmax)) a pixel.  buffers: BoundaryBuffers(B, H, W, dmax, torch.int32,
    metric="euclidean", max_components=rows of o's stats), reused call after call, or None; a list of them for a list
    result, which is handled with one call per item.

    Returns dict(dist2, peaks, n, dmax, shape), everything on the device:
      dist2   uint16 [.., H, W]: 0 on background, else min(D2, (dmax + 1)^2), D2 the smallest dy^2 + dx^2 to a position
              outside the image or of another id; (dmax + 1)^2 means "at least dmax + 1"
      peaks   int64 [.., max_components]: row id - 1 = (r2 << 32) | (0xFFFFFFFF - (y * W + x)), r2 the largest dist2 of the
              object -- the squared radius of its largest inscribed circle, a circle of radius sqrt(r2) around the centre of
              pixel (y, x) that reaches no farther than the centre of the nearest foreign pixel -- and (y, x) the first
              pixel in row-major order that has it: a label point that lies INSIDE the object, which a box centre or a
              centroid need not.  0 for an id without a pixel
      n       o's n, which thickness_to_host reads;  shape = (H, W)
    Three launches per call and no host synchronisation."""
    if not isinstance(o, dict) or "ids" not in o or "stats" not in o or "n" not in o:
        raise ValueError("object_thickness takes a label_objects or fill_holes result")
    ids, caps = _ids_caps(o, None, "object_thickness", "measure")
    if isinstance(ids, (list, tuple)):
        return _per_item(lambda i, b: _thickness_one(ids[i], o["n"][i], caps[i], dmax, b), len(ids), (buffers,),
                         "object_thickness: one buffers entry per item", ("dist2", "peaks", "n", "dmax", "shape"))
    return _thickness_one(ids, o["n"], caps, dmax, buffers)


def thickness_to_host(t):
    """object_thickness' result -> per image a list of (r2, (y, x), capped) over the objects in id order, with ONE
    synchronising copy of n and peaks (per item for a list result): r2 the squared radius of the largest inscribed circle,
    (y, x) its centre, capped True when r2 == (dmax + 1)^2, i.e. the radius is at least dmax + 1.  The list ends at the
    result's object count or at the table's last row; an id without a pixel gives (0, None, False).  A [H, W] result
    gives one image's list."""
    if not isinstance(t, dict) or any(k not in t for k in ("peaks", "n", "dmax", "shape")):
        raise ValueError("thickness_to_host takes an object_thickness result")
    if isinstance(t["peaks"], (list, tuple)):
        return [thickness_to_host({k: v[i] for k, v in t.items()}) for i in range(len(t["peaks"]))]
    single = t["peaks"].dim() == 1
    n, peaks = _lift(single, t["n"], t["peaks"])
    if peaks.dim() != 2 or peaks.dtype != torch.int64 or n.shape[0] != peaks.shape[0]:
        raise ValueError("thickness_to_host: peaks must be int64 [B, cap] and n must describe the same images")
    W, full = int(t["shape"][1]), (int(t["dmax"]) + 1) ** 2
    n, peaks = _to_host([n, peaks])                                   # the one copy
    out = []
    for b in range(peaks.shape[0]):
        rows = []
        for key in peaks[b, :min(int(n[b, 0]), peaks.shape[1])].tolist():
            r2, pos = key >> 32, 0xFFFFFFFF - (key & 0xFFFFFFFF)
            rows.append((r2, divmod(pos, W), r2 == full) if key else (0, None, False))
        out.append(rows)
    return out[0] if single else out


def _cores_one(o, radius, kw):
    t = object_thickness(o, dmax=max(radius, 1))
    d2 = t["dist2"].view(torch.int16).to(torch.int32) & 0xFFFF       # uint16 as integers every torch op takes
    labels = torch.where(d2 > radius * radius, o["labels"], torch.zeros_like(o["labels"]))
    return label_objects(labels, **kw)


def object_cores(o, radius, **label_objects_kwargs):
    """How many SEPARATE things an object is: the cores of a label_objects or fill_holes result o, its pixels farther than
    `radius` (an integer, 0..254) from their object's contour, labelled again -- two blobs that touch over a neck of up to
    2 * radius pixels fall apart, slivers thinner than that vanish.  A composition with no kernel of its own:
    object_thickness(o, dmax=radius), o's labels kept where dist2 > radius^2, then label_objects(those labels,
    **label_objects_kwargs) -- gt, connectivity, min_area, max_components, nlabels.  Returns label_objects' result for
    the cores (a dict of lists for a list result, one call per item)."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= _BOUNDARY_DMAX:
        raise ValueError(f"object_cores: radius must be an integer in 0..{_BOUNDARY_DMAX}, got {radius!r}")
    if "buffers" in label_objects_kwargs:
        raise ValueError("object_cores allocates its own buffers")
    if not isinstance(o, dict) or any(k not in o for k in ("ids", "labels", "stats", "n")):
        raise ValueError("object_cores takes a label_objects or fill_holes result")
    radius = int(radius)
    if isinstance(o["ids"], (list, tuple)):
        kw = label_objects_kwargs
        gts = kw.get("gt") or [None] * len(o["ids"])
        per = [_cores_one({k: v[i] for k, v in o.items()}, radius, dict(kw, gt=gts[i])) for i in range(len(o["ids"]))]
        return {key: [p[key] for p in per] for key in per[0]}
    return _cores_one(o, radius, label_objects_kwargs)


# ------------------------------------------------------------------------------------------------ instances

_SPLIT_KEYS = ("ids", "labels", "n", "stats", "counts", "parent", "cores", "nearest")


class SplitBuffers:
    """Everything one split_objects call of a shape writes, allocated once: `thick` (BoundaryBuffers of the Euclidean
    distance, with peaks), `seeds` (ComponentBuffers of the cores), nearest int32 [B, H, W], dist uint16 [B, H, W] and ws
    (what nearest_seeds writes, which takes these buffers as well), `out` (ComponentBuffers of the instances) and parent
    int32 [B, max_components].  max_components: the rows of the stats table of the result that is split, and of both
    tables made here.  A later call with the same buffers overwrites them."""

    def __init__(self, B, H, W, max_components=1024, device="cuda"):
        self.shape, self.max_components = (int(B), int(H), int(W)), int(max_components)
        if self.max_components < 1:
            raise ValueError("max_components must be at least 1")
        nbytes = ops_split.seg_nearest_workspace(*self.shape)
        if nbytes == 0:
            raise ValueError(f"seg_nearest refuses these sizes: {self.shape}")
        dev = torch.device(device)
        self.nearest = torch.empty(self.shape, dtype=torch.int32, device=dev)
        self.device = self.nearest.device
        self.dist = torch.empty(self.shape, dtype=torch.uint16, device=dev)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.parent = torch.empty(self.shape[0], self.max_components, dtype=torch.int32, device=dev)
        self.thick = BoundaryBuffers(B, H, W, _BOUNDARY_DMAX, torch.int32, dev, "euclidean", self.max_components)
        self.seeds = ComponentBuffers(B, H, W, self.max_components, dev)
        self.out = ComponentBuffers(B, H, W, self.max_components, dev)


def _nearest_one(ids, seeds, reach, passes, buffers):
    squeeze = ids.dim() == 2
    ids, seeds = _lift(squeeze, ids, seeds)
    if ids.dim() != 3 or ids.dtype != torch.int32 or not ids.is_cuda:
        raise ValueError("nearest_seeds takes an int32 device map [H, W] or [B, H, W], or a list of [h, w] maps")
    if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.int32 or seeds.shape != ids.shape:
        raise ValueError("nearest_seeds: seeds must be an int32 tensor shaped like the map")
    if isinstance(reach, bool) or not isinstance(reach, (int, np.integer)) or not 1 <= reach <= _BOUNDARY_DMAX:
        raise ValueError(f"nearest_seeds: reach must be an integer in 1..{_BOUNDARY_DMAX}, got {reach!r}")
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 1 <= passes <= 8:
        raise ValueError(f"nearest_seeds: passes must be an integer in 1..8, got {passes!r}")
    B, H, W = ids.shape
    if buffers is None:
        nearest = torch.empty_like(ids, memory_format=torch.contiguous_format)
        dist = torch.empty(B, H, W, dtype=torch.uint16, device=ids.device)
        ws = torch.empty(ops_split.seg_nearest_workspace(B, H, W), dtype=torch.uint8, device=ids.device)
    elif buffers.shape != (B, H, W) or buffers.device != ids.device:
        raise ValueError(f"buffers were made for {buffers.shape} on {buffers.device}, the map is {(B, H, W)} on {ids.device}")
    else:
        nearest, dist, ws = buffers.nearest, buffers.dist, buffers.ws
    ops_split.seg_nearest(ids.contiguous(), seeds.contiguous(), nearest, dist, ws, int(reach), int(passes))
    return _unlift(squeeze, dict(nearest=nearest, dist=dist, reach=int(reach), passes=int(passes), shape=(H, W)))


def nearest_seeds(ids, seeds, reach, passes=1, buffers=None):
    """For every pixel of an id map, the nearest seed that an L path INSIDE its object reaches (ops_split.seg_nearest).
    ids: an int32 device tensor [H, W] or [B, H, W] (0 = background, values compared for equality only), or a list of
    [h_i, w_i] maps; seeds: int32, shaped like it, every non-zero value a seed -- any map, not only cores.  A candidate
    of pixel (y, x) is a seed (y + dy, x + dx) with dy^2 + dx^2 <= reach^2 (reach 1..254) such that column x from row y to
    row y + dy and then row y + dy from x to x + dx hold the pixel's id; the candidate with the smallest (dy^2 + dx^2, seed
    value) wins.  passes (1..8) repeats that with the result as seeds: a pixel that holds a value keeps it, the others look
    again, so each pass carries every label round one more bend.  buffers: a SplitBuffers of this shape, or None.

    Returns dict(nearest, dist, reach, passes, shape) on the device: nearest int32, the winner's value, 0 without a
    candidate and on background; dist uint16, 0 on a seed and on background, else the winner's dy^2 + dx^2 (in the pass
    that gave the pixel its value), (reach + 1)^2 without a candidate.  2 * passes launches and no host synchronisation."""
    if isinstance(ids, (list, tuple)):
        if not isinstance(seeds, (list, tuple)) or len(seeds) != len(ids):
            raise ValueError("nearest_seeds: one seed map per id map")
        return _per_item(lambda i, b: _nearest_one(ids[i], seeds[i], reach, passes, b), len(ids), (buffers,),
                         "nearest_seeds: one buffers entry per item", ("nearest", "dist", "reach", "passes", "shape"))
    return _nearest_one(ids, seeds, reach, passes, buffers)


def _split_one(o, radius, reach, passes, min_area, connectivity, buffers):
    squeeze = o["ids"].dim() == 2
    ids, labels, n, stats = _lift(squeeze, o["ids"], o["labels"], o["n"], o["stats"])
    if ids.dim() != 3 or ids.dtype != torch.int32 or labels.dtype != torch.uint8 or labels.shape != ids.shape or not ids.is_cuda:
        raise ValueError("split_objects takes a label_objects or fill_holes result")
    B, H, W = ids.shape
    cap = stats.shape[-2]
    if buffers is not None and (buffers.shape != (B, H, W) or buffers.device != ids.device or buffers.max_components != cap):
        raise ValueError(f"split_objects: the buffers must be SplitBuffers({B}, {H}, {W}, max_components={cap}) on {ids.device}")
    o3 = dict(ids=ids, labels=labels, n=n, stats=stats)
    t = object_thickness(o3, dmax=max(radius, 1), buffers=buffers.thick if buffers else None)
    d2 = t["dist2"].view(torch.int16).to(torch.int32) & 0xFFFF       # uint16 as integers every torch op takes
    core = torch.where(d2 > radius * radius, labels, torch.zeros_like(labels))
    cores = label_objects(core, connectivity=connectivity, max_components=cap, buffers=buffers.seeds if buffers else None)
    near = nearest_seeds(ids, cores["ids"], reach, passes, buffers)
    r = label_objects(labels, connectivity=connectivity, min_area=min_area, max_components=cap,
                      buffers=buffers.out if buffers else None, keys=near["nearest"])
    # parent: o's id at every instance's first pixel, 0 behind the last instance
    first = r["stats"][..., 6].to(torch.int64)
    rows = torch.arange(cap, device=ids.device)[None] < r["n"][:, :1]
    parent = torch.where(rows, torch.gather(ids.reshape(B, H * W), 1, first), torch.zeros((), dtype=torch.int32, device=ids.device))
    if buffers is not None:
        parent = buffers.parent.copy_(parent)
    return _unlift(squeeze, dict(r, parent=parent, cores=cores["n"], nearest=near["nearest"]))


def split_objects(o, radius, reach=None, passes=3, min_area=0, buffers=None, connectivity=8):
    """Touching objects as separate INSTANCES: the cores of a label_objects or fill_holes result o (object_cores' rule:
    the pixels with dist2 > radius^2, labelled again) grown back over their objects.  A composition: object_thickness(o,
    dmax=radius), the cores, nearest_seeds(o's ids, the cores' ids, reach, passes), then label_objects(o's labels,
    keys=nearest, connectivity, min_area, max_components=rows of o's stats).  radius: an integer in 0..254.  reach: how far
    a pixel looks for a core, by default min(254, 2 * radius + 2); passes: 3 by default.  Both defaults are choices, not
    measurements: a pixel within `radius` of a core pixel is always reached in one pass when reach >= radius, the rest of a
    ragged object takes bends, one per pass.  connectivity: the one o was labelled with (a result does not carry it), used
    for the cores and for the instances.  buffers: a SplitBuffers of o's shape and rows, or None (a list for a list).

    An object without a core keeps key 0 everywhere and comes out as the one object it was.  Pixels of an object with a
    core that no pass reaches keep key 0 as well and form instances of their own; min_area removes them like any speck.

    Returns a label_objects result of the instances -- ids, labels, n, stats, counts (None) -- which every stage that takes
    one takes unchanged, with three more entries:
      parent   int32 [.., max_components]: row k - 1 = the id in o of instance k (o's id at the instance's first pixel), 0
               from row min(n, max_components) on
      cores    the cores' n, int32 [.., 2]
      nearest  int32 [.., H, W], nearest_seeds' map: the core id every pixel took, 0 for none
    A list result is handled with one call per item.  No host synchronisation."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= _BOUNDARY_DMAX:
        raise ValueError(f"split_objects: radius must be an integer in 0..{_BOUNDARY_DMAX}, got {radius!r}")
    if not isinstance(o, dict) or any(k not in o for k in ("ids", "labels", "stats", "n")):
        raise ValueError("split_objects takes a label_objects or fill_holes result")
    radius = int(radius)
    reach = min(_BOUNDARY_DMAX, 2 * radius + 2) if reach is None else reach
    if isinstance(o["ids"], (list, tuple)):
        return _per_item(lambda i, b: _split_one({k: o[k][i] for k in ("ids", "labels", "stats", "n")}, radius, reach, passes,
                                                 min_area, connectivity, b),
                         len(o["ids"]), (buffers,), "split_objects: one buffers entry per item", _SPLIT_KEYS)
    return _split_one(o, radius, reach, passes, min_area, connectivity, buffers)
