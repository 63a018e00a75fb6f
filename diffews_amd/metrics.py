"""Episode metric: intersection/union accumulation and mIoU / FB-IoU, plus the multi-GPU reduction.

Counterpart of `Evaluator.classify_prediction`
(/root/reference/evaluation_util/common/evaluation.py:12-39) and `AverageMeter`
(/root/reference/evaluation_util/common/logger.py:12-51).  The per-episode counts come from the
on-device kernel `dfw_seg_postprocess` (or from `classify_prediction` below for ready-made masks).

Deliberate difference: the reference accumulates pixel counts in fp32 `[2, nclass]` buffers, exact
only below 2**24 per cell; one COCO class cell receives ~50 episodes x 262144 px.  Here the buffers
are int64 (order-independent => bit-identical for any GPU count) and are converted to fp32 only inside
`compute_iou`, which then follows logger.py:42-51 literally.  The all-reduce of the two buffers is the
only collective on the evaluation path: one sum-all-reduce per evaluation.
"""
import torch

NCLASS = {"pascal": 20, "coco": 80, "fss": 1000, "paco_part": 448, "pascal_part": 100, "lvis": 1203}


def fold_class_ids(benchmark, fold, nfolds=None, split="val", cat_ids=None):
    """Classes a dataset split evaluates / trains on (`dataset.class_ids`, logger.py:15), per benchmark:
      coco   (evaluation_util/data/coco.py:64-70)    interleaved: val = fold + nfolds*v, v < nclass/nfolds
      pascal (evaluation_util/data/pascal.py:115-123) contiguous:  val = fold*n + i,     i < nclass/nfolds
      fss    (evaluation_util/data/fss.py:100-107)    fixed ranges per split, no folds: trn 0..519,
             val 520..759, test 760..999
      lvis   (evaluation_util/data/lvis.py:66-90)     10 folds, interleaved over the annotation file's
             category list -- pass that list as `cat_ids` (it comes from lvis_val.pkl / lvis_train.pkl,
             not from arithmetic); the meter is then indexed by position (lvis.py:28-29).
    Other benchmarks (paco_part, pascal_part) keep their class lists in dataset pickles: not derivable."""
    nclass = NCLASS[benchmark]
    if benchmark == "coco":
        nf = nfolds or 4
        val = [fold + nf * v for v in range(nclass // nf)]
        return val if split != "trn" else [c for c in range(nclass) if c not in val]
    if benchmark == "pascal":
        nf = nfolds or 4
        n = nclass // nf
        val = [fold * n + i for i in range(n)]
        return val if split != "trn" else [c for c in range(nclass) if c not in val]
    if benchmark == "fss":
        return {"trn": list(range(0, 520)), "val": list(range(520, 760)), "test": list(range(760, 1000))}[split]
    if benchmark == "lvis":
        if cat_ids is None:
            raise ValueError("lvis class ids come from the annotation pickles (lvis.py:66-90): pass cat_ids")
        nf = nfolds or 10
        cats = list(cat_ids)
        if split == "trn":
            raise NotImplementedError("lvis training split: class list = train categories minus the fold's "
                                      "validation categories (lvis.py:84), both from the annotation pickles")
        picked = [cats[fold + nf * v] for v in range(len(cats) // nf)]
        return sorted(range(len(picked)))
    raise NotImplementedError(f"class ids of benchmark {benchmark!r} live in its dataset files "
                              "(evaluation_util/data/%s.py); pass them to AverageMeter directly" % benchmark)


def classify_prediction(pred_mask, gt_mask, query_ignore_idx=None, ignore_index=255):
    """pred/gt [B, H, W] with values {0, 1}; -> (area_inter [2, B], area_union [2, B]) int64.
    Integer restatement of evaluation.py:12-39 (torch.histc with 2 bins over [0, 1] drops 255)."""
    pred = pred_mask.long()
    gt = gt_mask.long()
    if query_ignore_idx is not None:
        ign = query_ignore_idx.bool()
        gt = torch.where(ign, torch.full_like(gt, ignore_index), gt)
        pred = torch.where(ign, torch.full_like(pred, ignore_index), pred)
    out_i, out_u = [], []
    for p, g in zip(pred, gt):
        inter = torch.stack([((p == c) & (g == c)).sum() for c in (0, 1)])
        pa = torch.stack([(p == c).sum() for c in (0, 1)])
        ga = torch.stack([(g == c).sum() for c in (0, 1)])
        out_i.append(inter)
        out_u.append(pa + ga - inter)
    return torch.stack(out_i).t().contiguous(), torch.stack(out_u).t().contiguous()


class AverageMeter:
    def __init__(self, benchmark, class_ids, device="cpu"):
        self.benchmark = benchmark
        self.nclass = NCLASS[benchmark]
        self.class_ids_interest = torch.tensor(list(class_ids), dtype=torch.long, device=device)
        self.intersection_buf = torch.zeros(2, self.nclass, dtype=torch.int64, device=device)
        self.union_buf = torch.zeros(2, self.nclass, dtype=torch.int64, device=device)

    def update(self, inter_b, union_b, class_id):
        """inter_b / union_b [2, B] counts, class_id [B] (logger.py:35-37)."""
        cid = class_id.to(self.intersection_buf.device, torch.long)
        self.intersection_buf.index_add_(1, cid, inter_b.to(self.intersection_buf.device, torch.int64))
        self.union_buf.index_add_(1, cid, union_b.to(self.union_buf.device, torch.int64))

    def update_from_counts(self, counts, class_id):
        """counts [B, 4] int64 = inter0, inter1, union0, union1 from dfw_seg_postprocess.  On the GPU this
        is one library kernel (dfw_meter_update: int64 atomics, exact in any order); CPU buffers (the gloo
        rehearsal, host-side checks) take the index_add_ form of logger.py:35-37."""
        if self.intersection_buf.is_cuda:
            from . import ops
            cid = class_id.to(self.intersection_buf.device, torch.int64).contiguous()
            ops.meter_update(counts.contiguous(), cid, self.intersection_buf, self.union_buf)
            return
        self.update(counts[:, 0:2].t(), counts[:, 2:4].t(), class_id)

    def all_reduce(self, group=None):
        """Sum the two buffers over all ranks (RCCL over xGMI when the buffers are on the GPU,
        gloo on CPU).  int64 sums are exact and order-independent."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            both = torch.stack([self.intersection_buf, self.union_buf])
            dist.all_reduce(both, op=dist.ReduceOp.SUM, group=group)
            self.intersection_buf, self.union_buf = both[0].clone(), both[1].clone()

    def compute_iou(self):
        """logger.py:42-51 on fp32 copies of the (exact) buffers."""
        inter, union = self.intersection_buf.float(), self.union_buf.float()
        iou = inter / torch.max(torch.stack([union, torch.ones_like(union)]), dim=0)[0]
        iou = iou.index_select(1, self.class_ids_interest)
        miou = iou[1].mean() * 100
        fb_iou = (inter.index_select(1, self.class_ids_interest).sum(dim=1)
                  / union.index_select(1, self.class_ids_interest).sum(dim=1)).mean() * 100
        return miou, fb_iou, iou[1][:min(len(iou[1]), 20)]


def nway_iou(counts):
    """counts int64 [B, 2, N+1] (ops.seg_labels / segment_classes: per image and label, row 0 intersections, row 1 unions;
    label 0 = background) or their running sum [2, N+1] -> (iou [N+1] float64, miou): the counts are summed over the
    images (exact, int64), iou_l = 100 * inter_l / union_l (0 where the union is empty), and miou is the mean over the
    class labels 1..N whose union is non-zero (a class neither predicted nor present anywhere says nothing; 0.0 when
    there is none).  Percent, like AverageMeter.compute_iou."""
    c = counts.to(torch.int64)
    if c.dim() == 3:
        c = c.sum(0)
    if c.dim() != 2 or c.shape[0] != 2 or c.shape[1] < 2:
        raise ValueError(f"counts must be [B, 2, N+1] or [2, N+1] with N >= 1, got {tuple(counts.shape)}")
    inter, union = c[0].double(), c[1].double()
    seen = union > 0
    iou = torch.where(seen, 100.0 * inter / union.clamp(min=1.0), torch.zeros_like(union))
    fg = seen[1:]
    miou = float(iou[1:][fg].mean()) if bool(fg.any()) else 0.0
    return iou, miou


def boundary_width(h, w, ratio=0.02):
    """The band width of Boundary IoU (Cheng et al., CVPR 2021) for an h x w image: max(1, int(round(ratio * diagonal))),
    2 % of the diagonal by default -- 14 at 512 x 512, 116 at 4096 x 4096."""
    import math
    return max(1, int(round(float(ratio) * math.sqrt(int(h) * int(h) + int(w) * int(w)))))


def boundary_iou(counts):
    """Boundary IoU per class and its mean: nway_iou of objects.boundary_counts' counts int64 [B, 2, N+1] (a list of such
    tables from ragged sizes is summed first) -> (iou [N+1] float64, miou), percent.  Bin 0, the pixels in neither band, is
    not part of the mean."""
    if isinstance(counts, (list, tuple)):
        counts = torch.stack([c.reshape(-1, *c.shape[-2:]).sum(0) for c in counts])
    return nway_iou(counts)


def panoptic_quality(pq):
    """pq int64 [B, N+1, 4] (ops.seg_match / objects.match_objects: per image and class (TP, FP, FN, S), S the sum over the
    matched pairs of floor(IoU * 2^32); class 0 unused), a list of such tables, or their running sum [N+1, 4] -> dict(pq,
    sq, rq: float64 [N+1] per class; mean_pq, mean_sq, mean_rq: floats).  The counts are summed over the images (exact,
    int64), then per class SQ = S / 2^32 / TP (the mean IoU of the matched pairs, 0 without one), RQ = TP / (TP + FP / 2 +
    FN / 2), PQ = SQ * RQ; the means run over the classes 1..N with TP + FP + FN > 0 (a class neither predicted nor present
    says nothing; 0.0 when there is none).  Fractions in 0..1, not percent: PQ's usual scale."""
    if isinstance(pq, (list, tuple)):
        pq = torch.stack([p.reshape(-1, *p.shape[-2:]).sum(0) for p in pq])
    c = pq.to(torch.int64)
    if c.dim() == 3:
        c = c.sum(0)
    if c.dim() != 2 or c.shape[0] < 2 or c.shape[1] != 4:
        raise ValueError(f"pq must be [B, N+1, 4] or [N+1, 4] with N >= 1, got {tuple(pq.shape)}")
    tp, fp, fn, s = (c[:, i].double() for i in range(4))
    seen = (tp + fp + fn) > 0
    seen[0] = False
    sq = torch.where(tp > 0, s / 4294967296.0 / tp.clamp(min=1.0), torch.zeros_like(s))
    rq = torch.where(seen, tp / (tp + 0.5 * fp + 0.5 * fn).clamp(min=0.5), torch.zeros_like(s))
    q = sq * rq
    mean = lambda v: float(v[seen].mean()) if bool(seen.any()) else 0.0  # noqa: E731
    return dict(pq=q, sq=sq, rq=rq, mean_pq=mean(q), mean_sq=mean(sq), mean_rq=mean(rq))


_COCO_THRESHOLDS = tuple((n, 20) for n in range(10, 20))      # IoU 0.50, 0.55, .., 0.95


def _detection_rows(dets):
    """An array [k, 5], or lists of them nested in any depth, -> one int64 array in order."""
    import numpy as np
    if isinstance(dets, (list, tuple)):
        parts = [_detection_rows(d) for d in dets]
        return np.concatenate(parts) if parts else np.zeros((0, 5), np.int64)
    return np.asarray(dets, dtype=np.int64).reshape(-1, 5)


def average_precision(dets, npos, thresholds=_COCO_THRESHOLDS):
    """Average precision per class over a whole dataset.  dets: objects.detections_to_host's rows (class, sum, n, inter,
    union) -- an int64 array [k, 5], or lists of them (over images, over calls, nested), concatenated in order; npos int64
    [nlabels + 1], the ground-truth objects per class (the sum of detections_to_host's npos over the dataset; class 0
    unused).  thresholds: IoU thresholds as integer pairs (num, den), COCO's 0.50:0.05:0.95 by default; each needs
    2 * num >= den (the match table holds one partner, found above 1/2), ValueError otherwise.

    Per class with npos > 0 and per threshold: the class' detections are sorted by their score sum / n (the float64
    quotient of two exact integers; sum / (765 n) ranks the same) descending and stably, so ties keep image and then
    object order; a detection is a TP when it has a partner and inter * den > num * union in integers -- STRICTLY above,
    the matching rule of objects.match_objects, where COCO counts IoU >= threshold; precision TP / rank is made
    non-increasing from the right; it is sampled at the recalls k / 100, k = 0..100, at the first rank whose recall reaches
    the sample (searchsorted, side="left"), 0 beyond the last recall; AP is the mean of the 101 samples (their exactly
    rounded sum over 101).  A class without a detection has AP 0.  No area ranges and no maxDets.

    Returns dict(ap float64 [nlabels + 1, T], NaN for classes without positives; map = the nanmean over all of it, as the exactly
    rounded sum over the count (NaN when no class has a positive); ap50 = the column of (10, 20), or None without that threshold; thresholds)."""
    import math
    import numpy as np
    thresholds = tuple((int(a), int(b)) for a, b in thresholds)
    for num, den in thresholds:
        if num < 1 or den < num or 2 * num < den:
            raise ValueError(f"average_precision: the threshold {num}/{den} is not in [1/2, 1]")
    rows = _detection_rows(dets)
    npos = np.asarray(npos, dtype=np.int64).reshape(-1)
    ap = np.full((npos.shape[0], len(thresholds)), np.nan)
    samples = np.arange(101) / 100.0
    for c in range(1, npos.shape[0]):
        if npos[c] <= 0:
            continue
        d = rows[rows[:, 0] == c]
        score = d[:, 1].astype(np.float64) / d[:, 2].astype(np.float64)
        d = d[np.argsort(-score, kind="stable")]
        rank = np.arange(1, d.shape[0] + 1, dtype=np.float64)
        for t, (num, den) in enumerate(thresholds):
            tp = np.cumsum((d[:, 4] > 0) & (d[:, 3] * den > num * d[:, 4])).astype(np.float64)
            recall, prec = tp / float(npos[c]), tp / rank
            prec = np.maximum.accumulate(prec[::-1])[::-1]
            at = np.searchsorted(recall, samples, side="left")
            q = np.where(at < d.shape[0], prec[np.minimum(at, max(d.shape[0] - 1, 0))], 0.0) if d.shape[0] else np.zeros(101)
            ap[c, t] = math.fsum(q.tolist()) / 101.0
    vals = ap[~np.isnan(ap)].tolist()
    ap50 = ap[:, thresholds.index((10, 20))] if (10, 20) in thresholds else None
    return dict(ap=ap, map=math.fsum(vals) / len(vals) if vals else float("nan"), ap50=ap50, thresholds=thresholds)
