"""Episode-sharded evaluation loop: counterpart of `test_diffusion`
(/root/reference/evaluation_util/main_oss.py:84-171) for one process per GPU.

The reference evaluates on one GPU (E:308) with the threshold and the metric on the host
(E:128-137); here rank r runs episodes i == r (mod R), thresholding + inter/union counts stay on the
device, and the ranks meet once, in a sum all-reduce of the two `[2, nclass]` buffers
(evaluation_util/common/logger.py:30-31).  No data-path collective.
"""
import torch

from . import episodes as ep
from .metrics import AverageMeter, fold_class_ids


def episode_batches(indices, batch):
    for i in range(0, len(indices), batch):
        yield indices[i:i + batch]


@torch.no_grad()
def test_diffusion(pipe, n_episodes, nshot=1, res=512, batch=1, benchmark="coco", fold=0, r_threshold=0.25,
                   rank=0, world_size=1, make_batch=None, device=None, episodes=None, threshold=0.0,
                   batch_max=False, captured=True, use_original_imgsize=False, ignore_value=-1):
    """Run `n_episodes` episodes sharded over `world_size` ranks; returns (miou, fb_iou, meter).
    Sources, first match wins:
      episodes   -- indexable of HOST episodes (decoded PIL images / uint8 arrays + class-id masks, the
                    material of DatasetCOCO.load_frame, coco.py:77-107): this rank's share goes through the
                    GPU input pipeline (input_pipeline.EpisodeLoader: resize / normalise / mask kernels on a
                    side stream, prefetched);
      make_batch -- make_batch(indices) returns device tensors (dict of episodes.make_episode_batch + 'class_id');
      otherwise  -- synthetic episodes (episodes.make_episode_batch).
    captured: every step is one replay of the pipeline-owned HIP graph (pipeline.run_episodes(captured=True));
    the per-step results are consumed (meter update on the same stream) before the next replay overwrites them.
    r_threshold / threshold / batch_max: the launcher's thresholding flags (main_oss.py:128-135).
    use_original_imgsize (the launcher's flag of that name, main_oss.py:188): score every query at its own size -- the
    prediction resized back as the reference's pipeline does, thresholded on the resized image and counted against the
    query's class-id map at native size, pixels equal to `ignore_value` dropped (-1: none; 255: PASCAL's boundary) -- all
    on the device (ops.seg_native); the meter is fed from r["native"]["counts"].  Host episodes only: the other two
    sources have no native size, make_batch may return its own `native` (input_pipeline.NativeTargets)."""
    device = device or pipe.device
    meter = AverageMeter(benchmark, fold_class_ids(benchmark, fold), device=device)
    mine = ep.shard(n_episodes, rank, world_size)
    if episodes is not None:
        from .input_pipeline import EpisodeLoader
        loader = EpisodeLoader((episodes[i] for i in mine), res, batch, nshot, device=device,
                               native=use_original_imgsize, ignore_value=ignore_value)
        for bt in loader:
            r = pipe.run_episodes(bt["support_imgs"], bt["query_img"], bt["support_masks"], bt["query_mask"],
                                  r_threshold=r_threshold, threshold=threshold, batch_max=batch_max, captured=captured,
                                  native=bt.get("native"))
            counts = r["native"]["counts"] if use_original_imgsize else r["counts"]
            meter.update_from_counts(counts, bt["class_id"].to(device))
        meter.all_reduce()
        miou, fb_iou, _ = meter.compute_iou()
        return float(miou), float(fb_iou), meter
    for idx in episode_batches(mine, batch):
        if make_batch is not None:
            bt = make_batch(idx)
            cls = bt["class_id"]
        else:
            bt = ep.make_episode_batch(len(idx), nshot, res, seed=1000 + idx[0], device=device)
            cls = ep.episode_class_ids(idx, benchmark, fold)
        native = bt.get("native") if use_original_imgsize else None
        if use_original_imgsize and native is None:
            raise ValueError("use_original_imgsize needs native sizes: pass host `episodes`, or a make_batch whose "
                             "batches carry `native` (input_pipeline.NativeTargets)")
        r = pipe.run_episodes(bt["support_imgs"], bt["query_img"], bt["support_masks"], bt["query_mask"],
                              r_threshold=r_threshold, threshold=threshold, batch_max=batch_max, captured=captured,
                              native=native)
        meter.update_from_counts(r["native"]["counts"] if native is not None else r["counts"], cls.to(device))
    meter.all_reduce()
    miou, fb_iou, _ = meter.compute_iou()
    return float(miou), float(fb_iou), meter


@torch.no_grad()
def evaluate_support_set(pipe, support_imgs, support_masks, query_batches, class_id, benchmark="coco", fold=0, r_threshold=0.25,
                     threshold=0.0, batch_max=False, captured=True, device=None, use_original_imgsize=False, ignore_value=-1):
    """One fixed support set against a stream of queries: the bank is prepared ONCE (pipe.prepare_support), then every
    item of `query_batches` -- (query_img [b, 3, H, W], query_mask uint8 [b, H, W]) device tensors, b may vary -- goes
    through pipe.segment_queries and its counts into the AverageMeter under `class_id` (the support set's class).
    Returns (miou, fb_iou, meter) like test_diffusion; single process, no sharding (shard `query_batches` outside).
    use_original_imgsize: every item is (query_img, query_mask, native_gt) with native_gt the b queries' HOST class-id
    maps (or 0/1/255 masks with class_value 1) at their own sizes; they are staged (input_pipeline.NativeTargets with
    foreground value class_id + 1 and `ignore_value`) and the meter is fed from r["native"]["counts"]."""
    device = device or pipe.device
    meter = AverageMeter(benchmark, fold_class_ids(benchmark, fold), device=device)
    bank = pipe.prepare_support(support_imgs, support_masks)
    for item in query_batches:
        query_img, query_mask = item[0], item[1]
        native = None
        if use_original_imgsize:
            from .input_pipeline import NativeTargets
            native = NativeTargets(query_img.shape[-2:], [g.shape for g in item[2]], gt=item[2],
                                   class_value=int(class_id) + 1, ignore_value=ignore_value, device=device)
        r = pipe.segment_queries(bank, query_img, query_mask, r_threshold=r_threshold, threshold=threshold,
                                 batch_max=batch_max, captured=captured, native=native)
        cls = torch.full((query_img.shape[0],), int(class_id), dtype=torch.int64, device=device)
        meter.update_from_counts(r["native"]["counts"] if native is not None else r["counts"], cls)
    meter.all_reduce()
    miou, fb_iou, _ = meter.compute_iou()
    return float(miou), float(fb_iou), meter


@torch.no_grad()
def evaluate_class_set(pipe, support_imgs, support_masks, query_batches, r_threshold=0.25, threshold=0.0, batch_max=False,
                       max_batch=16, captured=True, use_original_imgsize=False, class_ids=None):
    """N fixed classes against a stream of queries: the N support sets (support_imgs / support_masks [N, s, 3, H, W], or
    two lists of N tensors [s_c, 3, H, W] for classes with different numbers of examples) are
    prepared ONCE (pipe.prepare_support_classes), then every item of `query_batches` -- (query_img [b, 3, H, W],
    query_labels uint8 [b, H, W] with 0 = background, 1 + c = class c, 255 = ignore) device tensors, b may vary -- goes
    through pipe.segment_classes and its per-label counts into one int64 [2, N+1] running sum on the device.
    Returns (miou, iou [N+1], counts [2, N+1]) as metrics.nway_iou defines them; single process, no sharding.
    use_original_imgsize: every item is (query_img, input_pipeline.NativeTargets) -- the b queries' own sizes and their
    ground truth at those sizes, label maps or, with class_ids (the ground-truth id of each class), class-id maps -- and the
    running sum is fed from r["native"]["counts"] (ops.seg_labels_native): labels scored at every image's own h x w."""
    from .metrics import nway_iou
    bankset = pipe.prepare_support_classes(support_imgs, support_masks)
    total = torch.zeros(2, bankset.nsets + 1, dtype=torch.int64, device=pipe.device)
    for query_img, target in query_batches:
        if use_original_imgsize:
            r = pipe.segment_classes(bankset, query_img, None, r_threshold=r_threshold, threshold=threshold,
                                     batch_max=batch_max, max_batch=max_batch, captured=captured, native=target,
                                     class_ids=class_ids)
            if r["native"]["counts"] is None:
                raise ValueError("use_original_imgsize needs NativeTargets that carry a ground truth")
            total += r["native"]["counts"].sum(0)
            continue
        r = pipe.segment_classes(bankset, query_img, target, r_threshold=r_threshold, threshold=threshold,
                                 batch_max=batch_max, max_batch=max_batch, captured=captured)
        total += r["counts"].sum(0)
    iou, miou = nway_iou(total)
    return miou, iou, total


@torch.no_grad()
def evaluate_stream(pipe, support_images, support_class_maps, class_id=None, queries=(), class_ids=None, size=512, batch=4,
                    depth=2, benchmark="coco", fold=0, r_threshold=0.25, threshold=0.0, batch_max=False, max_batch=16,
                    captured=True, ignore_value=-1):
    """Decoded images in, scores out: annotated examples and a stream of queries, both as the dataset hands them over
    (PIL / uint8 [H, W, 3] images of any sizes, [H, W] class-id maps), scored at every query's own size.

    Binary (class_id, the benchmark's class index; the maps hold class_id + 1 as coco.py:74-75 stores it):
      support_images / support_class_maps hold the s examples; returns (miou, fb_iou, meter) as evaluate_support_set does
      under use_original_imgsize.
    N-way (class_ids, the ground-truth id of each of the N classes): support_images / support_class_maps are N lists of
      examples (the classes may differ in how many), class c's maps hold class_ids[c]; returns (miou, iou [N+1], counts [2, N+1]) as evaluate_class_set does
      under use_original_imgsize with class_ids.
    The supports become tensors through input_pipeline.support_tensors (one copy, three launches) and are prepared ONCE;
    `queries` yields dicts with `query_img` and `gt` and runs through pipe.segment_stream (`size`: processing size; `batch`, `depth`); the meter (binary) or the int64 [2, N+1] running sum
    (N-way) is fed from r["native"]["counts"].  Single process, no sharding (shard `queries` outside)."""
    from .input_pipeline import support_tensors
    if (class_id is None) == (class_ids is None):
        raise ValueError("give class_id (one support set, binary scores) or class_ids (N support sets, N-way scores)")
    device = pipe.device
    stream = dict(batch=batch, size=size, depth=depth, ignore_value=ignore_value, r_threshold=r_threshold,
                  threshold=threshold, batch_max=batch_max, captured=captured)
    if class_ids is None:
        meter = AverageMeter(benchmark, fold_class_ids(benchmark, fold), device=device)
        sup, msk = support_tensors(support_images, support_class_maps, int(class_id) + 1, size, device)
        bank = pipe.prepare_support(sup, msk)
        for index, r in pipe.segment_stream(bank, queries, class_value=int(class_id) + 1, **stream):
            if r["native"]["counts"] is None:
                raise ValueError("evaluate_stream needs queries that carry `gt`")
            cls = torch.full((len(index),), int(class_id), dtype=torch.int64, device=device)
            meter.update_from_counts(r["native"]["counts"], cls)
        meter.all_reduce()
        miou, fb_iou, _ = meter.compute_iou()
        return float(miou), float(fb_iou), meter
    from .metrics import nway_iou
    ids = [int(c) for c in class_ids]
    sets = [list(x) for x in support_images]
    maps = [list(x) for x in support_class_maps]
    N = len(ids)
    if len(sets) != N or len(maps) != N or any(len(x) < 1 for x in sets) or any(len(x) != len(m) for x, m in zip(sets, maps)):
        raise ValueError("N-way: support_images / support_class_maps must be N lists of at least one example, each class "
                         "with as many maps as images")
    shots = [len(x) for x in sets]
    sup, msk = support_tensors([im for x in sets for im in x], [m for x in maps for m in x],
                               [c for c, s in zip(ids, shots) for _ in range(s)], size, device)
    if len(set(shots)) == 1:      # equal counts: the uniform stack
        bankset = pipe.prepare_support_classes(sup.view(N, shots[0], *sup.shape[1:]), msk.view(N, shots[0], *msk.shape[1:]))
    else:
        bankset = pipe.prepare_support_classes(list(sup.split(shots)), list(msk.split(shots)))
    total = torch.zeros(2, N + 1, dtype=torch.int64, device=device)
    for index, r in pipe.segment_stream(bankset, queries, class_ids=ids, max_batch=max_batch, **stream):
        if r["native"]["counts"] is None:
            raise ValueError("evaluate_stream needs queries that carry `gt`")
        total += r["native"]["counts"].sum(0)
    iou, miou = nway_iou(total)
    return miou, iou, total


@torch.no_grad()
def evaluate_routed(pipe, bankset, queries, class_of_set, gt_ids=None, benchmark="coco", fold=0, route="route", batch=4,
                    size=None, depth=2, r_threshold=0.25, threshold=0.0, batch_max=False, captured=True, ignore_value=-1):
    """The reference's class-wise protocol over a FIXED library of classes: `bankset` holds the prepared support sets
    (pipe.prepare_support_classes, uniform or ragged), `queries` yields dicts with `query_img`, `gt` (a class-id map at
    the image's own size) and the index of the one set the query is scored against (`route`: a key name or a callable on
    the dict) -- evaluation_util/main_oss.py's episodes, whose class changes from one to the next, without preparing a
    support set twice.  Every batch runs through pipe.segment_stream(route=...) / segment_routed, and its native-size
    binary counts go into the AverageMeter under class_of_set[route_i] (the benchmark's class index of set route_i).
    gt_ids[c]: the id class c's pixels carry in `gt`; default class_of_set[c] + 1, as coco.py:74-75 stores them.
    Returns (miou, fb_iou, meter) like evaluate_support_set; single process, no sharding."""
    device = pipe.device
    cls_of = [int(c) for c in class_of_set]
    if len(cls_of) != bankset.nsets:
        raise ValueError(f"class_of_set names {len(cls_of)} classes, the support bank set holds {bankset.nsets}")
    ids = [c + 1 for c in cls_of] if gt_ids is None else [int(c) for c in gt_ids]
    if len(ids) != bankset.nsets:
        raise ValueError(f"{len(ids)} gt_ids for a support bank set of {bankset.nsets}")
    meter = AverageMeter(benchmark, fold_class_ids(benchmark, fold), device=device)
    for index, r in pipe.segment_stream(bankset, queries, batch=batch, size=size, depth=depth, class_ids=ids,
                                        ignore_value=ignore_value, r_threshold=r_threshold, threshold=threshold,
                                        batch_max=batch_max, captured=captured, route=route):
        if r["native"]["counts"] is None:
            raise ValueError("evaluate_routed needs queries that carry `gt`")
        cls = torch.tensor([cls_of[c] for c in r["route"]], dtype=torch.int64, device=device)
        meter.update_from_counts(r["native"]["counts"], cls)
    meter.all_reduce()
    miou, fb_iou, _ = meter.compute_iou()
    return float(miou), float(fb_iou), meter


@torch.no_grad()
def evaluate_candidates(pipe, library, items, r_threshold=0.25, threshold=0.0, entry_batch=8, labels="set", captured=True,
                        use_original_imgsize=False, class_ids=None):
    """A library of classes against queries that each name their own candidate classes: `library` is a prepared
    SupportBankSet (pipe.prepare_support_classes, uniform or ragged), every item of `items` is (query_img [b, 3, H, W],
    candidates: b lists of set indices, label_map uint8 [b, H, W] in the labels pipe.segment_candidates writes -- 0 =
    background, 255 = ignore), b may vary.  Every item goes through pipe.segment_candidates and its per-label counts into
    one int64 running sum on the device; a ground-truth label outside a query's candidates is a miss in that label's
    union.  Returns (miou, iou [L+1], counts [2, L+1]) as evaluate_class_set does (metrics.nway_iou), L = the library's
    number of sets with labels="set", the longest candidate list seen with labels="local".
    use_original_imgsize: every item is (query_img, candidates, input_pipeline.NativeTargets) -- the b queries' own sizes
    and their ground truth at those sizes, label maps or, with class_ids (the ground-truth id of each set), class-id maps
    -- and the running sum is fed from r["native"]["counts"] (ops.seg_labels_cand_native): labels scored at every image's
    own h x w.  Single process, no sharding."""
    from .metrics import nway_iou
    total = torch.zeros(2, 255, dtype=torch.int64, device=pipe.device)
    width = library.nsets + 1 if labels == "set" else 0
    if class_ids is not None and not use_original_imgsize:
        raise ValueError("class_ids maps a native-size ground truth: give use_original_imgsize=True with it")
    for query_img, candidates, label_map in items:
        if use_original_imgsize:
            r = pipe.segment_candidates_native(library, query_img, candidates, label_map, class_ids, r_threshold=r_threshold,
                                               threshold=threshold, entry_batch=entry_batch, labels=labels, captured=captured)
            counts = r["native"]["counts"]
            if counts is None:
                raise ValueError("use_original_imgsize needs NativeTargets that carry a ground truth")
        else:
            r = pipe.segment_candidates(library, query_img, candidates, label_map, r_threshold=r_threshold,
                                        threshold=threshold, entry_batch=entry_batch, labels=labels, captured=captured)
            counts = r["counts"]
        n = counts.shape[2]
        total[:, :n] += counts.sum(0)
        width = max(width, n)
    total = total[:, :width].contiguous()
    iou, miou = nway_iou(total)
    return miou, iou, total


@torch.no_grad()
def evaluate_tiled(pipe, support, items, class_id=0, benchmark="coco", fold=0, overlap=None, ramp=None, batch=4,
                   r_threshold=0.25, threshold=0.0, max_batch=16, captured=True, entry_batch=8):
    """Images larger than the processing size against one prepared support, each segmented at its own resolution by
    pipe.segment_tiled (`overlap`, `ramp`, `batch`, `max_batch`, the thresholding flags and `captured` are its arguments).
    `items` yields (image, gt): PIL / uint8 [h, w, 3] of any size not below the tile, and a uint8 [h, w] label map (0 =
    background, 1 + c = class c, 255 = ignored; 0 / 1 / 255 for a bank).  An item may be (image, gt, candidates): that
    item goes through segment_tiled's candidate route (a SupportBankSet only) with `entry_batch`; the returns are unchanged.

    support a SupportBank: the counts go into the AverageMeter under `class_id` (the support set's class index); returns
    (miou, fb_iou, meter) as evaluate_stream does for one support set.  A SupportBankSet: the counts are summed into one
    int64 [2, N+1]; returns (miou, iou [N+1], counts) as evaluate_stream does N-way.  Single process, no sharding."""
    from .unet import SupportBankSet
    device = pipe.device
    flags = dict(overlap=overlap, ramp=ramp, batch=batch, r_threshold=r_threshold, threshold=threshold, max_batch=max_batch,
                 captured=captured)
    if not isinstance(support, SupportBankSet):
        meter = AverageMeter(benchmark, fold_class_ids(benchmark, fold), device=device)
        cls = torch.full((1,), int(class_id), dtype=torch.int64, device=device)
        for item in items:
            image, gt = item[0], item[1]
            if gt is None:
                raise ValueError("evaluate_tiled needs items that carry a ground truth")
            if len(item) > 2:
                raise ValueError("candidates name sets of a SupportBankSet; a SupportBank has only one")
            meter.update_from_counts(pipe.segment_tiled(support, image, gt, **flags)["counts"].view(1, 4), cls)
        meter.all_reduce()
        miou, fb_iou, _ = meter.compute_iou()
        return float(miou), float(fb_iou), meter
    from .metrics import nway_iou
    total = torch.zeros(2, support.nsets + 1, dtype=torch.int64, device=device)
    for item in items:
        image, gt = item[0], item[1]
        if gt is None:
            raise ValueError("evaluate_tiled needs items that carry a ground truth")
        cand = dict(candidates=item[2], entry_batch=entry_batch) if len(item) > 2 else {}
        total += pipe.segment_tiled(support, image, gt, **flags, **cand)["counts"]
    iou, miou = nway_iou(total)
    return miou, iou, total
