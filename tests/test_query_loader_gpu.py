"""GPU tests of the query stream's input half: the batched input transform (dfw_inputs_to_tensor through
DeviceImageTransform.batch) against Pillow / torch themselves and against the per-item image() / mask() calls, with 0xA5
guards around every item; its fixed launch count; the prefetching QueryLoader with a consumer that never synchronises;
pipeline.segment_stream and evaluate.evaluate_stream against the hand-written per-image loop.  Bytes and integers: every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import query_loader_ref as qr

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
RES = 64


def _fill(n):
    return torch.full((max(n, 1),), 0xA5, dtype=torch.uint8, device="cuda")


def _untouched(buf, regions):
    """True when every byte of `buf` outside the (offset, bytes) regions still holds 0xA5."""
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    for o, n in regions:
        keep[o:o + n] = False
    return bool((buf.cpu()[keep] == 0xA5).all())


@pytest.mark.parametrize("out_hw", qr.OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_equals_pillow_torch_and_per_item_calls(hip_lib, out_hw):
    """One call for seven images and seven class-id maps of assorted sizes == Image.resize(BILINEAR) + ToTensor + Normalize,
    F.interpolate(nearest), and tf.image() / tf.mask() item by item; tmp, dst, pm1 and bin are pre-filled with 0xA5 and
    laid out with 64 guard bytes after every item: no byte outside an item's own region changes.  Then the images-only and
    the masks-only call."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    d = qr.ragged(out_hw)
    oh, ow = out_hw
    tf = DeviceImageTransform(out_hw)
    plan = DeviceImageTransform(out_hw, device=None).batch(d["images"], d["masks"], d["mask_class"], d["want_pm1"],
                                                           d["want_bin"], guard=64)
    bufs = dict(tmp=_fill(plan.tmp_bytes), dst=_fill(plan.dst_bytes), pm1=_fill(plan.pm1_bytes), bin=_fill(plan.bin_bytes))
    r = tf.batch(d["images"], d["masks"], d["mask_class"], d["want_pm1"], d["want_bin"], guard=64, buffers=bufs)
    lay = r["layout"]
    n = len(d["images"])
    assert r["images"].shape == (n, 3, oh, ow) and r["images"].dtype == torch.float32
    assert r["pm1"].shape == (sum(d["want_pm1"]), 3, oh, ow) and r["bin"].shape == (sum(d["want_bin"]), oh, ow)
    assert r["bin"].dtype == torch.uint8 and r["images"].data_ptr() == bufs["dst"].data_ptr()
    got_img, got_pm1, got_bin = r["images"].cpu(), r["pm1"].cpu(), r["bin"].cpu()
    k1 = k2 = 0
    for i in range(n):
        assert torch.equal(got_img[i], d["ref_images"][i]), (i, d["images"][i].shape)
        assert torch.equal(got_img[i], tf.image(d["images"][i]).cpu()), i
        ref = d["ref_masks"][i]
        pm1_i, bin_i = tf.mask(d["masks"][i], d["mask_class"][i] - 1)
        assert torch.equal(bin_i.cpu().float(), ref), i
        if d["want_pm1"][i]:
            assert torch.equal(got_pm1[k1], ref[None].repeat(3, 1, 1) * 2 - 1), i
            assert torch.equal(got_pm1[k1], pm1_i.cpu()), i
            k1 += 1
        if d["want_bin"][i]:
            assert torch.equal(got_bin[k2].float(), ref), i
            assert torch.equal(got_bin[k2], bin_i.cpu()), i
            k2 += 1
    # guards: every item is followed by >= 64 untouched bytes, and nothing else outside the items' regions changed
    items, mitems = lay.img_items[:lay.n_img], lay.mask_items[:lay.n_mask]
    regions = dict(tmp=[(it.tmp_off, 3 * it.H * ow) for it in items], dst=[(it.dst_off, 12 * oh * ow) for it in items],
                   pm1=[(it.pm1_off, 12 * oh * ow) for it in mitems if it.pm1_off != -1],
                   bin=[(it.bin_off, oh * ow) for it in mitems if it.bin_off != -1])
    for name, regs in regions.items():
        ends = [o for o, _ in regs][1:] + [bufs[name].numel()]
        assert all(e - (o + m) >= 64 for (o, m), e in zip(regs, ends)), name
        assert _untouched(bufs[name], regs), name
        o, m = regs[0]
        assert not bool((bufs[name][o:o + m] == 0xA5).all()), name
    # images only / masks only
    ro = tf.batch(d["images"])
    assert ro["pm1"] is None and ro["bin"] is None and ro["images"].is_contiguous()
    assert torch.equal(ro["images"].cpu(), torch.stack(d["ref_images"]))
    rm = tf.batch([], d["masks"], d["mask_class"])
    assert rm["images"] is None and rm["pm1"].is_contiguous() and rm["bin"].is_contiguous()
    ref = torch.stack(d["ref_masks"])
    assert torch.equal(rm["bin"].cpu().float(), ref)
    assert torch.equal(rm["pm1"].cpu(), ref[:, None].repeat(1, 3, 1, 1) * 2 - 1)


def test_three_launches_whatever_the_batch(hip_lib):
    """Captured with 1 image + 1 map and with 7 + 7: three kernel nodes both times (horizontal, vertical + table, masks),
    images only: two; none of them a memset node; a replay equals the eager result."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    d = qr.ragged((48, 300))
    tf = DeviceImageTransform((48, 300))
    nodes = []
    for n_img, n_mask in ((1, 1), (7, 7), (7, 0)):
        # the one small item of the 1 + 1 case is the 37 x 41 one
        ims, mks, cls = d["images"][2:2 + n_img] if n_img == 1 else d["images"], d["masks"][:n_mask], d["mask_class"][:n_mask]
        eager = tf.batch(ims, mks, cls)                       # also stages the bytes and warms the allocator
        lay, staged = eager["layout"], eager["staged"]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = lay.run(staged, tf.lut, torch.cuda.current_stream().cuda_stream)
        n = C.c_int32(0)
        assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(n)) == 0
        nodes.append(n.value)
        graph.instantiate()
        graph.replay()
        torch.cuda.synchronize()
        for k in ("images", "pm1", "bin"):
            assert (out[k] is None) == (eager[k] is None), k
            if out[k] is not None:
                assert torch.equal(out[k], eager[k]), (n_img, n_mask, k)
    assert nodes == [3, 3, 2], nodes


# ------------------------------------------------------------------------------------------------ the tiny pipeline

def _kw(c):
    return {k: v for k, v in c.items() if not k.startswith("_")}


@pytest.fixture(scope="module", params=DTYPES, ids=["bf16", "f16"])
def models(request, hip_lib):
    """The tiny-config engine of tests/test_native_gpu.py (same seeds, weights rounded to the dtype)."""
    from diffews_amd import config, weights
    from diffews_amd.unet import MyUNet2DConditionModel
    from diffews_amd.vae import AutoencoderKL
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise
    from diffews_amd.scheduler import DDIMSchedulerCustomized
    dt = request.param
    ucfg, vcfg = config.get("tiny_unet"), config.get("tiny_vae")
    usd = weights.synthetic_unet_state_dict(ucfg, round_to=dt)
    vsd = weights.synthetic_vae_state_dict(vcfg, round_to=dt)
    te = weights.synthetic_text_embed(ucfg).to(dt).float()
    pipe = MarigoldPipelineRGBLatentNoise(MyUNet2DConditionModel(ucfg, usd, torch_dtype=dt),
                                          AutoencoderKL(vcfg, vsd, torch_dtype=dt),
                                          DDIMSchedulerCustomized(**_kw(config.get("scheduler"))), text_embeds=te)
    return dict(dt=dt, pipe=pipe)


CLASS_ID = 8                      # binary: a class of coco's fold 0 (fold + 4 v); the maps hold CLASS_ID + 1 = 9
CLASS_IDS = [9, 3, 7]             # N-way: the ground-truth id of each class
SIZES = [(48, 64), (80, 56), (64, 64), (23, 37), (97, 131)]


def _host_queries(n, seed, with_gt=True):
    """Decoded queries of assorted sizes; class-id maps (uint8 / int64 in turn) hold 0, the CLASS_IDS, 40 and 255."""
    assert CLASS_ID + 1 == CLASS_IDS[0]
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        h, w = SIZES[i % len(SIZES)]
        q = dict(query_img=rs.randint(0, 256, (h, w, 3)).astype(np.uint8))
        if with_gt:
            g = rs.choice([0, 9, 9, 3, 7, 40], size=(h, w)).astype(np.uint8 if i % 2 == 0 else np.int64)
            g[rs.rand(h, w) < 0.07] = 255
            q["gt"] = g
        out.append(q)
    return out


def _host_supports(ids, s, seed):
    """s annotated examples per id: images of 56 x 72 and 40 x 33, maps holding the id in a block plus speckle."""
    rs = np.random.RandomState(seed)
    images, maps = [], []
    for c in ids:
        ims, mps = [], []
        for k in range(s):
            h, w = [(56, 72), (40, 33)][k % 2]
            m = rs.choice([0, 0, 0, c, 40], size=(h, w)).astype(np.uint8)
            m[h // 4:3 * h // 4, w // 4:3 * w // 4] = c
            ims.append(rs.randint(0, 256, (h, w, 3)).astype(np.uint8))
            mps.append(m)
        images.append(ims)
        maps.append(mps)
    return images, maps


def _hand_supports(tf, images, maps, ids):
    """The per-image path: tf.image / tf.mask one call each -> ([N, s, 3, S, S], [N, s, 3, S, S])."""
    sup = torch.stack([torch.stack([tf.image(im) for im in ims]) for ims in images])
    msk = torch.stack([torch.stack([tf.mask(m, c - 1)[0] for m in mps]) for mps, c in zip(maps, ids)])
    return sup, msk


def _hand_batches(tf, qs, b, class_value=None):
    """The hand-written loop's inputs: per batch (query_img via tf.image per query, query_mask via tf.mask per query or
    None, host ground truth list, sizes)."""
    out = []
    for i in range(0, len(qs), b):
        part = qs[i:i + b]
        qry = torch.stack([tf.image(q["query_img"]) for q in part])
        qm = None
        if class_value is not None:
            qm = torch.stack([tf.mask(q["gt"], class_value - 1)[1] for q in part])
        out.append((qry, qm, [q["gt"] for q in part], [q["gt"].shape for q in part]))
    return out


@pytest.mark.parametrize("n,b", [(7, 3), (13, 2)])
def test_query_loader_batches_and_slot_recycling(models, n, b):
    """depth = 1: three slots.  7 queries in batches of 3 -> 3, 3, 1 with the right index; 13 in batches of 2 -> seven
    batches over three slots.  The consumer never synchronises: it queues GPU work, clones each batch's tensors on the
    stream and compares after the loop -- a slot overwritten early shows up as a mismatch.  query_img, query_mask, the
    S x S counts and the native counts equal the per-image path with host-staged NativeTargets."""
    from diffews_amd.input_pipeline import DeviceImageTransform, NativeTargets, QueryLoader
    pipe = models["pipe"]
    tf = DeviceImageTransform(RES)
    simg, smap = _host_supports([CLASS_ID + 1], 1, seed=3)
    sup, msk = _hand_supports(tf, simg, smap, [CLASS_ID + 1])
    bank = pipe.prepare_support(sup[0], msk[0])
    qs = _host_queries(n, seed=10 * n + b)
    slow = torch.randn(2048, 2048, device="cuda")
    got = []
    for bt in QueryLoader(qs, RES, b, depth=1, class_value=CLASS_ID + 1, ignore_value=255):
        for _ in range(4):                      # queued GPU work, no host sync: the producer runs ahead of the device
            slow = (slow @ slow).clamp_(-1, 1)
        r = pipe.segment_queries(bank, bt["query_img"], bt["query_mask"], captured=False, native=bt["native"])
        got.append(dict(index=bt["index"], query_img=bt["query_img"].clone(), query_mask=bt["query_mask"].clone(),
                        counts=r["counts"].clone(), native_counts=r["native"]["counts"].clone(),
                        sizes=list(bt["native"].sizes)))
    torch.cuda.synchronize()
    sizes = [b] * (n // b) + ([n % b] if n % b else [])
    assert [len(g["index"]) for g in got] == sizes and len(got) >= 3
    assert [i for g in got for i in g["index"]] == list(range(n))
    hand = _hand_batches(tf, qs, b, CLASS_ID + 1)
    for g, (qry, qm, gts, szs) in zip(got, hand):
        assert g["sizes"] == szs
        assert g["query_img"].dtype == torch.float32 and g["query_mask"].dtype == torch.uint8
        assert torch.equal(g["query_img"], qry), g["index"]
        assert torch.equal(g["query_mask"], qm), g["index"]
        t = NativeTargets((RES, RES), szs, gt=gts, class_value=CLASS_ID + 1, ignore_value=255)
        r = pipe.segment_queries(bank, qry, qm, captured=False, native=t)
        assert torch.equal(g["counts"], r["counts"]), g["index"]
        assert torch.equal(g["native_counts"], r["native"]["counts"]), g["index"]
        assert int(r["native"]["counts"][:, 2:].sum()) > 0


def test_query_loader_without_ground_truth(models):
    from diffews_amd.input_pipeline import DeviceImageTransform, QueryLoader
    pipe = models["pipe"]
    tf = DeviceImageTransform(RES)
    simg, smap = _host_supports([CLASS_ID + 1], 1, seed=3)
    sup, msk = _hand_supports(tf, simg, smap, [CLASS_ID + 1])
    bank = pipe.prepare_support(sup[0], msk[0])
    qs = _host_queries(3, seed=2, with_gt=False)
    batches = list(QueryLoader(qs, RES, 2, depth=1))
    assert [bt["index"] for bt in batches] == [[0, 1], [2]]
    for bt in batches:
        assert "query_mask" not in bt and not bt["native"].has_gt
    bt = batches[-1]
    r = pipe.segment_queries(bank, bt["query_img"], None, captured=False, native=bt["native"])
    assert r["counts"] is None and r["native"]["counts"] is None
    assert r["native"]["pred"][0].shape == qs[2]["query_img"].shape[:2]
    assert torch.equal(bt["query_img"][0], tf.image(qs[2]["query_img"]))


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_segment_stream_equals_the_hand_written_loop(models, captured):
    """A bank and a class set: segment_stream's pred / labels / counts per query == tf.image per query, NativeTargets(gt =
    host arrays), then segment_queries / segment_classes in the same mode."""
    from diffews_amd.input_pipeline import DeviceImageTransform, NativeTargets
    pipe = models["pipe"]
    pipe._graphs = {}
    tf = DeviceImageTransform(RES)
    n, b = 5, 2
    qs = _host_queries(n, seed=21)
    simg, smap = _host_supports(CLASS_IDS, 1, seed=4)
    sup, msk = _hand_supports(tf, simg, smap, CLASS_IDS)
    try:
        # ---- one support set
        bank = pipe.prepare_support(sup[0], msk[0])
        got = []
        for index, r in pipe.segment_stream(bank, qs, batch=b, size=RES, depth=1, class_value=CLASS_IDS[0], ignore_value=255,
                                            captured=captured):
            assert set(r) == {"z0", "dec", "seg_u8", "counts", "native"}
            got.append((index, [p.clone() for p in r["native"]["pred"]], r["native"]["counts"].clone(), r["counts"].clone()))
        assert [i for g in got for i in g[0]] == list(range(n)) and [len(g[0]) for g in got] == [2, 2, 1]
        for (index, pred, ncounts, counts), (qry, qm, gts, szs) in zip(got, _hand_batches(tf, qs, b, CLASS_IDS[0])):
            t = NativeTargets((RES, RES), szs, gt=gts, class_value=CLASS_IDS[0], ignore_value=255)
            r = pipe.segment_queries(bank, qry, qm, captured=captured, native=t)
            assert torch.equal(ncounts, r["native"]["counts"]) and torch.equal(counts, r["counts"]), index
            for x, y, hw in zip(pred, r["native"]["pred"], szs):
                assert x.shape == hw and torch.equal(x, y), index
        # ---- N classes
        bankset = pipe.prepare_support_classes(sup, msk)
        got = []
        for index, r in pipe.segment_stream(bankset, qs, batch=b, depth=1, ignore_value=255, class_ids=CLASS_IDS,
                                            captured=captured):
            assert set(r) == {"z0", "dec", "seg_u8", "labels", "counts", "native"} and r["counts"] is None
            got.append((index, [p.clone() for p in r["native"]["labels"]], r["native"]["counts"].clone()))
        assert [i for g in got for i in g[0]] == list(range(n))
        for (index, labels, ncounts), (qry, _, gts, szs) in zip(got, _hand_batches(tf, qs, b)):
            t = NativeTargets((RES, RES), szs, gt=gts, ignore_value=255)
            r = pipe.segment_classes(bankset, qry, None, captured=captured, native=t, class_ids=CLASS_IDS)
            assert torch.equal(ncounts, r["native"]["counts"]), index
            for x, y in zip(labels, r["native"]["labels"]):
                assert torch.equal(x, y), index
        with pytest.raises(ValueError):
            next(pipe.segment_stream(bankset, qs, class_value=7))
        with pytest.raises(ValueError):
            next(pipe.segment_stream(bank, qs, class_ids=CLASS_IDS))
        with pytest.raises(TypeError):
            next(pipe.segment_stream(None, qs))
    finally:
        pipe._graphs = {}


def test_evaluate_stream_equals_the_tensor_fed_evaluations(models):
    """evaluate_stream (decoded images in) == evaluate_support_set / evaluate_class_set under use_original_imgsize fed from
    the hand-built tensors: the integer buffers are equal, the binary scores too (same integers, same expression); the
    N-way mIoU is held to the bound tests/test_nway_native_gpu.py uses for it."""
    from diffews_amd import evaluate
    from diffews_amd.input_pipeline import DeviceImageTransform, NativeTargets
    pipe = models["pipe"]
    pipe._graphs = {}
    tf = DeviceImageTransform(RES)
    n, b, s = 5, 2, 2
    qs = _host_queries(n, seed=33)
    simg, smap = _host_supports(CLASS_IDS, s, seed=5)
    sup, msk = _hand_supports(tf, simg, smap, CLASS_IDS)
    hand = _hand_batches(tf, qs, b, CLASS_ID + 1)
    try:
        # ---- binary: class index CLASS_ID, the maps hold CLASS_ID + 1 == CLASS_IDS[0]
        assert CLASS_ID + 1 == CLASS_IDS[0]
        want = evaluate.evaluate_support_set(pipe, sup[0], msk[0], [(qry, qm, gts) for qry, qm, gts, _ in hand], CLASS_ID,
                                             captured=True, use_original_imgsize=True, ignore_value=255)
        got = evaluate.evaluate_stream(pipe, simg[0], smap[0], class_id=CLASS_ID, queries=qs, size=RES, batch=b, depth=1,
                                       captured=True, ignore_value=255)
        assert got[2].intersection_buf.dtype == torch.int64
        assert torch.equal(got[2].intersection_buf, want[2].intersection_buf)
        assert torch.equal(got[2].union_buf, want[2].union_buf) and int(want[2].union_buf.sum()) > 0
        assert want[0] > 0 and want[1] > 0              # the class is one of the fold's: the scores are not vacuous
        assert got[0] == want[0] and got[1] == want[1]
        # ---- N-way
        N = len(CLASS_IDS)
        batches = [(qry, NativeTargets((RES, RES), szs, gt=gts, ignore_value=255)) for qry, _, gts, szs in hand]
        miou, iou, total = evaluate.evaluate_class_set(pipe, sup, msk, batches, captured=False, use_original_imgsize=True,
                                                       class_ids=CLASS_IDS)
        g_miou, g_iou, g_total = evaluate.evaluate_stream(pipe, simg, smap, class_ids=CLASS_IDS, queries=qs, size=RES, batch=b,
                                                          depth=1, captured=False, ignore_value=255)
        assert g_total.dtype == torch.int64 and torch.equal(g_total, total) and int(total[1].sum()) > 0
        assert torch.equal(g_iou, iou)
        assert abs(float(g_miou) - float(miou)) <= 2 * N * 2.0 ** -53 * float(miou), (g_miou, miou)
        with pytest.raises(ValueError):
            evaluate.evaluate_stream(pipe, simg, smap, queries=qs, size=RES)
    finally:
        pipe._graphs = {}
