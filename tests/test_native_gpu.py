"""GPU tests of the native-size stage (ops.seg_native, csrc/seg_native.hip) against tests/native_ref.py -- Pillow's own
resize and the launcher's own torch expressions: every comparison is exact.  Ragged batches (odd widths, sizes below one
block, more than one block per axis, the identity, one image of 1 x 7), 0xA5 guards around every packed region, the three
thresholding modes, the three ground-truth forms, a fixed launch count, the tiny pipeline eager and captured, and the
loader + evaluation loop under use_original_imgsize."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import native_ref as nr

pytestmark = pytest.mark.gpu

SOURCES = [(64, 64), (40, 72)]
RAGGED = [(97, 131), (23, 37), (64, 50), (64, 64), (333, 500)]
SINGLE = [(1, 7)]
MODES = [(0.25, 0.0, False), (0.25, 0.0, True), (0.0, 0.5, False)]      # per image, batch_max, fixed threshold
DTYPES = [torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=None)
def _source(src, b):
    """uint8 [b, 3, Hs, Ws]: random, all-zero, all-255, a dim random image, random (cycled over b)."""
    g = torch.Generator().manual_seed(src[0] * 7 + src[1] + b)
    x = (torch.rand(b, 3, *src, generator=g) * 256).to(torch.uint8)
    for i in range(b):
        if i % 5 == 1:
            x[i] = 0
        elif i % 5 == 2:
            x[i] = 255
        elif i % 5 == 3:
            x[i] //= 3
    return x


CASES = [(src, sizes) for src in SOURCES for sizes in (RAGGED, SINGLE)] + [(nr.OVERSHOOT_SRC, [nr.OVERSHOOT_SIZE])]
CASE_IDS = [f"{s[0]}x{s[1]}-b{len(z)}" for s, z in CASES]


def _input(src, sizes):
    return nr.overshoot_image() if src == nr.OVERSHOOT_SRC else _source(src, len(sizes))


@functools.lru_cache(maxsize=None)
def _resized(src, sizes):
    """Pillow's resize of every image of the case, computed once and shared (never written)."""
    x = _input(src, list(sizes))
    return [nr.resize_u8(x[i], h, w) for i, (h, w) in enumerate(sizes)]


def _gts(sizes, form, seed=0):
    """Ground truth per query: 'mask' uint8 0/1/255, 'ids8' uint8 class map, 'ids32' int32 class map (class 7, some 255)."""
    rs = np.random.RandomState(11 + seed)
    out = []
    for h, w in sizes:
        if form == "mask":
            g = (rs.rand(h, w) > 0.5).astype(np.uint8)
        else:
            g = rs.choice([0, 3, 7, 7, 9], size=(h, w)).astype(np.uint8 if form == "ids8" else np.int32)
        g[rs.rand(h, w) < 0.07] = 255
        out.append(g)
    return out


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.mark.parametrize("src,sizes", CASES, ids=CASE_IDS)
def test_resized_bytes_equal_pillow_and_guards_hold(ops, src, sizes):
    """out_u8 of every image == Image.fromarray(hwc).resize((w, h)); tmp and both packed outputs are pre-filled with 0xA5
    and laid out with 64 guard bytes after every image: no byte outside an image's own region is written."""
    from diffews_amd.input_pipeline import NativeTargets
    x = _input(src, sizes).cuda()
    t = NativeTargets(src, sizes, guard=64)
    fill = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    u8, pred, tmp = fill(t.u8_bytes), fill(t.pred_bytes), fill(t.tmp_bytes)
    r = ops.seg_native(x, t, 0.25, 0.0, False, u8_out=u8, pred_out=pred, tmp=tmp)
    ref = _resized(src, tuple(sizes))
    assert r["counts"] is None and r["sizes"] == list(sizes)
    for i, (h, w) in enumerate(sizes):
        assert r["seg_u8"][i].shape == (3, h, w) and r["pred"][i].shape == (h, w)
        assert torch.equal(r["seg_u8"][i].cpu(), ref[i]), (i, h, w, int((r["seg_u8"][i].cpu() != ref[i]).sum()))
        assert int(r["mx"][i]) == int(ref[i].max()), (i, h, w)
    for buf, offs, per in ((u8.cpu(), [it.u8_off for it in t.items], [3 * h * w for h, w in sizes]),
                           (pred.cpu(), [it.pred_off for it in t.items], [h * w for h, w in sizes]),
                           (tmp.cpu(), [it.tmp_off for it in t.items], [3 * src[0] * w for _, w in sizes])):
        ends = offs[1:] + [buf.numel()]
        for o, n, e in zip(offs, per, ends):
            assert e - (o + n) >= 64 and bool((buf[o + n:e] == 0xA5).all()), (o, n, e)
        assert not bool((tmp.cpu()[:per[0]] == 0xA5).all())
    # the packed views are views of the caller's buffers
    assert r["seg_u8"][0].data_ptr() == u8.data_ptr() + t.items[0].u8_off
    # without want_u8 the resized bytes are staged behind tmp: same predictions and maxima, nothing returned
    r2 = ops.seg_native(x, t, 0.25, 0.0, False, want_u8=False)
    assert r2["seg_u8"] is None and torch.equal(r2["mx"], r["mx"])
    for a, b_ in zip(r2["pred"], r["pred"]):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("form", ["mask", "ids8", "ids32"])
@pytest.mark.parametrize("src,sizes", CASES, ids=CASE_IDS)
def test_pred_and_counts_equal_reference(ops, src, sizes, form):
    """pred and counts == native_ref for r_threshold 0.25 per image, batch_max and the fixed threshold 0.5, ground truth as
    uint8 0/1/255, uint8 class map and int32 class map (class_value 7), ignore_value 255 and -1; the all-zero image predicts
    no foreground; on the overshoot input the mask is the one of the RESIZED maximum (225), not of the source's (200)."""
    from diffews_amd.input_pipeline import NativeTargets
    x = _input(src, sizes)
    xd = x.cuda()
    gts = _gts(sizes, form)
    cv = 1 if form == "mask" else 7
    for ign in (255, -1):
        t = NativeTargets(src, sizes, gt=gts, class_value=cv, ignore_value=ign)
        for r_thr, thr, bmax in MODES:
            r = ops.seg_native(xd, t, r_thr, thr, bmax)
            ref = nr.native_ref(x, sizes, gts, cv, ign, r_thr, thr, bmax)
            what = (form, ign, r_thr, thr, bmax)
            for i in range(len(sizes)):
                assert torch.equal(r["pred"][i].cpu(), ref["pred"][i]), (what, i, sizes[i])
                if len(sizes) > 1 and i % 5 == 1:
                    assert int(r["pred"][i].sum()) == 0
            assert r["counts"].dtype == torch.int64 and torch.equal(r["counts"].cpu(), ref["counts"]), what
    if src == nr.OVERSHOOT_SRC:
        r = ops.seg_native(xd, NativeTargets(src, sizes), 0.25, 0.0, False)
        res = nr.to_tensor(_resized(src, tuple(sizes))[0].permute(1, 2, 0).numpy())
        before = nr.predict(res, 0.25, 0.0, mx=torch.tensor(200, dtype=torch.float32).div(255)).to(torch.uint8)
        assert int(r["mx"][0]) == 225 and not torch.equal(r["pred"][0].cpu(), before)


def test_launch_count_does_not_depend_on_the_batch(ops, hip_lib):
    """The table is staged beforehand; the stage captured with b = 1 and with b = 5 has the same number of nodes (zero,
    horizontal, vertical + maximum, count), all kernels: no memset node."""
    from diffews_amd.input_pipeline import NativeTargets
    nodes = []
    for sizes in (RAGGED[:1], RAGGED):
        x = _source((64, 64), len(sizes)).cuda()
        gts = _gts(sizes, "ids8")
        t = NativeTargets((64, 64), sizes, gt=gts, class_value=7, ignore_value=255)
        eager = ops.seg_native(x, t)                       # also warms the allocator
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = ops.seg_native(x, t)
        n = C.c_int32(0)
        assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(n)) == 0
        nodes.append(n.value)
        graph.instantiate()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["counts"], eager["counts"])
        for a, b_ in zip(out["pred"], eager["pred"]):
            assert torch.equal(a, b_)
    assert nodes[0] == nodes[1] == 4, nodes


# ------------------------------------------------------------------------------------------------ the tiny pipeline

def _kw(c):
    return {k: v for k, v in c.items() if not k.startswith("_")}


@pytest.fixture(scope="module", params=DTYPES, ids=["bf16", "f16"])
def models(request, hip_lib):
    """The tiny-config engine of tests/test_support_bank_gpu.py (same seeds, weights rounded to the dtype)."""
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


def _support_set(s, H, seed):
    g = torch.Generator().manual_seed(seed)
    sup = torch.rand(s, 3, H, H, generator=g) * 2 - 1
    m = torch.zeros(s, 1, H, H)
    m[:, :, H // 4:3 * H // 4, H // 4:3 * H // 4] = 1
    m = (m + (torch.rand(s, 1, H, H, generator=g) < 0.02).float()) % 2
    return sup, m.repeat(1, 3, 1, 1) * 2 - 1


def _check_native(r, sizes, gts, cv, ign, flags):
    ref = nr.native_ref(r["seg_u8"].cpu(), sizes, gts, cv, ign, *flags)
    n = r["native"]
    for i in range(len(sizes)):
        assert torch.equal(n["seg_u8"][i].cpu(), ref["seg_u8"][i]), (i, sizes[i])
        assert torch.equal(n["pred"][i].cpu(), ref["pred"][i]), (i, sizes[i])
    assert torch.equal(n["counts"].cpu(), ref["counts"])


def test_pipeline_native_entry(models):
    """segment_queries(..., native=t) and run_episodes(..., native=t): r["native"] == native_ref(r["seg_u8"]) exactly; z0, dec,
    seg_u8 and counts are bit-equal to the call without `native`; captured replays give what eager gives on two consecutive
    batches of different native sizes (the stage is outside the graph: one graph serves both)."""
    from diffews_amd.input_pipeline import NativeTargets
    pipe = models["pipe"]
    pipe._graphs = {}
    b, s, S = 2, 1, 64
    sup, msk = (t.cuda() for t in _support_set(s, S, seed=31))
    bank = pipe.prepare_support(sup, msk)
    gt = (torch.rand(b, S, S, generator=torch.Generator().manual_seed(1)) > 0.5).to(torch.uint8).cuda()
    flags = (0.25, 0.0, False)
    rep = lambda x: x.repeat(b, 1, 1, 1)
    batches = [([(48, 64), (97, 131)], 41), ([(80, 56), (64, 64)], 42)]
    entries = {"segment_queries": lambda qry, cap, **kw: pipe.segment_queries(bank, qry, gt, captured=cap, **kw),
               "run_episodes": lambda qry, cap, **kw: pipe.run_episodes(rep(sup), qry, rep(msk), gt, captured=cap, **kw)}
    clone = lambda r: {k: v.clone() for k, v in r.items()}
    for sizes, seed in batches:
        qry = (torch.rand(b, 3, S, S, generator=torch.Generator().manual_seed(seed)) * 2 - 1).cuda()
        gts = _gts(sizes, "ids8", seed)
        t = NativeTargets((S, S), sizes, gt=gts, class_value=7, ignore_value=255)
        for name, call in entries.items():
            eager = None
            for captured in (False, True):
                plain = clone(call(qry, captured))
                assert set(plain) == {"z0", "dec", "seg_u8", "counts"}
                r = call(qry, captured, native=t)
                assert set(r) == {"z0", "dec", "seg_u8", "counts", "native"}
                for k in plain:
                    assert torch.equal(plain[k], r[k]), (name, captured, k)
                _check_native(r, sizes, gts, 7, 255, flags)
                if eager is None:
                    eager = r
                    continue
                assert torch.equal(eager["seg_u8"], r["seg_u8"]), name
                assert torch.equal(eager["native"]["counts"], r["native"]["counts"]), name
                for x, y in zip(eager["native"]["pred"] + eager["native"]["seg_u8"], r["native"]["pred"] + r["native"]["seg_u8"]):
                    assert torch.equal(x, y), name
    assert len(pipe._graphs) == 2            # one per entry point: native sizes are not part of the key
    pipe._graphs = {}


def _host_episodes(n, nshot, seed):
    """Synthetic host episodes (the material of DatasetCOCO.load_frame): queries of 48x64, 80x56, 64x64 in turn, class-id
    maps holding class_id + 1, other ids and -- in episode 1 -- 255 boundary pixels."""
    rs = np.random.RandomState(seed)
    sizes = [(48, 64), (80, 56), (64, 64)]
    eps = []
    for i in range(n):
        h, w = sizes[i % 3]
        cid = [3, 7, 12][i % 3]

        def ids(hh, ww):
            m = rs.choice([0, cid + 1, cid + 1, 40], size=(hh, ww)).astype(np.uint8)
            m[hh // 4:hh // 2, ww // 4:ww // 2] = cid + 1
            return m
        qm = ids(h, w)
        if i == 1:
            qm[rs.rand(h, w) < 0.1] = 255
        eps.append(dict(query_img=rs.randint(0, 256, (h, w, 3)).astype(np.uint8), query_mask=qm,
                        support_imgs=[rs.randint(0, 256, (56, 72, 3)).astype(np.uint8) for _ in range(nshot)],
                        support_masks=[ids(56, 72) for _ in range(nshot)], class_id=cid))
    return eps


def test_loader_and_evaluation_at_native_size(models):
    """Six host episodes through EpisodeLoader(native=True) and evaluate.test_diffusion(use_original_imgsize=True), res 64,
    batch 2, ignore_value 255: the meter's two int64 buffers == a host loop feeding native_ref of the same pipeline outputs
    (seg_u8 of every step, recorded) and the episodes' own class-id maps into an AverageMeter."""
    from diffews_amd import evaluate
    from diffews_amd.metrics import AverageMeter, fold_class_ids
    pipe = models["pipe"]
    pipe._graphs = {}
    eps = _host_episodes(6, 1, seed=9)
    seen, inner = [], pipe.run_episodes

    def recording(*a, **kw):
        r = inner(*a, **kw)
        seen.append((r["seg_u8"].clone().cpu(), list(kw["native"].sizes), r["native"]["counts"].clone().cpu()))
        return r
    pipe.run_episodes = recording
    try:
        miou, fb, meter = evaluate.test_diffusion(pipe, 6, nshot=1, res=64, batch=2, episodes=eps,
                                                  use_original_imgsize=True, ignore_value=255)
    finally:
        del pipe.run_episodes
        pipe._graphs = {}
    assert len(seen) == 3
    host = AverageMeter("coco", fold_class_ids("coco", 0), device="cpu")
    for j, (seg, sizes, counts) in enumerate(seen):
        batch = eps[2 * j:2 * j + 2]
        assert sizes == [e["query_mask"].shape for e in batch]
        ref = nr.native_ref(seg, sizes, [e["query_mask"] for e in batch], [e["class_id"] + 1 for e in batch], 255)
        assert torch.equal(counts, ref["counts"]), j
        host.update_from_counts(ref["counts"], torch.tensor([e["class_id"] for e in batch]))
    assert meter.intersection_buf.dtype == torch.int64
    assert torch.equal(meter.intersection_buf.cpu(), host.intersection_buf)
    assert torch.equal(meter.union_buf.cpu(), host.union_buf)
    assert int(host.union_buf.sum()) > 0
