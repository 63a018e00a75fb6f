"""Stream ordering under certain, not likely, bad interleavings (tests/stream_stall.py): every scenario runs quiet (against
the reference its module's tests use), stalled once per stream it uses (byte-equal to quiet, host-visible state too, with
the ran-ahead witness holding) and once per cuttable edge (must DIFFER from quiet: the scenario sees that edge).

The stall of a scenario is max(20 ms, 4 x the quiet run's host enqueue time), measured in the test itself and printed
(profiles/stream_order.md holds the values of one run); above 250 ms the scenario fails as too large.  Cut runs produce
wrong bytes, never wrong addresses: see SAFETY in tests/stream_stall.py -- sources of one size, no NativeTargets, candidate
or routing tables across a cut edge, every buffer held until the test ends."""
import time

import numpy as np
import pytest
import torch

import query_loader_ref as qr
import scores_ref as sr
import stream_stall as ss

pytestmark = pytest.mark.gpu

RES, PIPE_RES, DEPTH = 32, 64, 1      # the tiny engine runs at 64 x 64, as in every other test of it
NSLOTS = DEPTH + 2
NB = 2 * NSLOTS + 2                   # batches of one: every slot is recycled twice


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def order(hip_lib):
    ss.ticks_per_ms()
    print(f"[stream-order] calibration {ss.CALIBRATION}")
    return ss.Order()


@pytest.fixture(scope="module")
def mods(hip_lib):
    return ss.product_modules()


@pytest.fixture(autouse=True)
def _budget(order):
    """At most 2 s of stalls per test, whatever the number of its runs."""
    order.new_test(apart=[torch.cuda.current_stream()])
    yield
    print(f"[stream-order] stalls enqueued by this test: {order.stalled_ms:.0f} ms, streams drawn again {order.rejected}")


@pytest.fixture(scope="module")
def models(hip_lib):
    """The tiny-config engine of tests/test_query_loader_gpu.py in bf16."""
    from diffews_amd import config, weights
    from diffews_amd.unet import MyUNet2DConditionModel
    from diffews_amd.vae import AutoencoderKL
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise
    from diffews_amd.scheduler import DDIMSchedulerCustomized
    dt = torch.bfloat16
    ucfg, vcfg = config.get("tiny_unet"), config.get("tiny_vae")
    usd = weights.synthetic_unet_state_dict(ucfg, round_to=dt)
    vsd = weights.synthetic_vae_state_dict(vcfg, round_to=dt)
    te = weights.synthetic_text_embed(ucfg).to(dt).float()
    sched = DDIMSchedulerCustomized(**{k: v for k, v in config.get("scheduler").items() if not k.startswith("_")})
    pipe = MarigoldPipelineRGBLatentNoise(MyUNet2DConditionModel(ucfg, usd, torch_dtype=dt), AutoencoderKL(vcfg, vsd, torch_dtype=dt),
                                          sched, text_embeds=te)
    return dict(dt=dt, pipe=pipe)


def _stall_for(scenario, t_host_s):
    ms = ss.stall_length(t_host_s * 1e3)
    print(f"[stream-order] {scenario}: t_host {t_host_s * 1e3:.2f} ms -> stall {ms:.1f} ms")
    return ms


def _same(a, b):
    """Byte-equal nested results (tensors, lists, dicts, host values)."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and \
            torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


# ================================================================================================ S1: the prefetcher

def _sources(n, seed, grow=False):
    """(image, class-id map) pairs: one size, or sizes that grow so fast that a slot's buffers regrow at every reuse."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        h, w = (16 + 12 * i, 20 + 12 * i) if grow else (40, 48)
        out.append((rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(0, 3, (h, w)).astype(np.uint8)))
    return out


def _loader(kind, src, native=False, res=RES):
    """Built under the installed proxy: the loader's stream and events are the proxy's."""
    from diffews_amd.input_pipeline import EpisodeLoader, QueryLoader
    n = len(src) // 2
    if kind == "episodes":
        eps = [dict(query_img=src[i][0], query_mask=src[i][1], support_imgs=[src[n + i][0]], support_masks=[src[n + i][1]],
                    class_id=1) for i in range(n)]
        return EpisodeLoader(eps, res, 1, 1, depth=DEPTH, native=native)
    return QueryLoader([dict(query_img=im, gt=m) for im, m in src[:n]], res, 1, depth=DEPTH, class_value=2)


KEYS = {"episodes": ("support_imgs", "query_img", "support_masks", "query_mask"), "queries": ("query_img", "query_mask")}


def _drain(order, loader, kind, mode="quiet", ms=0.0, cut=None, consumer=None, use=None):
    """One pass over the loader with a consumer that never synchronises and clones each batch on its stream.
    mode "side": the loader's stream is stalled at every _stage entry; "consumer": the consumer's stream in front of
    every clone.  Returns (clones per batch, host enqueue time, the run's log)."""
    cons = consumer or torch.cuda.current_stream()
    got, wit, keep = [], None, []
    t0 = time.perf_counter()
    with order.run(cut=cut, stalls=[(loader.stream, ms)] if mode == "side" else []), torch.cuda.stream(cons):
        for k, bt in enumerate(loader):
            keep.append(bt)                              # every batch object lives until the test ends
            if mode == "consumer":
                order.enqueue_stall(cons, ms)
            g = {key: bt[key].clone() for key in KEYS[kind]}
            if use is not None:
                g.update(use(bt))
            got.append(g)
            if mode == "consumer" and wit is None:
                wit = ss.witness(cons, "the consumer's clone of the first batch")
            if mode == "side" and k == 0:
                order.witness.held("the consumer's clone of the first batch")
            if mode == "side" and cut == ss._COPIED and k == NSLOTS:
                order.witness.held("the hand-over of the batch that refilled the first slot's pinned bytes")
            if mode == "consumer" and k == NSLOTS:
                wit.held("the hand-over of the batch that overwrites the first slot")
        t_host = time.perf_counter() - t0
        log = list(order.log)
    torch.cuda.synchronize()
    loader._keep = keep
    return got, t_host, log


def _check_against_host(kind, got, src, res=RES):
    n = len(src) // 2
    assert len(got) == n
    for i, g in enumerate(got):
        assert torch.equal(g["query_img"][0].cpu(), qr.host_image(src[i][0], (res, res))), i
        assert torch.equal(g["query_mask"][0].cpu().float(), qr.host_mask(src[i][1], 2, (res, res))), i
        if kind == "episodes":
            assert torch.equal(g["support_imgs"][0].cpu(), qr.host_image(src[n + i][0], (res, res))), i
            assert torch.equal(g["support_masks"][0].cpu(), qr.host_mask(src[n + i][1], 2, (res, res))[None].repeat(3, 1, 1) * 2 - 1), i


def _quiet(order, kind, src, res=RES, use=None):
    """The quiet run twice (the first one allocates, loads code objects, captures): the second one's results, host time
    and log."""
    _drain(order, _loader(kind, src, res=res), kind, use=use)
    return _drain(order, _loader(kind, src, res=res), kind, use=use)


def _consumer(order, other):
    """None (the default stream) or a further stream apart from it; the loader built next stays apart from both."""
    if not other:
        return None
    s = order.Stream()
    order.apart.append(s)
    return s


S1_RUNS = [("side", False, None), ("consumer", False, None), ("side", True, None), ("consumer", True, None),
           ("side", False, ss._EVENT), ("side", False, ss._COPIED), ("consumer", False, ss._RELEASE)]


def _s1_id(mode, other, cut):
    edge = "" if cut is None else "-cut-" + cut.split(".")[-1].replace(":", "-")
    return f"{mode}-stalled{'-other-stream' if other else ''}{edge}"


@pytest.mark.parametrize("mode,other,cut", S1_RUNS, ids=[_s1_id(*r) for r in S1_RUNS])
@pytest.mark.parametrize("kind", ["episodes", "queries"])
def test_s1_prefetcher_stalled_and_cut(order, mods, kind, mode, other, cut):
    """Sources of one size, eight batches of one over three slots.  Quiet == Pillow / ATen on the host.  Side stream
    stalled at every _stage entry (`event`, `copied`) or consumer stalled before each clone (`release`), consumer on the
    default or on another stream: byte-equal to quiet.  With `event` or `copied` cut under the side stall, or `release`
    under the consumer stall, the bytes differ."""
    src = _sources(2 * NB, seed=5)
    with order.installed(*mods):
        quiet, t_host, log = _quiet(order, kind, src)
        _check_against_host(kind, quiet, src)
        assert log.count(ss._EVENT) == NB and log.count(ss._RELEASE) == NB - NSLOTS and log.count(ss._COPIED) == NB - NSLOTS
        ms = _stall_for(f"S1 {kind}", t_host)
        consumer = _consumer(order, other)            # before the loader: its stream stays apart from this one too
        got, _, log = _drain(order, _loader(kind, src), kind, mode, ms, cut=cut, consumer=consumer)
        assert order.stall_count == NB and log.count(ss._EVENT) == NB
        if cut is None:
            assert _same(got, quiet)
        else:
            assert order.cut_hits == (NB if cut == ss._EVENT else NB - NSLOTS)
            assert not _same(got, quiet), f"cutting {cut} under a stalled {mode} stream changed nothing: the scenario is blind to it"


@pytest.mark.parametrize("mode,other", [("side", False), ("side", True), ("consumer", False)],
                         ids=["side-stalled", "side-stalled-other-stream", "consumer-stalled"])
@pytest.mark.parametrize("kind", ["episodes", "queries"])
def test_s1_prefetcher_regrows_its_buffers_under_a_stall(order, mods, kind, mode, other):
    """Sources of growing sizes: `dev`, the pinned buffer and `tmp` of a slot regrow at every reuse while the side stream
    still has the previous batch's kernels queued (record_stream); also with the consumer on a non-default stream."""
    src = _sources(2 * NB, seed=6, grow=True)
    with order.installed(*mods):
        quiet, t_host, _ = _quiet(order, kind, src)
        _check_against_host(kind, quiet, src)
        ms = _stall_for(f"S1 {kind} growing", t_host)
        consumer = _consumer(order, other)
        ld = _loader(kind, src)
        seen, slot = [], ld._slot

        def watched(i, lay):
            s = slot(i, lay)
            seen.append((i, s["dev"].numel(), s["tmp"].numel()))
            return s
        ld._slot = watched
        got, _, _ = _drain(order, ld, kind, mode, ms, consumer=consumer)
        assert _same(got, quiet)
        assert len({d for i, d, _ in seen if i == 0}) == 3 and len({t for i, _, t in seen if i == 0}) == 3, "slot 0 did not regrow"


@pytest.mark.parametrize("mode", ["side", "consumer"])
def test_s1_native_targets_of_a_stalled_loader(order, mods, models, mode):
    """QueryLoader batches with their NativeTargets fed to segment_queries(native=...) (the captured step: one graph
    launch per batch, so that the host stays ahead): pred, counts and native counts with the side stream or the consumer
    stalled equal the quiet run's."""
    pipe = models["pipe"]
    src = _sources(2 * NB, seed=7, grow=True)
    g = torch.Generator().manual_seed(3)
    sup = torch.rand(1, 3, PIPE_RES, PIPE_RES, generator=g).cuda() * 2 - 1
    msk = (torch.rand(1, 1, PIPE_RES, PIPE_RES, generator=g) > 0.5).float().repeat(1, 3, 1, 1).cuda() * 2 - 1
    bank = pipe.prepare_support(sup, msk)

    def use(bt):
        r = pipe.segment_queries(bank, bt["query_img"], bt["query_mask"], captured=True, native=bt["native"])
        return dict(pred=[p.clone() for p in r["native"]["pred"]], counts=r["counts"].clone(),
                    native_counts=r["native"]["counts"].clone())
    saved, pipe._graphs = pipe._graphs, {}
    try:
        with order.installed(*mods):
            quiet, t_host, _ = _quiet(order, "queries", src, res=PIPE_RES, use=use)
            _check_against_host("queries", quiet, src, PIPE_RES)
            assert all(q["pred"][0].shape == src[i][1].shape for i, q in enumerate(quiet))
            assert sum(int(q["native_counts"].sum()) for q in quiet) > 0
            ms = _stall_for("S1 native", t_host)
            got, _, _ = _drain(order, _loader("queries", src, res=PIPE_RES), "queries", mode, ms, use=use)
            assert _same(got, quiet)
    finally:
        pipe._graphs = saved


# ================================================================================================ S2: the bucket reducer

BUCKET, NBUCKETS = 4096, 4


def _reducer_case(order, comm_dtype, stalled=None, ms=0.0, cut=None):
    """A flat fp32 buffer of four buckets plus the tail, poisoned with NaN; writers copy the final values bucket by bucket
    from the end towards the start and mark them.  stalled "compute": the current stream is stalled in front of the first
    writer; "comm": the comm stream at every _fire.  Returns dict(snaps per bucket, after = buf.clone() right behind
    finish(), fired_order)."""
    from diffews_amd.train import GradBucketReducer, ParamStore
    n = BUCKET * NBUCKETS
    g = torch.Generator().manual_seed(11)
    final = torch.randn(n + ParamStore.TAIL, generator=g).cuda()
    buf = torch.full((n + ParamStore.TAIL,), float("nan"), device="cuda")
    spec = {f"p{i}": (i * BUCKET // 2, BUCKET // 2) for i in range(2 * NBUCKETS)}
    snaps = {}
    red = GradBucketReducer(buf, spec, bucket_elems=BUCKET, world_size=2, comm_dtype=comm_dtype,
                            collective=lambda t: snaps.__setitem__(len(snaps), t.clone()))
    assert len(red.ranges) == NBUCKETS + 1
    cur = torch.cuda.current_stream()
    t0 = time.perf_counter()
    with order.run(cut=cut, stalls=[(red.comm, ms)] if stalled == "comm" else []):
        red.begin(final[n])
        if stalled == "compute":
            order.enqueue_stall(cur, ms)
        wit = None
        for i in range(2 * NBUCKETS - 1, -1, -1):
            a = i * BUCKET // 2
            buf[a:a + BUCKET // 2].copy_(final[a:a + BUCKET // 2])
            if wit is None:
                wit = ss.witness(cur, "the first writer on the compute stream")
            red.mark([f"p{i}"])
        red.finish()
        after = buf.clone()
        t_host = time.perf_counter() - t0
        if stalled == "compute":
            wit.held("finish(): every collective is enqueued")
        if stalled == "comm":
            order.witness.held("the clone behind finish()")
        log = list(order.log)
    torch.cuda.synchronize()
    return dict(snaps=[snaps[k] for k in sorted(snaps)], after=after, fired_order=list(red.fired_order)), t_host, log, \
        (final, buf, red, snaps)


@pytest.mark.parametrize("comm_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_s2_reducer_stalled_and_cut(order, mods, comm_dtype):
    """(a) compute stream stalled before the first writer: every snapshot holds the final values.  (b) comm stalled at
    _fire: buf.clone() on the compute stream right behind finish() equals final * 0.5 exactly (fp32; the bf16 wire's
    rounding, exactly as the quiet run).  Cuts: _fire's wait_event under (a), finish's wait_stream under (b)."""
    from diffews_amd.train import ParamStore
    keep = []
    with order.installed(*mods):
        keep.append(_reducer_case(order, comm_dtype)[3])         # first use: code objects, the comm stream's pool
        quiet, t_host, log, k = _reducer_case(order, comm_dtype)
        keep.append(k)
        final = k[0]
        n = BUCKET * NBUCKETS
        # the tail range holds no parameter: finish() fires it, with the loss in its first slot
        assert quiet["fired_order"] == [3, 2, 1, 0, 4] and log == [ss._FIRE] * 5 + [ss._FINISH]
        for b, snap in zip(quiet["fired_order"], quiet["snaps"]):
            want = final[b * BUCKET:min((b + 1) * BUCKET, n + ParamStore.TAIL)]
            if b == NBUCKETS:                                   # the rest of the tail was never written
                assert float(snap[0]) == float(final[n].to(comm_dtype))
            else:
                assert torch.equal(snap.float(), want.to(comm_dtype).float())
        if comm_dtype == torch.float32:
            assert torch.equal(quiet["after"][:n + 1], final[:n + 1] * 0.5)
        else:
            assert torch.equal(quiet["after"][:n + 1], final[:n + 1].bfloat16().float() * 0.5)
        ms = _stall_for(f"S2 {comm_dtype}", t_host)
        for stalled in ("compute", "comm"):
            got, _, _, k = _reducer_case(order, comm_dtype, stalled, ms)
            keep.append(k)
            assert _same(got, quiet), stalled
        for stalled, edge in (("compute", ss._FIRE), ("comm", ss._FINISH)):
            got, _, _, k = _reducer_case(order, comm_dtype, stalled, ms, cut=edge)
            keep.append(k)
            assert order.cut_hits >= 1 and not _same(got, quiet), f"cutting {edge} changed nothing"


def test_s2_trainer_backward_with_a_stalled_compute_stream(order, mods):
    """(a) once more through UNetTrainer.forward_backward(reducer=...) on the tiny config, no cut: snapshots, gradient,
    loss and fired_order equal the quiet run's."""
    from test_backward_gpu import _train_setup
    from diffews_amd.train import UNetTrainer, GradBucketReducer
    dtype = torch.bfloat16
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, 1, seed=11)
    args = (z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
    with order.installed(*mods):
        tr = UNetTrainer(ucfg, usd, torch_dtype=dtype)
        tr.forward_backward(*args)                       # warm-up (lazy derived weights)
        spec = {k: (off, max(1, int(torch.tensor(shape).prod()))) for k, (off, shape) in tr.P.spec.items()}
        cur = torch.cuda.current_stream()
        keep = []

        def once(ms):
            for name in tr.P.spec:
                tr.P.g(name).fill_(float("nan"))
            snaps = []
            red = GradBucketReducer(tr.P.grad_buf, spec, bucket_elems=1 << 21, world_size=2,
                                    collective=lambda t: snaps.append(t.clone()))
            keep.append(red)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with order.run():
                wit = None
                if ms:
                    order.enqueue_stall(cur, ms)
                    wit = ss.witness(cur, "the stall in front of the forward")
                loss, _ = tr.forward_backward(*args, reducer=red)
                avg = red.finish().clone()
                grad = tr.P.grad_buf.clone()
                t_host = time.perf_counter() - t0
                if wit is not None:
                    wit.held("finish(): the whole backward is enqueued")
                log = list(order.log)
            torch.cuda.synchronize()
            return dict(snaps=snaps, loss=loss.clone(), avg=avg, grad=grad, fired_order=list(red.fired_order)), t_host, log
        quiet, t_host, log = once(0.0)
        red = keep[-1]
        assert len(quiet["snaps"]) == len(red.ranges) >= 8 and sorted(quiet["fired_order"]) == list(range(len(red.ranges)))
        assert log.count(ss._FIRE) == len(quiet["snaps"]) and log[-1] == ss._FINISH
        final = quiet["grad"] * 2.0                      # the fp32 path multiplied each bucket by 1 / world AFTER the snapshot
        for b, snap in zip(quiet["fired_order"], quiet["snaps"]):
            s0, s1 = red.ranges[b]
            n = min(s1, tr.P.numel) - s0
            assert torch.isfinite(snap[:n]).all() and torch.equal(snap[:n], final[s0:s0 + n]), b
        assert float(quiet["avg"]) == pytest.approx(float(quiet["loss"]) * 0.5)
        got, _, _ = once(_stall_for("S2 trainer", t_host))
        assert _same(got, quiet)


# ================================================================================================ S3: the overflow word

def test_s3_overflow_word_stalled_and_cut(order, mods):
    """fp16 tiny trainer, an inf planted in the gradient, the current stream stalled in front of optimizer_step: the next
    _resolve_overflow still reports the skip (skipped_steps 1, the scale halved, the step taken back).  With
    _resolve_overflow's synchronize cut, on a fresh trainer, the host reads the word before the copy: the outcome differs."""
    from test_backward_gpu import _train_setup
    from diffews_amd.train import UNetTrainer
    dtype = torch.float16
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, 1, seed=7)
    args = (z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
    cur = torch.cuda.current_stream()
    keep = []

    def once(ms, cut=None):
        tr = UNetTrainer(ucfg, usd, torch_dtype=dtype, loss_scale=1024.0)
        keep.append(tr)
        assert tr.dynamic_loss_scale
        tr.forward_backward(*args)
        tr.optimizer_step(1e-4)
        tr._resolve_overflow()
        assert (tr.step_count, tr.skipped_steps, tr.loss_scale) == (1, 0, 1024.0)
        tr.forward_backward(*args)
        tr.P.grad[12345] = float("inf")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with order.run(cut=cut):
            wit = None
            if ms:
                order.enqueue_stall(cur, ms)
                wit = ss.witness(cur, "the stall in front of optimizer_step")
            tr.optimizer_step(1e-4)
            t_host = time.perf_counter() - t0
            if wit is not None:
                wit.held("the host's read of the found-inf word")
            tr._resolve_overflow()
            log = list(order.log)
        torch.cuda.synchronize()
        return dict(step_count=tr.step_count, skipped_steps=tr.skipped_steps, loss_scale=tr.loss_scale,
                    master=tr.P.master.clone()), t_host, log
    with order.installed(*mods):
        quiet, t_host, log = once(0.0)
        assert (quiet["step_count"], quiet["skipped_steps"], quiet["loss_scale"]) == (1, 1, 512.0)
        assert log.count(ss._OVERFLOW) == 1
        ms = _stall_for("S3", t_host)
        got, _, _ = once(ms)
        assert _same(got, quiet)
        got, _, _ = once(ms, cut=ss._OVERFLOW)
        assert order.cut_hits >= 1
        state = lambda r: (r["step_count"], r["skipped_steps"], r["loss_scale"])
        assert state(got) != state(quiet), "cutting the synchronize in front of the found-inf word changed nothing"
        assert torch.equal(got["master"], quiet["master"])       # the device skipped the step either way


# ================================================================================================ S4: the plane table

def test_s4_plane_table_stalled_and_cut(order, mods, ops):
    """Two object_scores calls back to back on a stalled stream with two plane tables of the same number of planes (both
    valid for the same seg_u8): each call's scores equal tests/scores_ref.py for its own table.  With ScoreBuffers.stage's
    synchronize cut the first call reads the second table."""
    from diffews_amd.objects import ScoreBuffers, object_scores
    rs = np.random.RandomState(4)
    B, H, W, cap, N = 1, 24, 40, 8, 3
    lab = np.zeros((B, H, W), np.uint8)
    lab[0, 2:10, 3:20], lab[0, 12:22, 5:15], lab[0, 4:20, 25:38] = 1, 2, 3
    ids_np = lab.astype(np.int32)                                # one object per label: id == label
    u8 = rs.randint(0, 256, (N, 3, H, W)).astype(np.uint8)
    tables = [np.array([[-1, 0, 1, 2]], np.int32), np.array([[-1, 2, 0, 1]], np.int32)]
    want = [sr.scores(ids_np, lab, u8, t, cap) for t in tables]
    assert not np.array_equal(want[0], want[1])
    o = dict(ids=torch.from_numpy(ids_np).cuda(), labels=torch.from_numpy(lab).cuda(),
             stats=torch.zeros(B, cap, 8, dtype=torch.int32, device="cuda"))
    seg = torch.from_numpy(u8).cuda()
    cur = torch.cuda.current_stream()
    keep = []

    def once(ms, cut=None):
        bufs = ScoreBuffers(B, cap, N)
        keep.append(bufs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with order.run(cut=cut):
            wit = None
            if ms:
                order.enqueue_stall(cur, ms)
                wit = ss.witness(cur, "the stall in front of the first call")
            got = []
            for k, t in enumerate(tables):
                r = object_scores(o, seg, torch.from_numpy(t.copy()), buffers=bufs)
                got.append(r["scores"].clone())
                if wit is not None and (k == 0 or cut is not None):      # uncut, the second call waits for the first copy
                    wit.held(f"the return of call {k}")
            t_host = time.perf_counter() - t0
            log = list(order.log)
        torch.cuda.synchronize()
        return got, t_host, log
    with order.installed(*mods):
        once(0.0)                                    # first use: code objects
        quiet, t_host, log = once(0.0)
        assert log == [ss._PLANES]
        for g, w in zip(quiet, want):
            assert np.array_equal(g.cpu().numpy(), w)
        ms = _stall_for("S4", t_host)
        got, _, _ = once(ms)
        assert _same(got, quiet)
        got, _, _ = once(ms, cut=ss._PLANES)
        assert order.cut_hits == 1
        assert not torch.equal(got[0], quiet[0]), "cutting the synchronize in front of the pinned plane table changed nothing"
        assert np.array_equal(got[0].cpu().numpy(), want[1]) and torch.equal(got[1], quiet[1])


# ================================================================================================ S5: host buffers, stalled only

def _stalled_twice(order, scenario, call):
    """call() quiet, then behind a stall on the current stream; the witness is checked when call() has returned, that is
    after the host has dropped or overwritten what the asynchronous copies read."""
    cur = torch.cuda.current_stream()
    torch.cuda.synchronize()
    call()                                        # first use: allocations, lazy tables
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with order.run():
        quiet = call()
        t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    ms = _stall_for(scenario, t_host)
    with order.run():
        order.enqueue_stall(cur, ms)
        wit = ss.witness(cur, "the stall in front of the calls")
        got = call()
        wit.held("the return of the last call")
    torch.cuda.synchronize()
    assert _same(got, quiet), scenario
    return quiet


def test_s5_transform_and_targets_behind_a_stall(order, mods):
    """DeviceImageTransform.batch twice in a row and NativeTargets built twice, the host arrays overwritten as soon as each
    call returns: the pinned staging buffers are dropped while their copies are still queued behind the stall."""
    from diffews_amd.input_pipeline import DeviceImageTransform, NativeTargets
    src = _sources(4, seed=8, grow=True)
    tf = DeviceImageTransform(RES)

    def transform():
        out = []
        for k in (0, 2):
            ims, mks = [src[k][0].copy(), src[k + 1][0].copy()], [src[k][1].copy(), src[k + 1][1].copy()]
            r = tf.batch(ims, mks, [2, 1])
            for a in ims + mks:
                a[...] = 0xEE
            out.append({key: r[key] for key in ("images", "pm1", "bin")})
        return out
    with order.installed(*mods):
        quiet = _stalled_twice(order, "S5 transform", transform)
    for k, r in zip((0, 2), quiet):
        for j in range(2):
            assert torch.equal(r["images"][j].cpu(), qr.host_image(src[k + j][0], (RES, RES)))
            assert torch.equal(r["bin"][j].cpu().float(), qr.host_mask(src[k + j][1], 2 - j, (RES, RES)))

    def targets():
        out = []
        for k in (0, 2):
            gts = [src[k][1].copy(), src[k + 1][1].copy()]
            t = NativeTargets((RES, RES), [g.shape for g in gts], gt=gts, class_value=[2, 1], ignore_value=255)
            for g in gts:
                g[...] = 0xEE
            out.append(t.dev)
            del t
        return out
    with order.installed(*mods):
        quiet = _stalled_twice(order, "S5 targets", targets)
    for k, dev in zip((0, 2), quiet):
        ref = NativeTargets((RES, RES), [src[k][1].shape, src[k + 1][1].shape], gt=[src[k][1], src[k + 1][1]], class_value=[2, 1],
                            ignore_value=255, device=None)
        assert np.array_equal(dev.cpu().numpy(), ref.host)


def _library(pipe, n, seed):
    g = torch.Generator().manual_seed(seed)
    sup = torch.rand(n, 1, 3, PIPE_RES, PIPE_RES, generator=g).cuda() * 2 - 1
    msk = (torch.rand(n, 1, 1, PIPE_RES, PIPE_RES, generator=g) > 0.5).float().repeat(1, 1, 3, 1, 1).cuda() * 2 - 1
    return pipe.prepare_support_classes(sup, msk)


TOL_EP_BF16 = 2.9e-2          # tests/test_support_bank_gpu.py TOL_EP: what the routed and candidate tests allow against one pass


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("route", ["routed", "candidates"])
def test_s5_routed_and_candidate_tables_behind_a_stall(order, mods, models, route):
    """One routed pass / one candidates pass of the tiny pipeline, eager, the caller's route and candidate lists mutated
    as soon as the call returns: the pinned tables built from them are dropped behind the stall.  The quiet result is, per
    entry, within 1.5 x TOL_EP of segment_queries against that entry's own set, as in the routes' own tests."""
    pipe = models["pipe"]
    bankset = _library(pipe, 3, seed=31)
    g = torch.Generator().manual_seed(32)
    qry = (torch.rand(2, 3, PIPE_RES, PIPE_RES, generator=g) * 2 - 1).cuda()

    def one_pass():
        if route == "routed":
            table = [2, 0]
            r = pipe.segment_routed(bankset, qry, table, captured=False)
            table[:] = [1, 1]
            return {k: r[k] for k in ("z0", "seg_u8")}
        cands = [[0, 2], [1]]
        c = pipe.segment_candidates(bankset, qry, cands, captured=False)
        cands[0][:] = [1, 0]
        cands[1][:] = [0]
        return {k: c[k] for k in ("z0", "seg_u8", "labels")}
    with order.installed(*mods):
        quiet = _stalled_twice(order, f"S5 {route}", one_pass)
    entries = [(0, 2), (1, 0)] if route == "routed" else [(0, 0), (0, 2), (1, 1)]      # (query, set) of every entry
    assert quiet["z0"].shape[0] == len(entries)
    for e, (i, c) in enumerate(entries):
        one = pipe.segment_queries(bankset.bank(c), qry[i:i + 1], captured=False)
        assert _rel(quiet["z0"][e:e + 1], one["z0"]) < 1.5 * TOL_EP_BF16, (e, i, c)


@pytest.mark.parametrize("route", ["dense", "candidates"])
def test_s5_tiled_image_and_window_tables_behind_a_stall(order, mods, models, route):
    """segment_tiled on an 80 x 96 image (four windows of 64 x 64), eager, dense and with per-window candidate lists: image
    and ground truth go through one pinned buffer, the window table through another, and the caller overwrites its arrays
    and lists as soon as the call returns.  The quiet labels and counts are those of tests/nway_ref.py on the call's own
    merged bytes (dense) or label map (candidates).  One UNet pass each (the dense route with all four windows in one
    batch, the candidate route with two listed windows in one group): behind a stalled stream the host gets about 18 ms
    of this engine's eager launches ahead, then a launch blocks until the stream moves (measured with three passes: the
    third one's launches returned when the stall ended), and a run in which the host had to wait proves nothing."""
    import nway_ref
    pipe = models["pipe"]
    bankset = _library(pipe, 3, seed=33)
    rs = np.random.RandomState(34)
    hw = (80, 96)
    img0 = rs.randint(0, 256, hw + (3,)).astype(np.uint8)
    gt0 = rs.randint(0, 4, hw).astype(np.uint8)
    gt0[rs.rand(*hw) < 0.05] = 255
    lists = [[0], [2], [], []]
    keys = ("seg_u8", "labels", "counts", "mx") if route == "dense" else ("labels", "counts", "mx", "area")

    def one_pass():
        img, gt, cands = img0.copy(), gt0.copy(), [list(c) for c in lists]
        r = pipe.segment_tiled(bankset, img, gt, batch=4 if route == "dense" else 2, captured=False, entry_batch=2,
                               candidates=cands if route == "candidates" else None)
        img[...] = 0xEE
        gt[...] = 0xEE
        for c in cands:
            c[:] = [0]
        assert r["plan"].T == 4
        return {k: r[k].clone() for k in keys}
    with order.installed(*mods):
        quiet = _stalled_twice(order, f"S5 tiled {route}", one_pass)
    gt_t = torch.from_numpy(gt0)[None]
    if route == "dense":
        ref_l, ref_c = nway_ref.seg_labels(quiet["seg_u8"].cpu()[:, None], gt_t)
        assert torch.equal(quiet["labels"].cpu(), ref_l[0]) and torch.equal(quiet["counts"].cpu(), ref_c[0])
    else:
        assert torch.equal(quiet["counts"].cpu(), nway_ref.counts(quiet["labels"].cpu()[None], gt_t, 3)[0])
        assert quiet["area"].shape == (3, 2) and int(quiet["area"].sum()) > 0


def test_s5_captured_stream_with_the_loader_running(order, mods, models):
    """segment_stream(captured=True) with its loader running and the consumer stream stalled in front of every batch:
    warm-up on a side stream, capture, static-input copies in front of each replay.  pred and counts equal the quiet run's,
    which equals the eager route."""
    pipe = models["pipe"]
    src = _sources(2 * 4, seed=9, grow=True)
    qs = [dict(query_img=im, gt=m) for im, m in src[:4]]
    g = torch.Generator().manual_seed(3)
    sup = torch.rand(1, 3, PIPE_RES, PIPE_RES, generator=g).cuda() * 2 - 1
    msk = (torch.rand(1, 1, PIPE_RES, PIPE_RES, generator=g) > 0.5).float().repeat(1, 3, 1, 1).cuda() * 2 - 1
    bank = pipe.prepare_support(sup, msk)
    cur = torch.cuda.current_stream()

    def stream(captured, ms=0.0):
        got, wit = [], None
        t0 = time.perf_counter()
        with order.run():
            for index, r in pipe.segment_stream(bank, qs, batch=1, size=PIPE_RES, depth=DEPTH, class_value=2, ignore_value=255,
                                                captured=captured):
                got.append(dict(index=list(index), pred=[p.clone() for p in r["native"]["pred"]],
                                ncounts=r["native"]["counts"].clone(), counts=r["counts"].clone()))
                if ms:
                    order.enqueue_stall(cur, ms)
                    if wit is None:
                        wit = ss.witness(cur, "the stall behind the first batch")
            t_host = time.perf_counter() - t0
            if wit is not None:
                wit.held("the last replay")
            log = list(order.log)
        torch.cuda.synchronize()
        return got, t_host, log
    saved, pipe._graphs = pipe._graphs, {}
    try:
        with order.installed(*mods):
            eager, _, _ = stream(False)
            first, _, log = stream(True)             # captures: the warm-up edges are passed here
            assert [n.split(":")[1] for n in log if "._replay:" in n] == ["wait_stream#0", "wait_stream#1", "synchronize#0"]
            quiet, t_host, log = stream(True)        # replays only
            assert not any("._replay:" in n for n in log)
            assert _same(first, eager) and _same(quiet, eager)
            got, _, _ = stream(True, _stall_for("S5 captured stream", t_host))
            assert _same(got, quiet)
    finally:
        pipe._graphs = saved


# ================================================================================================ S6: allocator edges

def test_s6_targets_dropped_and_restaged_on_the_loaders_stream(order, mods, models):
    """A NativeTargets staged on a side stream is consumed by segment_queries on the stalled main stream and dropped; the
    side stream at once stages a second NativeTargets of the same sizes (the allocator's favourite block) with another
    class value and ground truth.  The first call's result equals the quiet run's: ops._native_setup's record_stream keeps
    the block until the stalled read has run."""
    import native_ref
    from diffews_amd.input_pipeline import NativeTargets
    pipe = models["pipe"]
    g = torch.Generator().manual_seed(3)
    sup = torch.rand(1, 3, PIPE_RES, PIPE_RES, generator=g).cuda() * 2 - 1
    msk = (torch.rand(1, 1, PIPE_RES, PIPE_RES, generator=g) > 0.5).float().repeat(1, 3, 1, 1).cuda() * 2 - 1
    bank = pipe.prepare_support(sup, msk)
    qry = (torch.rand(2, 3, PIPE_RES, PIPE_RES, generator=g) * 2 - 1).cuda()
    rs = np.random.RandomState(12)
    sizes = [(40, 48), (23, 37)]
    gts = [[rs.randint(0, 3, hw).astype(np.uint8) for hw in sizes] for _ in range(2)]
    side, cur = order.Stream(), torch.cuda.current_stream()
    base = {k: v.clone() for k, v in pipe.segment_queries(bank, qry, captured=False).items() if k in ("z0", "seg_u8")}

    def once(ms):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with order.run():
            with torch.cuda.stream(side):
                t = NativeTargets((PIPE_RES, PIPE_RES), sizes, gt=gts[0], class_value=[1, 2], ignore_value=255)
                staged = torch.cuda.Event()
                staged.record(side)
            cur.wait_event(staged)
            wit = None
            if ms:
                order.enqueue_stall(cur, ms)
                wit = ss.witness(cur, "the stall in front of the consuming call")
            r = pipe.segment_queries(bank, qry, captured=False, native=t)
            ptr = t.dev.data_ptr()
            del t
            with torch.cuda.stream(side):
                t2 = NativeTargets((PIPE_RES, PIPE_RES), sizes, gt=gts[1], class_value=[2, 1], ignore_value=255)
            t_host = time.perf_counter() - t0
            if wit is not None:
                wit.held("the second staging on the side stream")
            out = dict(pred=[p.clone() for p in r["native"]["pred"]], counts=r["native"]["counts"].clone())
        torch.cuda.synchronize()
        return out, t_host, (ptr, t2.dev.data_ptr())
    with order.installed(*mods):
        once(0.0)
        quiet, t_host, _ = once(0.0)
        want = pipe.segment_queries(bank, qry, captured=False,
                                    native=NativeTargets((PIPE_RES, PIPE_RES), sizes, gt=gts[0], class_value=[1, 2], ignore_value=255))
        torch.cuda.synchronize()
        assert _same(quiet, dict(pred=list(want["native"]["pred"]), counts=want["native"]["counts"]))
        got, _, ptrs = once(_stall_for("S6", t_host))
        assert _same(got, quiet)
        assert ptrs[0] != ptrs[1], "the block of the targets still being read was handed out again"
    assert torch.equal(base["seg_u8"], want["seg_u8"])
    ref = native_ref.native_ref(base["seg_u8"], sizes, gts[0], [1, 2], 255)          # Pillow's resize and the launcher's rule
    assert torch.equal(quiet["counts"].cpu(), ref["counts"])
    for p, q in zip(quiet["pred"], ref["pred"]):
        assert torch.equal(p.cpu(), q)


# ================================================================================================ S7: captured training steps

@pytest.mark.parametrize("form", ["captured", "segmented"])
def test_s7_captured_training_step_behind_a_stall(order, mods, form):
    """forward_backward_captured / forward_backward_segmented on the tiny trainer: the capture passes the warm-up edges
    (side stream, device synchronize); a replay behind a stalled stream, its inputs overwritten by the caller as soon as the
    call returns, gives the loss, prediction and gradient of the quiet replay, which are the eager step's (a second
    trainer; the segmented form against the eager overlapped step with the same injected collective)."""
    from test_backward_gpu import _train_setup
    from diffews_amd.train import UNetTrainer
    dtype = torch.bfloat16
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, 1, seed=13)
    cur = torch.cuda.current_stream()
    with order.installed(*mods):
        a, b = UNetTrainer(ucfg, usd, torch_dtype=dtype), UNetTrainer(ucfg, usd, torch_dtype=dtype)
        ra = rb = None
        if form == "segmented":
            ra = a.make_reducer(bucket_elems=1 << 21, world_size=2, collective=lambda t: t.mul_(2.0))
            rb = b.make_reducer(bucket_elems=1 << 21, world_size=2, collective=lambda t: t.mul_(2.0))

        def once(ms, eager=False):
            tr = a if eager else b
            ins = [z_refcat.cuda(), z_tag.cuda(), target.cuda()]
            e = ehs.cuda()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with order.run():
                wit = None
                if ms:
                    order.enqueue_stall(cur, ms)
                    wit = ss.witness(cur, "the stall in front of the replay")
                if form == "captured":
                    loss, pred = (tr.forward_backward if eager else tr.forward_backward_captured)(ins[0], ins[1], ins[2], 1, e)
                elif eager:
                    _, pred = tr.forward_backward(ins[0], ins[1], ins[2], 1, e, reducer=ra)
                    loss = ra.finish()
                else:
                    loss, pred = tr.forward_backward_segmented(ins[0], ins[1], ins[2], 1, e, rb)
                out = dict(loss=loss.clone(), pred=pred.clone(), grad=tr.P.grad.clone())
                for t in ins:
                    t.fill_(7.0)                     # queued behind the static-input copies on the same stream
                t_host = time.perf_counter() - t0
                if wit is not None:
                    wit.held("the overwrite of the caller's inputs")
                log = list(order.log)
            torch.cuda.synchronize()
            if rb is not None and not eager:
                out["fired_order"] = list(rb.fired_order)
            return out, t_host, log
        eager, _, _ = once(0.0, eager=True)
        if ra is not None:
            eager["fired_order"] = list(ra.fired_order)
        first, _, log = once(0.0)
        name = f"UNetTrainer.forward_backward_{form}:"
        waits = ["wait_stream#0", "wait_stream#1", "synchronize#0"] + (["wait_stream#2"] if form == "segmented" else [])
        assert [n for n in log if n.startswith(name)] == [name + w for w in waits]
        quiet, t_host, log = once(0.0)
        assert not any(n.startswith(name) for n in log)
        assert _same(first, eager) and _same(quiet, eager)
        got, _, _ = once(_stall_for(f"S7 {form}", t_host))
        assert _same(got, quiet)
