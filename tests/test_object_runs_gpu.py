"""GPU tests of the run-length stage: ops.seg_rle against tests/rle_ref.py on runs, run_off and nruns, in both orders, on
ids that ops.seg_components made (4 and 8 neighbours) at the smallest shapes that reach every path of the kernels -- one
pixel, one row, one column, exactly a scan block, a block plus one, three blocks with an odd width (the scalar path), a
width that is a multiple of four -- and on hand-made id maps that cross the sort's digit boundaries and chunk sizes; then
truncation, the area / box invariants, batches, guards, poisoned and repeated launches, a captured launch behind
seg_components, and objects.object_runs / runs_to_host / runs_to_coco / runs_to_mask / pipe.object_runs on top.  All
integers: every comparison is exact.

Every buffer sits inside sentinel guards.  All buffers of this stage hold 32-bit words, so the odd pad that puts a byte
buffer off word alignment elsewhere is here a pad of 61 WORDS in front of ids and of 60 bytes in front of the workspace:
both then miss the 16-byte alignment of the vector loads and take the scalar path (a workspace off word alignment is
DFW_ESHAPE, tests/test_object_runs_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rle_ref as rr

pytestmark = pytest.mark.gpu

SENT = 0xA5


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def block(hip_lib):
    p, r = C.c_int32(), C.c_int32()
    assert hip_lib.dfw_seg_rle_block(C.byref(p), C.byref(r)) == 0
    return p.value, r.value


class _Guarded:
    """A tensor inside a flat allocation with `pad` sentinel elements (0xA5 bytes / -7 words) on either side; the tensor
    itself starts as sentinels too, or as `fill` bytes."""

    def __init__(self, shape, dtype, pad, fill=None):
        n = int(np.prod(shape))
        self.sent = SENT if dtype == torch.uint8 else -7
        self.flat = torch.full((n + 2 * pad,), self.sent, dtype=dtype, device="cuda")
        self.t = self.flat[pad:pad + n].view(shape)
        self.pad, self.n = pad, n
        if fill is not None:
            self.t.view(torch.uint8).fill_(fill)

    def check(self, name):
        assert (self.flat[:self.pad] == self.sent).all() and (self.flat[self.pad + self.n:] == self.sent).all(), f"wrote outside {name}"


def _components(ops, labels, conn, cap=8):
    """ids and stats of ops.seg_components on numpy uint8 [B, H, W]."""
    lab = torch.from_numpy(labels).cuda()
    B, H, W = lab.shape
    ids = torch.empty(B, H, W, dtype=torch.int32, device="cuda")
    n = torch.empty(B, 2, dtype=torch.int32, device="cuda")
    stats = torch.empty(B, cap, 8, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.seg_components_workspace(B, H, W), dtype=torch.uint8, device="cuda")
    ops.seg_components(lab, ids, n, ws, stats=stats, connectivity=conn)
    return ids.cpu().numpy(), stats.cpu().numpy(), n.cpu().numpy()


def _launch(ops, ids, cap, max_runs, order, pad=4, ws_pad=64, fill=None, bufs=None, repeat=1):
    """ops.seg_rle on `ids` (numpy int32 [B, H, W]) into guarded buffers, optionally pre-filled with a byte; returns numpy
    results after checking every guard, and the buffers."""
    B, H, W = ids.shape
    if bufs is None:
        bufs = dict(ids=_Guarded((B, H, W), torch.int32, pad), runs=_Guarded((B, max_runs, 2), torch.int32, 4, fill),
                    run_off=_Guarded((B, cap + 1), torch.int32, 4, fill), nruns=_Guarded((B, 2), torch.int32, 4, fill),
                    ws=_Guarded((ops.seg_rle_workspace(B, H, W, cap, max_runs, order),), torch.uint8, ws_pad, fill))
    bufs["ids"].t.copy_(torch.from_numpy(ids))
    g = {k: v.t for k, v in bufs.items()}
    for _ in range(repeat):
        ops.seg_rle(g["ids"], g["runs"], g["run_off"], g["nruns"], g["ws"], cap, order)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert np.array_equal(g["ids"].cpu().numpy(), ids), "the input was modified"
    return {k: g[k].cpu().numpy() for k in ("runs", "run_off", "nruns")}, bufs


def _same(got, want, what, rest=-7):
    """nruns and run_off whole, runs up to kept; the rows behind hold `rest`, what the buffer was filled with."""
    assert np.array_equal(got["nruns"], want["nruns"]), (what, got["nruns"].tolist(), want["nruns"].tolist())
    assert np.array_equal(got["run_off"], want["run_off"]), (what, "run_off")
    for b, w in enumerate(want["runs"]):
        assert np.array_equal(got["runs"][b, :len(w)], w), (what, "runs", b, int((got["runs"][b, :len(w)] != w).sum()))
        assert (got["runs"][b, len(w):] == rest).all(), (what, "rows behind kept were written", b)


def _word(fill):
    return int(np.array([fill] * 4, np.uint8).view(np.int32)[0])


def _shapes(block):
    P, _ = block
    assert P % 64 == 0 and (P + 1) % 3 == 0
    return [(1, 1), (1, 37), (37, 1), (5, 7), (P // 64, 64), (3, (P + 1) // 3), (75, 3 * P // 75 + 2), (70, 60)]


@pytest.mark.parametrize("which", range(8), ids=["1x1", "1x37", "37x1", "5x7", "block", "block+1", "3-blocks-odd-W", "W%4==0"])
def test_equals_the_reference(ops, block, which):
    """Every content, ids of both connectivities, both orders, cap = 1 / 16 / above every id; max_runs = H * W, so nothing
    truncates.  The ids buffer of the 8-neighbour half lies 61 words into its allocation, its workspace 60 bytes."""
    P, R = block
    H, W = _shapes(block)[which]
    if which == 4:
        assert H * W == P
    if which == 5:
        assert H * W == P + 1 and W % 2 == 1
    if which == 6:
        assert 3 * P < H * W < 4 * P and W % 2 == 1
    if which == 7:
        assert W % 4 == 0 and H * W > 2 * P
    rs = np.random.RandomState(1000 * H + W)
    for name, lab in rr.contents(H, W, rs).items():
        for conn in (4, 8):
            ids, _, n = _components(ops, lab[None], conn)
            top = int(ids.max())
            assert top == n[0, 0]
            for cap in (1, 16, top + 3):
                for order in rr.ORDERS:
                    want = rr.rle(ids, cap, H * W, order)
                    got, _ = _launch(ops, ids, cap, H * W, order, pad=61 if conn == 8 else 4, ws_pad=60 if conn == 8 else 64)
                    _same(got, want, (name, H, W, conn, cap, order))
                    found = int(want["nruns"][0, 1])
                    if name == "background":
                        assert found == 0 and not got["run_off"].any()
                    if name == "one object":
                        assert got["runs"][0, 0].tolist() == [0, H * W] and found == 1      # one run over every block
                    if name == "vertical stripes" and cap > top and H > 1 and W > 3:
                        assert found == (top if order == "column" else H * top)
                    if name == "horizontal stripes" and cap > top and W > 1 and H > 3:
                        assert found == (top if order == "row" else W * top)                 # a run wraps the line's end


@pytest.mark.parametrize("cap", [255, 256, 257, 65535, 65537])
def test_hand_made_ids_across_the_sort_digits(ops, block, cap):
    """40 x 50, ids random in [-2, cap + 3] (so: negative, zero, the cap itself, above it): one, two and three digit passes
    at a size that costs nothing.  Low ids are made frequent so that runs of one id meet and objects hold several runs."""
    rs = np.random.RandomState(cap)
    ids = rs.randint(-2, cap + 4, (1, 40, 50)).astype(np.int32)
    ids[0, rs.rand(40, 50) < 0.3] = cap                                    # the highest digit pattern, often
    ids[0, rs.rand(40, 50) < 0.3] = rs.randint(1, 4)
    ids[0, 7, 3:30] = cap - 1
    for order in rr.ORDERS:
        want = rr.rle(ids, cap, 2000, order)
        assert want["nruns"][0, 1] > 1000
        got, _ = _launch(ops, ids, cap, 2000, order)
        _same(got, want, (cap, order))


@pytest.mark.parametrize("cap", [255, 300])
def test_more_runs_than_one_and_three_sort_chunks(ops, block, cap):
    P, R = block
    rs = np.random.RandomState(7 + cap)
    for H, W, least, most in ((37, R // 37 + 25, R, 2 * R), (61, 3 * R // 61 + 30, 3 * R, 4 * R)):
        ids = rs.randint(0, 303, (1, H, W)).astype(np.int32)
        for order in rr.ORDERS:
            want = rr.rle(ids, cap, H * W, order)
            assert least < want["nruns"][0, 0] < most, want["nruns"]
            got, _ = _launch(ops, ids, cap, H * W, order)
            _same(got, want, (H, W, cap, order))
            # and with the table cut inside the last chunk
            cut = int(want["nruns"][0, 0]) - 5
            got, _ = _launch(ops, ids, cap, cut, order)
            _same(got, rr.rle(ids, cap, cut, order), (H, W, cap, order, "cut"))


def test_truncation_keeps_the_runs_that_start_first(ops, block):
    rs = np.random.RandomState(13)
    H, W = 33, 45
    lab = rr.contents(H, W, rs)["noise 0.5"]
    ids, _, n = _components(ops, lab[None], 8)
    cap = int(n[0, 0]) + 1
    for order in rr.ORDERS:
        found = int(rr.rle(ids, cap, H * W, order)["nruns"][0, 1])
        assert found > 100
        for max_runs in (1, found - 1, found, found + 1):
            want = rr.rle(ids, cap, max_runs, order)
            kept = min(found, max_runs)
            assert want["nruns"].tolist() == [[kept, found]] and want["run_off"][0, -1] == kept
            got, _ = _launch(ops, ids, cap, max_runs, order)
            _same(got, want, (order, max_runs))                            # rows from kept on keep the sentinel
            assert (got["runs"][0, kept:] == -7).all() and got["nruns"].tolist() == [[kept, found]]


def test_lengths_sum_to_the_area_and_runs_span_the_box(ops, block):
    from diffews_amd.objects import runs_to_mask
    rs = np.random.RandomState(19)
    H, W = 41, 67
    for name in ("noise 0.5", "rings", "snake"):
        lab = rr.contents(H, W, rs)[name]
        ids, stats, n = _components(ops, lab[None], 8, cap=1024)
        top = int(n[0, 0])
        assert 0 < top <= 1024
        for order in rr.ORDERS:
            got, _ = _launch(ops, ids, 1024, H * W, order)
            assert got["nruns"][0, 0] == got["nruns"][0, 1]
            off = got["run_off"][0]
            for k in range(1, top + 1):
                rows = got["runs"][0, off[k - 1]:off[k]]
                _, area, y0, x0, y1, x1, _, _ = stats[0, k - 1].tolist()
                assert rows[:, 1].sum() == area, (name, order, k)
                ys, xs = np.nonzero(runs_to_mask(rows, H, W, order))
                assert (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1) == (y0, x0, y1, x1), (name, order, k)


def test_three_images_are_independent(ops, block):
    rs = np.random.RandomState(23)
    H, W = 39, 58
    c = rr.contents(H, W, rs)
    labs = np.stack([c["noise 0.5"], c["rings"], c["checkerboard"]])
    ids, _, _ = _components(ops, labs, 4)
    for order in rr.ORDERS:
        for cap, max_runs in ((2000, H * W), (5, 40)):
            got, _ = _launch(ops, ids, cap, max_runs, order)
            _same(got, rr.rle(ids, cap, max_runs, order), ("B = 3", order, cap))
            for b in range(3):
                one, _ = _launch(ops, ids[b:b + 1], cap, max_runs, order)
                kept = one["nruns"][0, 0]
                assert np.array_equal(one["nruns"][0], got["nruns"][b]) and np.array_equal(one["run_off"][0], got["run_off"][b])
                assert np.array_equal(one["runs"][0, :kept], got["runs"][b, :kept]), (order, b)


def test_poisoned_and_repeated_launches_give_the_same_bits(ops, block):
    """Outputs and workspace pre-filled with 0xFF and with 0x7B, two launches back to back into the same buffers, and the
    same buffers on another map: the reference's bits every time -- nothing is read before it is written, nothing
    accumulates across launches, and the rows behind kept still hold the fill."""
    P, R = block
    rs = np.random.RandomState(29)
    H, W = 67, 2 * P // 67 + 4
    c = rr.contents(H, W, rs)
    ids, _, _ = _components(ops, np.stack([c["noise 0.5"], c["snake"]]), 8)
    other, _, _ = _components(ops, np.stack([c["checkerboard"], c["rings"]]), 4)
    for order in rr.ORDERS:
        for cap, max_runs in ((700, H * W), (300, 1500)):
            want = rr.rle(ids, cap, max_runs, order)
            for fill in (0xFF, 0x7B):
                got, bufs = _launch(ops, ids, cap, max_runs, order, fill=fill)
                _same(got, want, (order, hex(fill)), rest=_word(fill))
            again, _ = _launch(ops, ids, cap, max_runs, order, bufs=bufs, repeat=2)
            _same(again, want, "back to back", rest=_word(0x7B))
            got, _ = _launch(ops, other, cap, max_runs, order, bufs=bufs)
            wo = rr.rle(other, cap, max_runs, order)
            for b, w in enumerate(wo["runs"]):                              # rows behind kept: the fill or the map before
                assert np.array_equal(got["runs"][b, :len(w)], w)
            assert np.array_equal(got["nruns"], wo["nruns"]) and np.array_equal(got["run_off"], wo["run_off"])


def test_captured_launch_follows_the_input_tensor(ops, hip_lib, block):
    """seg_components and seg_rle in one torch.cuda.graph: no memset node, and each replay encodes whatever the label
    tensor holds."""
    from diffews_amd.objects import ComponentBuffers, RunBuffers
    rs = np.random.RandomState(31)
    B, H, W, cap = 2, 41, 72, 600
    c = rr.contents(H, W, rs)
    maps = [np.stack([c["noise 0.5"], c["rings"]]), np.stack([c["snake"], c["noise 0.3"]]),
            np.stack([c["background"], c["vertical stripes"]])]
    buf = ComponentBuffers(B, H, W, cap)
    for order in rr.ORDERS:
        rb = RunBuffers(B, H, W, cap, max_runs=1000, order=order)
        lab = torch.zeros(B, H, W, dtype=torch.uint8, device="cuda")

        def call():
            ops.seg_components(lab, buf.ids, buf.n, buf.ws, stats=buf.stats, connectivity=8)
            ops.seg_rle(buf.ids, rb.runs, rb.run_off, rb.nruns, rb.ws, cap, order)
        call()                                                             # modules loaded before the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            call()
        nodes = C.c_int32()
        assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0
        assert nodes.value == 8 + 5 + (order == "column") + 3 * 2           # cap = 600: two digit passes
        graph.instantiate()
        for m in maps + maps[:1]:
            lab.copy_(torch.from_numpy(m))
            graph.replay()
            torch.cuda.synchronize()
            ids = buf.ids.cpu().numpy()
            want = rr.rle(ids, cap, 1000, order)
            got = dict(runs=rb.runs.cpu().numpy(), run_off=rb.run_off.cpu().numpy(), nruns=rb.nruns.cpu().numpy())
            for b, w in enumerate(want["runs"]):
                assert np.array_equal(got["runs"][b, :len(w)], w), (order, b)
            assert np.array_equal(got["nruns"], want["nruns"]) and np.array_equal(got["run_off"], want["run_off"])
            assert np.array_equal(ids > 0, m > 0)


# ------------------------------------------------------------------------------------------------ objects.py

def _check_host(per_image, ids, cap, max_runs, order):
    """runs_to_host's list of one image against the reference and back to masks."""
    from diffews_amd.objects import runs_to_coco, runs_to_mask
    H, W = ids.shape
    runs, off, (kept, found) = rr.rle_image(ids, cap, max_runs, order)
    n = min(int(ids.max()), cap)
    assert len(per_image) == n
    for k in range(1, n + 1):
        assert per_image[k - 1].dtype == np.int32 and np.array_equal(per_image[k - 1], rr.object_rows(runs, off, k)), (order, k)
        if kept == found:
            assert np.array_equal(runs_to_mask(per_image[k - 1], H, W, order), ids == k)
            if order == "column":
                coco = runs_to_coco(per_image[k - 1], H, W)
                assert coco["size"] == [H, W] and sum(coco["counts"]) == H * W and min(coco["counts"][1:]) > 0
                flat = np.repeat(np.arange(len(coco["counts"])) % 2, coco["counts"]).astype(bool)
                assert np.array_equal(flat.reshape(W, H).T, ids == k)
    return kept < found


def test_object_runs_on_a_list_of_native_size_views(hip_lib):
    """label_objects on two maps of different sizes cut out of one packed buffer, then object_runs on its result: one call
    per item, every value a list; runs_to_host / runs_to_coco / runs_to_mask against the reference; buffers reused and
    aliased; a wrong shape refused."""
    from diffews_amd.objects import RunBuffers, label_objects, object_runs, runs_to_coco, runs_to_host
    rs = np.random.RandomState(37)
    sizes = [(37, 53), (20, 64)]
    maps = [rr.contents(h, w, rs)["noise 0.5"] for h, w in sizes]
    packed = torch.full((3 + 37 * 53 + 20 * 64 + 5,), SENT, dtype=torch.uint8, device="cuda")
    views, off = [], 3
    for m in maps:
        v = packed[off:off + m.size].view(m.shape)
        v.copy_(torch.from_numpy(m))
        views.append(v)
        off += m.size
    o = label_objects(views, connectivity=4, max_components=512)
    for order in rr.ORDERS:
        r = object_runs(o, order=order)
        assert all(isinstance(r[k], list) and len(r[k]) == 2 for k in ("runs", "run_off", "nruns", "order", "shape"))
        assert r["order"] == [order] * 2 and r["shape"] == sizes
        host, truncated = runs_to_host(r)
        assert not truncated and len(host) == 2
        for i, (h, w) in enumerate(sizes):
            assert r["runs"][i].shape == (h * w, 2) and r["run_off"][i].shape == (513,) and r["nruns"][i].shape == (2,)
            assert not _check_host(host[i], o["ids"][i].cpu().numpy(), 512, h * w, order)
    with pytest.raises(ValueError):
        runs_to_coco(host[0][0], 37, 53, order="row")                      # COCO has no row order
    # a batch, a small table: truncated, and the lists hold what the reference keeps
    lab = torch.from_numpy(np.stack([rr.contents(9, 11, rs)[k] for k in ("checkerboard", "rings")])).cuda()
    o = label_objects(lab, connectivity=4, max_components=8)
    r = object_runs(o, order="column", max_runs=99)
    assert r["runs"].shape == (2, 99, 2) and r["run_off"].shape == (2, 9) and r["shape"] == (9, 11)
    host, truncated = runs_to_host(r)
    ids = o["ids"].cpu().numpy()
    assert not truncated and r["nruns"].tolist() == [[8, 8], [int(rr.rle_image(ids[1], 8, 99, "column")[2][1])] * 2]
    assert [_check_host(host[b], ids[b], 8, 99, "column") for b in range(2)] == [False, False]
    r = object_runs(o, order="row", max_runs=5)
    host, truncated = runs_to_host(r)
    assert truncated and r["nruns"][1].tolist()[0] == 5
    for b in range(2):
        runs, off_, (kept, found) = rr.rle_image(ids[b], 8, 5, "row")
        assert [h.tolist() for h in host[b]] == [rr.object_rows(runs, off_, k).tolist() for k in range(1, len(host[b]) + 1)]
        assert sum(len(h) for h in host[b]) == kept
    # one [H, W] map: no batch axis; an id tensor with max_components; caller-owned buffers reused and aliased
    one = object_runs(o["ids"][1], max_components=8, order="row")
    assert one["runs"].dim() == 2 and one["nruns"].shape == (2,)
    h1, t1 = runs_to_host(one)
    assert not t1 and not _check_host(h1, ids[1], 8, 99, "row")
    rb = RunBuffers(2, 9, 11, max_components=8, max_runs=99, order="column")
    for _ in range(2):
        r = object_runs(o, buffers=rb)
        assert r["runs"].data_ptr() == rb.runs.data_ptr() and r["run_off"].data_ptr() == rb.run_off.data_ptr()
        host, truncated = runs_to_host(r)
        assert not truncated and not _check_host(host[1], ids[1], 8, 99, "column")
    with pytest.raises(ValueError):
        object_runs(o, order="row", buffers=rb)                            # made for the other order
    with pytest.raises(ValueError):
        object_runs(o["ids"][:1], max_components=8, buffers=rb)           # made for another shape
    with pytest.raises(ValueError):
        object_runs(o["ids"], buffers=rb)                                  # an id tensor without max_components
    with pytest.raises(ValueError):
        object_runs(o, order="diagonal")
    with pytest.raises(ValueError):
        object_runs(o["ids"].float(), max_components=8)
    assert (packed[:3] == SENT).all() and (packed[off:] == SENT).all()


# ------------------------------------------------------------------------------------------------ the routes, tiny engine

@pytest.fixture(scope="module")
def pipe(hip_lib):
    """The tiny-config engine of tests/test_support_bank_gpu.py (bf16), without its oracle."""
    from diffews_amd import config, weights
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise
    from diffews_amd.scheduler import DDIMSchedulerCustomized
    from diffews_amd.unet import MyUNet2DConditionModel
    from diffews_amd.vae import AutoencoderKL
    dt = torch.bfloat16
    kw = lambda cfg: {k: v for k, v in cfg.items() if not k.startswith("_")}  # noqa: E731
    ucfg, vcfg = config.get("tiny_unet"), config.get("tiny_vae")
    unet = MyUNet2DConditionModel(ucfg, weights.synthetic_unet_state_dict(ucfg, round_to=dt), torch_dtype=dt)
    vae = AutoencoderKL(vcfg, weights.synthetic_vae_state_dict(vcfg, round_to=dt), torch_dtype=dt)
    te = weights.synthetic_text_embed(ucfg).to(dt).float()
    return MarigoldPipelineRGBLatentNoise(unet, vae, DDIMSchedulerCustomized(**kw(config.get("scheduler"))), text_embeds=te)


def test_pipe_object_runs_on_the_n_way_route(pipe):
    """pipe.object_runs(pipe.objects(r)) on segment_classes' result (b = 2): the reference run on the ids the route
    returned, both orders."""
    from diffews_amd.objects import runs_to_host
    from test_support_bank_gpu import _queries, _support_set
    sets = [_support_set(s, 64, seed=910 + 10 * c) for c, s in enumerate((1, 3, 2))]
    library = pipe.prepare_support_classes([a.cuda() for a, _ in sets], [m.cuda() for _, m in sets])
    r = pipe.segment_classes(library, _queries(2, 64, 77).cuda(), captured=False)
    o = pipe.objects(r, connectivity=8, max_components=256)
    ids = o["ids"].cpu().numpy()
    assert ids.shape == (2, 64, 64)
    for order in rr.ORDERS:
        rl = pipe.object_runs(o, order=order)
        assert rl["order"] == order and rl["shape"] == (64, 64) and rl["run_off"].shape == (2, 257)
        want = rr.rle(ids, 256, 64 * 64, order)
        got = {k: rl[k].cpu().numpy() for k in ("runs", "run_off", "nruns")}
        for b, w in enumerate(want["runs"]):
            assert np.array_equal(got["runs"][b, :len(w)], w), (order, b)
        assert np.array_equal(got["nruns"], want["nruns"]) and np.array_equal(got["run_off"], want["run_off"])
        host, truncated = runs_to_host(rl)
        assert not truncated
        for b in range(2):
            _check_host(host[b], ids[b], 256, 64 * 64, order)
