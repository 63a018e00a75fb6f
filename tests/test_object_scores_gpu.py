"""GPU tests of the score stage: ops.seg_scores against tests/scores_ref.py on ids that ops.seg_components made (4 and 8
neighbours) at the smallest shapes that reach every path of the kernel -- one pixel, one row, one column, exactly a block,
a block plus one, three blocks with an odd width (the scalar path), a width that is a multiple of four over more than two
blocks (the vector path) -- then extreme values, the plane table (entries left out, labels and ids out of range, entry-major
planes, a device table overwritten behind the validation), batches, guards, poisoned and repeated launches, a captured launch
behind seg_components, objects.object_scores / scores_to_host, pipe.object_scores on the routes of the tiny engine, and the
device chain objects -> scores -> match -> detections_to_host -> average_precision against the host references.  All
integers: every comparison is exact.

Every buffer sits inside sentinel guards.  Half of the cases put ids 61 WORDS into their allocation (off the 16-byte
alignment of the vector loads) and the workspace 60 bytes (a 4- but not 8-byte aligned workspace, whose 64-bit accumulators
start at the next boundary); a third put labels and planes 3 BYTES into theirs, which takes the byte loads."""
import ctypes as C

import numpy as np
import pytest
import torch

import match_ref as mr
import rle_ref as rr
import scores_ref as sr

pytestmark = pytest.mark.gpu

SENT = 0xA5


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def P(ops):
    return ops.seg_scores_block()


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


def _three(lab):
    """The contents of rle_ref carry bytes up to 7: folded into the classes 1..3 of the N = 3 planes."""
    return np.where(lab > 0, 1 + (lab.astype(np.int32) - 1) % 3, 0).astype(np.uint8)


def _components(ops, labels, conn):
    """ids and n of ops.seg_components on numpy uint8 [B, H, W] (no filter: the filtered map is the input)."""
    lab = torch.from_numpy(labels).cuda()
    B, H, W = lab.shape
    ids = torch.empty(B, H, W, dtype=torch.int32, device="cuda")
    n = torch.empty(B, 2, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.seg_components_workspace(B, H, W), dtype=torch.uint8, device="cuda")
    ops.seg_components(lab, ids, n, ws, connectivity=conn)
    return ids.cpu().numpy(), n.cpu().numpy()


def _class_table(N, B):
    return np.array([[-1] + [c * B + b for c in range(N)] for b in range(B)], np.int32)


def _launch(ops, ids, labels, u8, table, cap, id_pad=4, byte_pad=64, ws_pad=64, fill=None, bufs=None, repeat=1, device_table=None):
    """ops.seg_scores on numpy inputs in guarded buffers, optionally pre-filled with a byte; returns the numpy scores after
    checking every guard and that no input changed, and the buffers.  device_table: what the device copy of the table holds
    when it differs from the validated host mirror."""
    B, H, W = ids.shape
    if bufs is None:
        bufs = dict(ids=_Guarded((B, H, W), torch.int32, id_pad), labels=_Guarded((B, H, W), torch.uint8, byte_pad),
                    u8=_Guarded(u8.shape, torch.uint8, byte_pad), planes=_Guarded(table.shape, torch.int32, 4),
                    scores=_Guarded((B, cap, 4), torch.int64, 4, fill),
                    ws=_Guarded((ops.seg_scores_workspace(B, cap),), torch.uint8, ws_pad, fill))
    dev = table if device_table is None else device_table
    for k, v in (("ids", ids), ("labels", labels), ("u8", u8), ("planes", dev)):
        bufs[k].t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    g = {k: v.t for k, v in bufs.items()}
    host = torch.from_numpy(np.ascontiguousarray(table))
    for _ in range(repeat):
        ops.seg_scores(g["ids"], g["labels"], g["u8"].view(-1, 3, H, W), g["planes"], host, g["scores"], g["ws"])
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert np.array_equal(g["ids"].cpu().numpy(), ids) and np.array_equal(g["labels"].cpu().numpy(), labels)
    assert np.array_equal(g["u8"].cpu().numpy(), u8) and np.array_equal(g["planes"].cpu().numpy(), dev), "an input was modified"
    return g["scores"].cpu().numpy(), bufs


def _shapes(P):
    assert P % 64 == 0 and (P + 1) % 3 == 0
    return [(1, 1), (1, 37), (37, 1), (5, 7), (P // 64, 64), (3, (P + 1) // 3), (75, 3 * P // 75 + 2), (70, 60)]


@pytest.mark.parametrize("which", range(8), ids=["1x1", "1x37", "37x1", "5x7", "block", "block+1", "3-blocks-odd-W", "W%4==0"])
def test_equals_the_reference(ops, P, which):
    """Every content, ids of both connectivities, cap = 1 / 16 / above every id, B = 1, random plane bytes, N = 3
    class-major planes."""
    H, W = _shapes(P)[which]
    if which == 4:
        assert H * W == P
    if which == 5:
        assert H * W == P + 1 and W % 2 == 1
    if which == 6:
        assert 3 * P < H * W < 4 * P and W % 2 == 1
    if which == 7:
        assert W % 4 == 0 and H * W > 2 * P and H * W % 8 == 0
    rs = np.random.RandomState(1000 * H + W)
    u8 = rs.randint(0, 256, (3, 1, 3, H, W)).astype(np.uint8)
    table = _class_table(3, 1)
    case = 0
    for name, lab in rr.contents(H, W, rs).items():
        lab = _three(lab)[None]
        for conn in (4, 8):
            ids, n = _components(ops, lab, conn)
            top = int(ids.max())
            assert top == n[0, 0]
            for cap in (1, 16, top + 3):
                want = sr.scores(ids, lab, u8.reshape(-1, 3, H, W), table, cap)
                got, _ = _launch(ops, ids, lab, u8, table, cap, id_pad=61 if conn == 8 else 4,
                                 byte_pad=3 if case % 3 == 0 else 64, ws_pad=60 if conn == 8 else 64)
                case += 1
                assert np.array_equal(got, want), (name, H, W, conn, cap, int((got != want).sum()))
                if name == "background":
                    assert not got.any()
                if name == "one object":                                   # one run across every block: label 7 -> class 1
                    s = u8[0, 0].astype(np.int64).sum(0)
                    assert got[0, 0].tolist() == [int(s.sum()), H * W, int(s.min()), int(s.max())] and not got[0, 1:].any()
                if name == "checkerboard" and conn == 4 and cap > top:     # a run per pixel
                    assert (got[0, :top, 1] == 1).all() and (got[0, :top, 2] == got[0, :top, 3]).all()


def test_extreme_values(ops, P):
    """One component of 2P + 5 pixels -- three blocks, all four waves of the first two -- with every plane byte 255: the sum
    is 765 n exactly and min == max == 765; one pixel of 0 in the last block brings min to 0; a 1-pixel object behind it
    keeps its own row."""
    W = 2 * P + 5
    table = _class_table(3, 1)
    lab = np.ones((1, 1, W), np.uint8)
    ids, n = _components(ops, lab, 8)
    assert n[0, 0] == 1
    u8 = np.full((3, 1, 3, 1, W), 255, np.uint8)
    got, _ = _launch(ops, ids, lab, u8, table, 4)
    assert got[0].tolist() == [[765 * W, W, 765, 765], [0] * 4, [0] * 4, [0] * 4]
    u8[0, 0, :, 0, W - 2] = 0
    got, _ = _launch(ops, ids, lab, u8, table, 4, id_pad=61, byte_pad=3)
    assert got[0].tolist() == [[765 * (W - 1), W, 0, 765], [0] * 4, [0] * 4, [0] * 4]
    lab = np.concatenate([lab, np.full((1, 1, 1), 2, np.uint8)], 2)
    ids, n = _components(ops, lab, 8)
    assert n[0, 0] == 2 and ids[0, 0, -1] == 2
    u8 = np.concatenate([u8, np.full((3, 1, 3, 1, 1), 255, np.uint8)], 4)
    u8[1, 0, :, 0, W] = (1, 2, 3)
    got, _ = _launch(ops, ids, lab, u8, table, 4)
    assert got[0].tolist() == [[765 * (W - 1), W, 0, 765], [6, 1, 6, 6], [0] * 4, [0] * 4]
    assert np.array_equal(got, sr.scores(ids, lab, u8.reshape(-1, 3, 1, W + 1), table, 4))


def test_the_plane_table_decides_what_is_counted(ops, P):
    rs = np.random.RandomState(43)
    H, W, cap = 33, 2 * P // 33 + 7, 40
    lab = rs.randint(0, 5, (2, H, W)).astype(np.uint8)                     # label 4 is above nlabels = 3
    lab[rs.rand(2, H, W) < 0.02] = 255
    blob = mr.blobs(H, W, rs)
    lab[0] = np.where(rs.rand(H, W) < 0.7, blob, lab[0])                   # some larger objects among the noise
    ids, n = _components(ops, lab, 8)
    assert n.min() > cap                                                    # ids above cap exist
    ids[:, 0, :9] = -4
    ids[:, 1, :9] = 0
    ids[:, 2, :9] = cap + 1
    ids[:, 3, :9] = cap
    # whole labels left out, per image: image 0 has no planes for label 2, image 1 none for labels 1 and 3
    u8 = rs.randint(0, 256, (5, 3, H, W)).astype(np.uint8)
    table = np.array([[9, 4, -1, 0], [9, -1, 2, -1]], np.int32)
    want = sr.scores(ids, lab, u8, table, cap)
    got, _ = _launch(ops, ids, lab, u8, table, cap, id_pad=61, byte_pad=3)
    assert np.array_equal(got, want)
    area = np.stack([np.bincount(ids[b][(ids[b] >= 1) & (ids[b] <= cap)], minlength=cap + 1)[1:] for b in range(2)])
    assert (got[..., 1] <= area).all() and (got[..., 1] < area).any() and got[..., 1].any()
    # entry-major planes, B = 2, another candidate list per image: [(2, 0), (1,)] -> entries (0: q0 c0, 1: q0 c2, 2: q1 c1)
    from diffews_amd.objects import planes_for_candidates
    table = planes_for_candidates([(2, 0), (1,)], 3).numpy()
    assert table.tolist() == [[-1, 0, -1, 1], [-1, -1, 2, -1]]
    u8 = rs.randint(0, 256, (3, 3, H, W)).astype(np.uint8)
    got, _ = _launch(ops, ids, lab, u8, table, cap)
    assert np.array_equal(got, sr.scores(ids, lab, u8, table, cap)) and got[0, :, 1].any() and got[1, :, 1].any()
    # the device table overwritten behind the validation: the kernel clamps what it reads, those labels are not counted
    bad = np.array([[7, 3, -5, 1], [7, 1 << 30, 2, -(1 << 31)]], np.int32)
    want = sr.scores(ids, lab, u8, bad, cap)
    got, _ = _launch(ops, ids, lab, u8, table, cap, id_pad=61, byte_pad=3, device_table=bad)
    assert np.array_equal(got, want) and got[..., 1].any()
    assert np.array_equal(want, sr.scores(ids, lab, u8, np.array([[-1, -1, -1, 1], [-1, -1, 2, -1]]), cap))


def test_three_images_are_independent(ops, P):
    rs = np.random.RandomState(23)
    H, W = 39, P // 39 + 30
    c = rr.contents(H, W, rs)
    labs = np.stack([_three(c[k]) for k in ("noise 0.5", "rings", "checkerboard")])
    ids, _ = _components(ops, labs, 4)
    u8 = rs.randint(0, 256, (3, 3, 3, H, W)).astype(np.uint8)
    table = _class_table(3, 3)
    for cap in (2000, 5):
        got, _ = _launch(ops, ids, labs, u8, table, cap)
        assert np.array_equal(got, sr.scores(ids, labs, u8.reshape(-1, 3, H, W), table, cap))
        for b in range(3):
            one, _ = _launch(ops, ids[b:b + 1], labs[b:b + 1], u8, table[b:b + 1], cap)
            assert np.array_equal(one[0], got[b]), (cap, b)


def test_poisoned_and_repeated_launches_give_the_same_bits(ops, P):
    """Outputs and workspace pre-filled with 0xFF and with 0x7B, two launches back to back into the same buffers, and the
    same buffers on another map: the reference's bits every time -- nothing is read before it is written and nothing
    accumulates across launches."""
    rs = np.random.RandomState(29)
    H, W = 67, 2 * P // 67 + 4
    c = rr.contents(H, W, rs)
    labs = np.stack([_three(c["noise 0.5"]), _three(c["snake"])])
    other = np.stack([_three(c["one object"]), _three(c["rings"])])
    ids, _ = _components(ops, labs, 8)
    oids, _ = _components(ops, other, 4)
    u8 = rs.randint(0, 256, (3, 2, 3, H, W)).astype(np.uint8)
    flat, table = u8.reshape(-1, 3, H, W), _class_table(3, 2)
    for cap in (700, 3):
        want = sr.scores(ids, labs, flat, table, cap)
        for fill in (0xFF, 0x7B):
            got, bufs = _launch(ops, ids, labs, u8, table, cap, ws_pad=60, fill=fill)
            assert np.array_equal(got, want), (cap, hex(fill))
        again, _ = _launch(ops, ids, labs, u8, table, cap, bufs=bufs, repeat=2)
        assert np.array_equal(again, want), "back to back"
        got, _ = _launch(ops, oids, other, u8, table, cap, bufs=bufs)
        assert np.array_equal(got, sr.scores(oids, other, flat, table, cap)), "the same buffers on another map"


def test_captured_launch_follows_the_labels_and_the_table(ops, hip_lib):
    """seg_components and seg_scores in one torch.cuda.graph: no memset node, 8 + 3 kernel nodes, and each replay scores
    whatever the label tensor AND the device plane table hold."""
    from diffews_amd.objects import ComponentBuffers, ScoreBuffers
    rs = np.random.RandomState(31)
    B, H, W, cap = 2, 41, 72, 600
    c = rr.contents(H, W, rs)
    maps = [np.stack([_three(c[a]), _three(c[b])]) for a, b in (("noise 0.5", "rings"), ("snake", "noise 0.3"),
                                                                 ("background", "vertical stripes"))]
    tables = [_class_table(3, 2), np.array([[-1, 5, -1, 0], [-1, 2, 2, 4]], np.int32), _class_table(3, 2)]
    u8 = rs.randint(0, 256, (6, 3, H, W)).astype(np.uint8)
    buf, sb = ComponentBuffers(B, H, W, cap), ScoreBuffers(B, cap, 3)
    lab = torch.zeros(B, H, W, dtype=torch.uint8, device="cuda")
    planes = torch.from_numpy(u8).cuda()
    host = torch.from_numpy(_class_table(3, 2))                            # what the captured call validated
    sb.planes.copy_(host)

    def call():
        ops.seg_components(lab, buf.ids, buf.n, buf.ws, stats=buf.stats, connectivity=8)
        ops.seg_scores(buf.ids, lab, planes, sb.planes, host, sb.scores, sb.ws)
    call()                                                                 # modules loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    nodes = C.c_int32()
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0
    assert nodes.value == 8 + 3
    graph.instantiate()
    for m, t in list(zip(maps, tables)) + [(maps[0], tables[1])]:
        lab.copy_(torch.from_numpy(m))
        sb.planes.copy_(torch.from_numpy(t))
        graph.replay()
        torch.cuda.synchronize()
        ids = buf.ids.cpu().numpy()
        assert np.array_equal(ids > 0, m > 0)
        assert np.array_equal(sb.scores.cpu().numpy(), sr.scores(ids, m, u8, t, cap))


# ------------------------------------------------------------------------------------------------ objects.py

def test_object_scores_on_a_list_of_native_size_views(hip_lib):
    """label_objects on two maps of different sizes cut out of one packed buffer, object_scores on its result with planes
    cut out of another: one call per item, every value a list; scores_to_host against the reference; buffers reused and
    aliased; a wrong shape, dtype or table size refused."""
    from diffews_amd.objects import (ScoreBuffers, label_objects, object_scores, planes_for_binary, planes_for_classes,
                                     scores_to_host)
    rs = np.random.RandomState(37)
    sizes = [(37, 53), (20, 64)]
    maps = [rr.contents(h, w, rs)["noise 0.5"] for h, w in sizes]
    u8s = [rs.randint(0, 256, (3, 3, h, w)).astype(np.uint8) for h, w in sizes]
    packed = torch.full((3 + 37 * 53 + 20 * 64 + 5,), SENT, dtype=torch.uint8, device="cuda")
    pu8 = torch.full((5 + 9 * (37 * 53 + 20 * 64) + 3,), SENT, dtype=torch.uint8, device="cuda")
    views, segs, off, uoff = [], [], 3, 5
    for m, u in zip(maps, u8s):
        v = packed[off:off + m.size].view(m.shape)
        v.copy_(torch.from_numpy(m))
        views.append(v)
        off += m.size
        s = pu8[uoff:uoff + u.size].view(u.shape)
        s.copy_(torch.from_numpy(u))
        segs.append(s)
        uoff += u.size
    o = label_objects(views, connectivity=4, max_components=2048)
    table = planes_for_classes(3, 1)
    r = object_scores(o, segs, table)
    assert all(isinstance(r[k], list) and len(r[k]) == 2 for k in ("scores", "planes"))
    host = scores_to_host(r)
    for i, (h, w) in enumerate(sizes):
        assert r["scores"][i].shape == (2048, 4) and r["scores"][i].dtype == torch.int64 and r["planes"][i].tolist() == table[0].tolist()
        ids, lab = o["ids"][i].cpu().numpy(), o["labels"][i].cpu().numpy()
        want = sr.scores_image(ids, lab, u8s[i], table[0].numpy(), 2048)
        assert want[:, 1].sum() == (maps[i] > 0).sum()
        for k, col in enumerate(("sum", "n", "min", "max")):
            assert host[i][col].dtype == np.int64 and np.array_equal(host[i][col], want[:, k]), (i, col)
        assert host[i]["mean"].dtype == np.float64
        assert host[i]["mean"].tolist() == [sr.mean(int(t), int(n)) for t, n in zip(want[:, 0], want[:, 1])]
    # a table per item
    r2 = object_scores(o, segs, [table, [[-1, 1, -1, 0]]])
    want = sr.scores_image(o["ids"][1].cpu().numpy(), o["labels"][1].cpu().numpy(), u8s[1], [-1, 1, -1, 0], 2048)
    assert np.array_equal(r2["scores"][1].cpu().numpy(), want) and torch.equal(r2["scores"][0], r["scores"][0])
    # a batch; caller-owned buffers reused and aliased; one [H, W] map has no batch axis
    lab = torch.from_numpy(np.stack([rr.contents(9, 11, rs)[k] for k in ("noise 0.5", "rings")])).cuda()
    u8 = rs.randint(0, 256, (3, 2, 3, 9, 11)).astype(np.uint8)
    seg = torch.from_numpy(u8).cuda()
    o = label_objects(lab, connectivity=4, max_components=8)
    ids, flt = o["ids"].cpu().numpy(), o["labels"].cpu().numpy()
    want = sr.scores(ids, flt, u8.reshape(-1, 3, 9, 11), planes_for_classes(3, 2).numpy(), 8)
    sb = ScoreBuffers(2, 8, 3)
    for _ in range(2):
        r = object_scores(o, seg, planes_for_classes(3, 2), buffers=sb)
        assert r["scores"].data_ptr() == sb.scores.data_ptr() and r["planes"].data_ptr() == sb.planes.data_ptr()
        assert np.array_equal(r["scores"].cpu().numpy(), want) and sb.planes_host.is_pinned()
    r = object_scores(o, seg, planes_for_classes(3, 2).tolist())            # a nested list, fresh buffers
    assert np.array_equal(r["scores"].cpu().numpy(), want)
    one = {k: o[k][1] for k in ("ids", "labels", "stats")}
    r1 = object_scores(one, seg[:, 1].contiguous(), planes_for_classes(3, 1))
    assert r1["scores"].shape == (8, 4) and r1["planes"].shape == (4,) and np.array_equal(r1["scores"].cpu().numpy(), want[1])
    h1 = scores_to_host(r1)
    assert h1["sum"].shape == (8,) and np.array_equal(h1["n"], want[1][:, 1])
    for bad in (lambda: object_scores(o, seg, planes_for_classes(3, 1)),            # one row for two images
                lambda: object_scores(o, seg, planes_for_binary(2), buffers=sb),    # buffers made for three labels
                lambda: object_scores(o, seg[:, :, :, :8], planes_for_classes(3, 2)),   # another size, and not contiguous
                lambda: object_scores(o, seg.int(), planes_for_classes(3, 2)),
                lambda: object_scores(o, seg, planes_for_classes(3, 2).cuda()),     # the table is a host table
                lambda: object_scores(o, seg, planes_for_classes(3, 2).float()),
                lambda: object_scores(dict(o, labels=o["labels"].int()), seg, planes_for_classes(3, 2)),
                lambda: object_scores(o, seg, torch.full((2, 4), 6, dtype=torch.int32)),   # group 6 of 6: the library refuses
                lambda: object_scores({k: [v] for k, v in o.items()}, seg, planes_for_classes(3, 2))):   # a list needs a list
        with pytest.raises((ValueError, RuntimeError)):
            bad()
    assert (packed[:3] == SENT).all() and (packed[off:] == SENT).all() and (pu8[:5] == SENT).all() and (pu8[uoff:] == SENT).all()


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


@pytest.fixture(scope="module")
def library(pipe):
    from test_support_bank_gpu import _support_set
    sets = [_support_set(s, 64, seed=910 + 10 * c) for c, s in enumerate((1, 3, 2))]
    return pipe.prepare_support_classes([a.cuda() for a, _ in sets], [m.cuda() for _, m in sets])


CAP = 4096      # above every id a 64 x 64 or 96 x 80 map can hold after the 8-neighbour labelling of random labels


def _route(pipe, r, key, seg_u8, table, N, seed, every=True, **kw):
    """pipe.object_scores on the route's own objects, and on a seeded random label map (labels 0..N) put in the place of
    the route's map, both against the reference on the route's own planes through `table`."""
    from diffews_amd.objects import label_objects
    flat = seg_u8.cpu().numpy()
    flat = flat.reshape(-1, *flat.shape[-3:])
    o = pipe.objects(r, key=key, connectivity=8, max_components=CAP)
    rs = np.random.RandomState(seed)
    shape = tuple(o["labels"].shape)
    rnd = torch.from_numpy(((rs.rand(*shape) < 0.6) * rs.randint(1, N + 1, shape)).astype(np.uint8)).cuda()
    for oo in (o, label_objects(rnd, connectivity=8, max_components=CAP)):
        s = pipe.object_scores(r, oo, key=key, **kw)
        ids, lab = oo["ids"].cpu().numpy(), oo["labels"].cpu().numpy()
        if ids.ndim == 2:
            want = sr.scores_image(ids, lab, flat, table[0], CAP)
        else:
            want = sr.scores(ids, lab, flat, table, CAP)
        assert s["scores"].shape == want.shape and np.array_equal(s["scores"].cpu().numpy(), want)
        assert s["planes"].cpu().numpy().reshape(table.shape).tolist() == table.tolist()
    counted, labelled = int(want[..., 1].sum()), int((rnd > 0).sum())
    assert counted == labelled if every else 0 < counted < labelled         # of the random map; a table with gaps counts less
    return o


def test_pipe_object_scores_on_the_n_way_route(pipe, library):
    from test_support_bank_gpu import _queries
    r = pipe.segment_classes(library, _queries(2, 64, 77).cuda(), captured=False)
    assert r["seg_u8"].shape == (3, 2, 3, 64, 64)
    _route(pipe, r, "labels", r["seg_u8"], _class_table(3, 2), 3, 51)


def test_pipe_object_scores_on_the_candidate_route(pipe, library):
    from test_support_bank_gpu import _queries
    cands = [(2, 0), (1,)]
    r = pipe.segment_candidates(library, _queries(2, 64, 78).cuda(), cands, captured=False)
    assert r["seg_u8"].shape == (3, 3, 64, 64) and r["entries"] == [(0, 0), (0, 2), (1, 1)]
    table = np.array([[-1, 0, -1, 1], [-1, -1, 2, -1]], np.int32)
    o = _route(pipe, r, "labels", r["seg_u8"], table, 3, 52, every=False, candidates=cands)
    with pytest.raises(ValueError, match="candidates"):
        pipe.object_scores(r, o)


def test_pipe_object_scores_on_the_binary_native_route(pipe):
    """segment_queries with NativeTargets: objects of key="pred", a list of native-size maps, scored on the native planes."""
    from diffews_amd.input_pipeline import NativeTargets
    from diffews_amd.objects import label_objects
    from test_support_bank_gpu import _queries, _support_set
    sup, msk = _support_set(2, 64, seed=930)
    bank = pipe.prepare_support(sup.cuda(), msk.cuda())
    sizes = [(50, 70), (33, 41)]
    r = pipe.segment_queries(bank, _queries(2, 64, 79).cuda(), native=NativeTargets((64, 64), sizes), captured=False)
    planes = [p.cpu().numpy() for p in r["native"]["seg_u8"]]
    assert [p.shape for p in planes] == [(3, h, w) for h, w in sizes]
    o = pipe.objects(r, key="pred", connectivity=8, max_components=1024)
    rs = np.random.RandomState(53)
    rnd = [torch.from_numpy((rs.rand(h, w) < 0.6).astype(np.uint8)).cuda() for h, w in sizes]
    for oo in (o, label_objects(rnd, connectivity=8, max_components=1024)):
        s = pipe.object_scores(r, oo, key="pred")
        assert isinstance(s["scores"], list) and len(s["scores"]) == 2
        for i in range(2):
            want = sr.scores_image(oo["ids"][i].cpu().numpy(), oo["labels"][i].cpu().numpy(), planes[i][None], [-1, 0], 1024)
            assert np.array_equal(s["scores"][i].cpu().numpy(), want), i
    assert want[:, 1].sum() == int(rnd[1].sum())
    with pytest.raises(KeyError):
        pipe.object_scores(r, o, key="labels")


def test_pipe_object_scores_on_the_dense_tiled_route(pipe, library):
    rs = np.random.RandomState(54)
    img = rs.randint(0, 256, (96, 80, 3)).astype(np.uint8)
    r = pipe.segment_tiled(library, img, batch=3, captured=False)
    assert r["seg_u8"].shape == (3, 3, 96, 80) and r["labels"].shape == (96, 80)
    _route(pipe, r, "labels", r["seg_u8"], _class_table(3, 1), 3, 55)


def test_routes_without_planes_at_the_label_maps_size_are_refused(pipe):
    """The N-way / candidate native routes and tiled-with-candidates keep no planes at their label map's size: their
    results' shapes are enough to tell, so the results are made by hand here."""
    z = torch.zeros(8, 8, dtype=torch.uint8, device="cuda")
    o = dict(ids=[z.int()], labels=[z], stats=[torch.zeros(4, 8, dtype=torch.int32, device="cuda")])
    nway_native = dict(seg_u8=torch.zeros(3, 1, 3, 16, 16, dtype=torch.uint8, device="cuda"), labels=z[None],
                       native=dict(labels=[z], counts=None, mx=None, seg_u8=None, sizes=[(8, 8)]))
    with pytest.raises(ValueError, match="native"):
        pipe.object_scores(nway_native, o)
    cand_native = dict(nway_native, entries=[(0, 0)], offsets=[0, 1])
    with pytest.raises(ValueError, match="native"):
        pipe.object_scores(cand_native, o, candidates=[(0,)])
    tiled_cand = dict(labels=z, mx=None, plan=object(), counts=None)
    with pytest.raises(ValueError, match="merged"):
        pipe.object_scores(tiled_cand, {k: v[0] for k, v in o.items()})


# ------------------------------------------------------------------------------------------------ end to end

def test_detections_and_average_precision_end_to_end(hip_lib):
    """One 41 x 67 "noise 0.5" map as prediction, a copy shifted by two columns as ground truth, random planes: objects ->
    scores -> match -> detections_to_host -> average_precision on the device chain equals scores_ref + match_ref + the loop
    AP on the host, bit for bit (both sides divide the same integers)."""
    from diffews_amd.metrics import average_precision
    from diffews_amd.objects import (coco_results, detections_to_host, label_objects, match_objects, object_runs, object_scores,
                                     objects_to_host, planes_for_classes, runs_to_host, scores_to_host)
    rs = np.random.RandomState(61)
    H, W, N, cap = 41, 67, 3, 1024
    pred = rr.contents(H, W, rs)["noise 0.5"]
    gt = np.roll(pred, 2, 1)
    u8 = rs.randint(0, 256, (N, 1, 3, H, W)).astype(np.uint8)
    o = label_objects(torch.from_numpy(pred).cuda(), connectivity=8, max_components=cap)
    og = label_objects(torch.from_numpy(gt).cuda(), connectivity=8, max_components=cap)
    s = object_scores(o, torch.from_numpy(u8).cuda(), planes_for_classes(N, 1))
    m = match_objects(o, og, nlabels=N, iou=(1, 2))
    dets, npos = detections_to_host(o, s, m)
    got = average_precision([dets], npos)
    # the host side
    ids, gids = o["ids"].cpu().numpy(), og["ids"].cpu().numpy()
    stats, gstats = o["stats"].cpu().numpy(), og["stats"].cpu().numpy()
    n = int(o["n"][0])
    assert 20 < n <= cap
    sc = sr.scores_image(ids, pred, u8.reshape(-1, 3, H, W), [-1, 0, 1, 2], cap)
    mm = mr.match_image(ids, gids, cap, cap, N, H * W, H * W, stats, gstats)
    rows = []
    for p in range(1, n + 1):
        if sc[p - 1, 1] > 0 and mm["area"][p] > 0:
            g, inter, union = mm["match"][p - 1].tolist()
            rows.append([int(stats[p - 1, 0]), int(sc[p - 1, 0]), int(sc[p - 1, 1]), inter if g else 0, union if g else 0])
    assert dets.dtype == np.int64 and dets.tolist() == rows and len(rows) == n
    want_npos = (mm["pq"][:, 0] + mm["pq"][:, 2]).tolist()
    assert npos.tolist() == want_npos and sum(want_npos) == int(og["n"][0])
    assert any(r[3] for r in rows) and any(not r[3] for r in rows)        # partners and none
    thr = got["thresholds"]
    assert thr == tuple((k, 20) for k in range(10, 20))
    want = sr.loop_ap(rows, want_npos, thr)
    for c in range(N + 1):
        if want[c] is None:
            assert np.isnan(got["ap"][c]).all()
        else:
            assert got["ap"][c].tolist() == want[c], c
    assert got["map"] == sr.loop_map(want) and 0.0 < got["map"] < 1.0
    # and the COCO records of the same image from the three host tables
    o_host, _ = objects_to_host(o)
    runs_host, truncated = runs_to_host(object_runs(o))
    assert not truncated
    recs = coco_results(o_host, runs_host, scores_to_host(s), 5, [11, 22, 33], H, W)
    assert len(recs) == n
    for p, rec in enumerate(recs, 1):
        ys, xs = np.nonzero(ids == p)
        assert rec["bbox"] == [xs.min(), ys.min(), xs.max() + 1 - xs.min(), ys.max() + 1 - ys.min()] and rec["area"] == len(ys)
        assert rec["category_id"] == 11 * int(stats[p - 1, 0]) and sum(rec["segmentation"]["counts"]) == H * W
        assert rec["score"] == sr.mean(int(sc[p - 1, 0]), int(sc[p - 1, 1]))
