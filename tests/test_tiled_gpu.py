"""GPU tests of tiled segmentation: ops.tiles_merge against the host reference (tests/tiles_ref.py) on random bytes at the
smallest shapes that reach every path of the kernel (one window, two windows overlapping by 7, widths that are no multiple
of 4 with origins that are not 4-aligned, a non-square tile, misaligned buffers), ops.tiles_cut against
DeviceImageTransform and numpy, cut -> merge round trip, and pipe.segment_tiled / evaluate.evaluate_tiled on the tiny
engine against the routed calls merged by the reference.  Every comparison is exact (integers, bit-equal floats)."""
import numpy as np
import pytest
import torch

import nway_ref
import tiles_ref as tr
from test_support_bank_gpu import models, _support_set  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

# (tile, image, overlap): origins of 64 x 64 on 88 x 150 are ys [0, 24], xs [0, 43, 86]; on 64 x 193 xs [0, 43, 86, 129]
MERGE_CASES = [((8, 8), (8, 8), 2), ((8, 8), (8, 9), 2), ((8, 8), (13, 29), 2), ((8, 8), (23, 8), 2), ((8, 16), (19, 37), 3),
               ((64, 64), (88, 150), 8), ((64, 64), (64, 193), 8)]
IDS = [f"{t[0]}x{t[1]}-on-{s[0]}x{s[1]}" for t, s, _ in MERGE_CASES]
SENT = 0xA5


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


def _plan(hw, tile, ov, ramp=None):
    from diffews_amd.input_pipeline import TilePlan
    return TilePlan(hw, tile, ov, ramp)


def _merge_guarded(ops, p, win, guard):
    """tiles_merge into buffers with sentinels before and after `out` and `mx`; returns (out, mx) on the host."""
    N = win.shape[0]
    n = N * 3 * p.img_h * p.img_w
    flat = torch.full((n + 2 * guard,), SENT, dtype=torch.uint8, device="cuda")
    mxb = torch.full((N + 2,), -7, dtype=torch.int32, device="cuda")
    out, mx = ops.tiles_merge(p, win, out=flat[guard:guard + n].view(N, 3, p.img_h, p.img_w), mx=mxb[1:N + 1])
    torch.cuda.synchronize()
    assert (flat[:guard] == SENT).all() and (flat[guard + n:] == SENT).all(), "tiles_merge wrote outside out"
    assert mxb[0].item() == -7 and mxb[-1].item() == -7, "tiles_merge wrote outside mx"
    return out.cpu(), mx.cpu()


@pytest.mark.parametrize("tile,hw,ov", MERGE_CASES, ids=IDS)
def test_tiles_merge_equals_reference(ops, tile, hw, ov):
    rs = np.random.RandomState(hw[0] * 1000 + hw[1])
    for N in (1, 3):
        for ramp in sorted({1, ov, min(tile) // 2}):
            p = _plan(hw, tile, ov, ramp)
            win = rs.randint(0, 256, (N, p.T, 3) + tile).astype(np.uint8)
            want, want_mx = tr.merge(win, hw, p.ys, p.xs, ramp)
            for guard in (64, 61):            # 61: out itself is not word-aligned
                got, mx = _merge_guarded(ops, p, torch.from_numpy(win).cuda(), guard)
                what = (tile, hw, N, ramp, guard)
                assert torch.equal(got, torch.from_numpy(want)), (what, int((got.numpy() != want).sum()))
                assert mx.tolist() == want_mx.tolist(), what
            if p.T == 1:
                assert torch.equal(got, torch.from_numpy(win[:, 0])), "one window must be the identity"


@pytest.mark.parametrize("tile,hw,ov", MERGE_CASES[1:], ids=IDS[1:])
def test_tiles_merge_one_bright_window(ops, tile, hw, ov):
    """One window all 255, the rest 0: the overlaps show the rounding (half goes up) and the maximum is 255 per class that
    has the window, 0 for the class that has none."""
    for ramp in sorted({1, ov, min(tile) // 2}):
        p = _plan(hw, tile, ov, ramp)
        win = np.zeros((2, p.T, 3) + tile, np.uint8)
        win[0, p.T - 1] = 255
        want, want_mx = tr.merge(win, hw, p.ys, p.xs, ramp)
        got, mx = _merge_guarded(ops, p, torch.from_numpy(win).cuda(), 64)
        assert torch.equal(got, torch.from_numpy(want)) and mx.tolist() == want_mx.tolist() == [255, 0], (tile, hw, ramp)
    if tile == (8, 8) and hw == (8, 9):
        p = _plan(hw, tile, ov, 1)
        got, _ = _merge_guarded(ops, p, torch.from_numpy(win).cuda(), 64)
        assert (got[0, :, :, 1:8] == 128).all() and (got[0, :, :, 0] == 0).all() and (got[0, :, :, 8] == 255).all()


CUT_CASES = [((8, 8), (13, 29), 2), ((8, 16), (19, 37), 3), ((8, 6), (19, 20), 2), ((64, 64), (88, 150), 8)]


@pytest.mark.parametrize("tile,hw,ov", CUT_CASES, ids=[f"{t[0]}x{t[1]}-on-{s[0]}x{s[1]}" for t, s, _ in CUT_CASES])
def test_tiles_cut_equals_the_input_transform(ops, tile, hw, ov):
    """Every window is bit for bit DeviceImageTransform(tile).image(crop) and lut[crop] in numpy; a first / count sub-range
    writes only its windows, also into a buffer that is not 16-byte aligned."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    rs = np.random.RandomState(hw[1])
    img = rs.randint(0, 256, hw + (3,)).astype(np.uint8)
    p = _plan(hw, tile, ov)
    tf = DeviceImageTransform(tile)
    dev = torch.from_numpy(img).cuda()
    got = ops.tiles_cut(p, dev, tf.lut)
    assert got.shape == (p.T, 3) + tile and got.dtype == torch.float32
    lut = tf.lut.cpu().numpy()
    for t, (y, x) in enumerate(tr.windows(p.ys, p.xs)):
        crop = img[y:y + tile[0], x:x + tile[1]]
        assert torch.equal(got[t].cpu(), torch.from_numpy(lut[crop].transpose(2, 0, 1).copy())), t
        assert torch.equal(got[t], tf.image(crop)), t
    per = 3 * tile[0] * tile[1]
    first, count = 1, min(3, p.T - 1)
    for lead in (4, 1):                       # floats before the slice: 16-byte aligned or not
        flat = torch.full(((count + 2) * per + lead,), 777.0, device="cuda")
        out = flat[lead + per:lead + (count + 1) * per].view(count, 3, *tile)
        ops.tiles_cut(p, dev, tf.lut, first, count, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, got[first:first + count]), lead
        assert (flat[:lead + per] == 777.0).all() and (flat[lead + (count + 1) * per:] == 777.0).all(), lead


@pytest.mark.parametrize("tile,hw,ov", [((8, 16), (19, 37), 3), ((64, 64), (88, 150), 8)], ids=["8x16", "64x64"])
def test_cut_then_merge_returns_the_image(ops, tile, hw, ov):
    """The windows' floats go back to bytes through the inverse of the table (it is strictly increasing) and merge to
    exactly the image's planes, for every ramp."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    img = np.random.RandomState(4).randint(0, 256, hw + (3,)).astype(np.uint8)
    tf = DeviceImageTransform(tile)
    for ramp in sorted({1, ov, min(tile) // 2}):
        p = _plan(hw, tile, ov, ramp)
        q = ops.tiles_cut(p, torch.from_numpy(img).cuda(), tf.lut)
        win = torch.searchsorted(tf.lut, q.contiguous()).to(torch.uint8)
        assert torch.equal(tf.lut[win.long()], q)
        got, mx = ops.tiles_merge(p, win[None].contiguous())
        assert torch.equal(got[0].cpu(), torch.from_numpy(img).permute(2, 0, 1)), ramp
        assert mx.tolist() == [int(img.max())]


# ------------------------------------------------------------------------------------------------ the route, tiny engine

HW, TILE = (88, 150), (64, 64)
SHOTS = (1, 3, 2)


def _image(hw, seed):
    return np.random.RandomState(seed).randint(0, 256, hw + (3,)).astype(np.uint8)


def _gt(hw, N, seed):
    rs = np.random.RandomState(seed)
    g = rs.randint(0, N + 1, hw).astype(np.uint8)
    g[rs.rand(*hw) < 0.05] = 255
    return g


def _supports(pipe, nway):
    if not nway:
        sup, msk = _support_set(2, 64, seed=900)
        return pipe.prepare_support(sup.cuda(), msk.cuda())
    sets = [_support_set(s, 64, seed=910 + 10 * c) for c, s in enumerate(SHOTS)]
    return pipe.prepare_support_classes([a.cuda() for a, _ in sets], [m.cuda() for _, m in sets])


def _routed_windows(pipe, ops, support, nway, plan, img, batch, captured):
    """The seg_u8 the routed call returns for every window, in segment_tiled's grouping: batches of `batch` in window order,
    the last one padded by repeating the image's last window.  -> uint8 [N, T, 3, th, tw] on the host."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    q = ops.tiles_cut(plan, torch.from_numpy(img).cuda(), DeviceImageTransform(TILE).lut)
    parts = []
    for first in range(0, plan.T, batch):
        qb = q[first:first + batch]
        count = qb.shape[0]
        if count < batch:
            qb = torch.cat([qb, qb[-1:].expand(batch - count, -1, -1, -1)])
        if nway:
            parts.append(pipe.segment_classes(support, qb.contiguous(), captured=captured)["seg_u8"][:, :count].cpu())
        else:
            parts.append(pipe.segment_queries(support, qb.contiguous(), captured=captured)["seg_u8"][None, :count].cpu())
    return torch.cat(parts, dim=1).numpy()


@pytest.mark.parametrize("nway,batch", [(False, 2), (True, 2), (False, 4)], ids=["bank-b2", "set-b2", "bank-b4-padded"])
def test_segment_tiled_equals_routed_calls_merged_by_the_reference(models, ops, nway, batch):
    """88 x 150 against a 2-shot bank and a ragged 3-class set, eager and captured: seg_u8 is the reference's merge of the
    routed calls' seg_u8 (same grouping, padding and captured flag), mx its maxima, labels / counts are ops.seg_labels on the
    merged bytes and the torch rule of tests/nway_ref.py; one graph per support (not per batch), without a memset node."""
    pipe = models["pipe"]
    pipe._graphs = {}
    support = _supports(pipe, nway)
    N = len(SHOTS) if nway else 1
    img, gt = _image(HW, 5), _gt(HW, N, 6)
    try:
        for captured in (False, True):
            before = len(pipe._graphs)
            pipe.graph_nodes = 0
            r = pipe.segment_tiled(support, img, gt, batch=batch, captured=captured)
            r = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}
            assert len(pipe._graphs) == before + int(captured)
            assert (pipe.graph_nodes > 0) == captured             # every capture is checked for memset nodes
            p = r["plan"]
            assert (p.ys, p.xs, p.T, p.overlap, p.ramp) == ([0, 24], [0, 43, 86], 6, 8, 8)
            win = _routed_windows(pipe, ops, support, nway, p, img, batch, captured)
            assert len(pipe._graphs) == before + int(captured)    # the same key: nothing new was captured
            want, want_mx = tr.merge(win, HW, p.ys, p.xs, p.ramp)
            assert r["seg_u8"].shape == (N, 3) + HW and torch.equal(r["seg_u8"].cpu(), torch.from_numpy(want)), captured
            assert r["mx"].tolist() == want_mx.tolist()
            gtd = torch.from_numpy(gt).cuda()[None]
            lab, cnt = ops.seg_labels(r["seg_u8"].view(N, 1, 3, *HW), r["mx"], gtd)
            ref_l, ref_c = nway_ref.seg_labels(r["seg_u8"].cpu()[:, None], torch.from_numpy(gt)[None])
            assert r["labels"].shape == HW and r["labels"].dtype == torch.uint8
            assert torch.equal(r["labels"], lab[0]) and torch.equal(r["labels"].cpu(), ref_l[0])
            if nway:
                assert "pred" not in r and r["counts"].shape == (2, N + 1)
                assert torch.equal(r["counts"], cnt[0]) and torch.equal(r["counts"].cpu(), ref_c[0])
            else:
                assert torch.equal(r["pred"], r["labels"]) and r["counts"].shape == (4,)
                assert r["counts"].tolist() == cnt.flatten().tolist() == ref_c.flatten().tolist()
            assert pipe.segment_tiled(support, img, batch=batch, captured=captured)["counts"] is None
    finally:
        pipe._graphs = {}


def test_segment_tiled_of_one_window_is_segment_queries(models, ops):
    """A 64 x 64 image is one window: seg_u8 and, with gt, counts are exactly segment_queries' for that query (in the same
    batch: the window and its padding copy)."""
    from diffews_amd.input_pipeline import DeviceImageTransform
    pipe = models["pipe"]
    bank = _supports(pipe, False)
    img, gt = _image(TILE, 7), _gt(TILE, 1, 8)
    r = pipe.segment_tiled(bank, img, gt, batch=2, captured=False)
    assert r["plan"].T == 1
    q = DeviceImageTransform(TILE).image(img)
    gtd = torch.from_numpy(gt).cuda()
    one = pipe.segment_queries(bank, torch.stack([q, q]), torch.stack([gtd, gtd]), captured=False)
    assert torch.equal(r["seg_u8"][0], one["seg_u8"][0])
    assert r["counts"].tolist() == one["counts"][0].tolist()
    with pytest.raises(ValueError, match="segment_stream"):
        pipe.segment_tiled(bank, _image((63, 150), 1))
    with pytest.raises(TypeError):
        pipe.segment_tiled(None, img)


@pytest.mark.parametrize("nway", [False, True], ids=["bank", "set"])
def test_evaluate_tiled_sums_the_calls_counts(models, nway):
    from diffews_amd.evaluate import evaluate_tiled
    from diffews_amd.metrics import nway_iou
    pipe = models["pipe"]
    pipe._graphs = {}
    support = _supports(pipe, nway)
    N = len(SHOTS) if nway else 1
    items = [(_image(HW, 11), _gt(HW, N, 12)), (_image((64, 100), 13), _gt((64, 100), N, 14))]
    try:
        total = sum(pipe.segment_tiled(support, im, g, batch=2, captured=True)["counts"].clone() for im, g in items)
        if nway:
            miou, iou, counts = evaluate_tiled(pipe, support, items, batch=2)
            assert torch.equal(counts, total)
            ref_iou, ref_miou = nway_iou(total)
            assert miou == ref_miou and torch.equal(iou, ref_iou)
        else:
            miou, fb_iou, meter = evaluate_tiled(pipe, support, items, class_id=3, batch=2)
            assert meter.intersection_buf[:, 3].tolist() == total[:2].tolist()
            assert meter.union_buf[:, 3].tolist() == total[2:].tolist()
            assert int(meter.intersection_buf.sum()) == int(total[:2].sum())
        assert len(pipe._graphs) == 1                 # one support, one batch shape: one graph for both images
    finally:
        pipe._graphs = {}
