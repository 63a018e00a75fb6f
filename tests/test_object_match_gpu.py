"""GPU tests of the matching stage: ops.seg_match against tests/match_ref.py on n, pairs[:kept], pair_off, area, match,
gmatch and pq, bit for bit -- at the smallest shapes that reach every path of the kernels (one pixel, one row, a block of
positions less one, exactly, plus one with a record across the border, two blocks and a bit), on ids that
ops.seg_components made of a prediction and a perturbed ground truth, on hand-made ids across the sort's one to four digit
passes and across its chunk sizes; then both truncations, skip, classes, thresholds, guards, poisoned and repeated
launches, a captured launch, and objects.match_objects / matches_to_host / pipe.match_objects on top.  All integers: every
comparison is exact.

Every buffer sits inside sentinel guards; in half of the cases the id maps lie 61 words and skip 3 bytes into their
allocations, off the alignment of the vector loads, and the workspace 60 bytes into its own."""
import ctypes as C

import numpy as np
import pytest
import torch

import match_ref as mr

pytestmark = pytest.mark.gpu

SENT = 0xA5
TABLES = ("n", "pair_off", "area", "match", "gmatch", "pq")


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.fixture(scope="module")
def block(hip_lib):
    p, r = C.c_int32(), C.c_int32()
    assert hip_lib.dfw_seg_match_block(C.byref(p), C.byref(r)) == 0
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


def _launch(ops, pids, gids, cap_p, cap_g, nlabels, max_records, max_pairs, pstats=None, gstats=None, skip=None, iou=(1, 2),
            odd=False, fill=None, bufs=None, repeat=1):
    """ops.seg_match on numpy maps [B, H, W] into guarded buffers, optionally pre-filled with a byte; returns numpy results
    after checking every guard, and the buffers.  odd: the inputs and the workspace off the vector alignment."""
    B, H, W = pids.shape
    i32, u8 = torch.int32, torch.uint8
    if bufs is None:
        nbytes = ops.seg_match_workspace(B, H, W, cap_p, cap_g, max_records, max_pairs)
        assert nbytes > 0
        bufs = dict(pids=_Guarded((B, H, W), i32, 61 if odd else 4), gids=_Guarded((B, H, W), i32, 61 if odd else 8),
                    pstats=_Guarded((B, cap_p, 8), i32, 4), gstats=_Guarded((B, cap_g, 8), i32, 4),
                    skip=_Guarded((B, H, W), u8, 3 if odd else 16),
                    pairs=_Guarded((B, max_pairs, 3), i32, 4, fill), pair_off=_Guarded((B, cap_p + 2), i32, 4, fill),
                    area=_Guarded((B, cap_p + cap_g + 2), i32, 4, fill), match=_Guarded((B, cap_p, 3), i32, 4, fill),
                    gmatch=_Guarded((B, cap_g), i32, 4, fill), pq=_Guarded((B, nlabels + 1, 4), torch.int64, 2, fill),
                    n=_Guarded((B, 4), i32, 4, fill), ws=_Guarded((nbytes,), u8, 60 if odd else 64, fill))
    given = dict(pids=pids, gids=gids, pstats=pstats, gstats=gstats, skip=skip)
    for k, v in given.items():
        if v is not None:
            bufs[k].t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    g = {k: v.t for k, v in bufs.items()}
    for _ in range(repeat):
        ops.seg_match(g["pids"], g["gids"], g["pairs"], g["pair_off"], g["area"], g["match"], g["gmatch"], g["pq"], g["n"],
                      g["ws"], max_records, pstats=None if pstats is None else g["pstats"],
                      gstats=None if gstats is None else g["gstats"], skip=None if skip is None else g["skip"], iou=iou)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    for k, v in given.items():
        if v is not None:
            assert np.array_equal(g[k].cpu().numpy(), v), f"the input {k} was modified"
    return {k: g[k].cpu().numpy() for k in TABLES + ("pairs",)}, bufs


def _same(got, want, what, rest=-7):
    """Every table whole, pairs up to kept; the rows behind hold `rest`, what the buffer was filled with."""
    for k in TABLES:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())
    for b, w in enumerate(want["pairs"]):
        assert np.array_equal(got["pairs"][b, :len(w)], w), (what, "pairs", b)
        if rest is not None:
            assert (got["pairs"][b, len(w):] == rest).all(), (what, "rows behind kept were written", b)


def _word(fill):
    return int(np.array([fill] * 4, np.uint8).view(np.int32)[0])


def _both(ops, pids, gids, cap_p, cap_g, nlabels, M, MP, what, **kw):
    """One launch against the reference; returns both."""
    odd = kw.pop("odd", False)
    want = mr.match(pids, gids, cap_p, cap_g, nlabels, M, MP, **kw)
    got, _ = _launch(ops, pids, gids, cap_p, cap_g, nlabels, M, MP, odd=odd, **kw)
    _same(got, want, what)
    return got, want


def _runs_map(B, H, W, top, rs, mean=3):
    """int32 [B, H, W]: runs of a mean length over the flattened map, values in [-1, top + 1] with 0 frequent."""
    n = B * H * W
    cuts = rs.rand(n) < 1.0 / mean
    vals = rs.randint(-1, top + 2, n)
    vals[rs.rand(n) < 0.3] = 0
    return vals[np.cumsum(cuts) - 1].astype(np.int32).reshape(B, H, W)   # index -1 in front of the first cut: any value


def _stats(B, cap, nlabels, rs):
    s = rs.randint(0, 1000, (B, cap, 8)).astype(np.int32)                # only column 0 is read: the rest is noise
    s[:, :, 0] = rs.randint(0, nlabels + 2, (B, cap))                    # class 0 and nlabels + 1 among them
    return s


SHAPES = ["1x1", "1x7", "5x3", "block-1", "block", "block+1", "two-blocks-and-a-bit"]


@pytest.mark.parametrize("which", range(7), ids=SHAPES)
def test_equals_the_reference(ops, block, which):
    P, R = block
    H, W = [(1, 1), (1, 7), (5, 3), (1, P - 1), (1, P), (1, P + 1), (37, 2 * P // 37 + 9)][which]
    if which == 6:
        assert 2 * P < H * W < 3 * P and W % 2 == 1
    rs = np.random.RandomState(1000 * H + W)
    for rep in range(3):
        cap_p, cap_g, nl = (3, 2, 2) if rep == 0 else (9, 12, 3)
        pids, gids = _runs_map(1, H, W, cap_p, rs, 2 + 3 * rep), _runs_map(1, H, W, cap_g, rs, 4)
        if which >= 3 and W > P - 6:                                     # one record across the border of the first block
            pids[0, 0, P - 5:P + 3] = 2
            gids[0, 0, P - 5:P + 3] = 1
        if which == 6:
            flat_p, flat_g = pids.reshape(-1), gids.reshape(-1)
            flat_p[2 * P - 3:2 * P + 2], flat_g[2 * P - 3:2 * P + 2] = 1, 2
        skip = (rs.rand(1, H, W) < 0.2).astype(np.uint8) * 255
        skip[rs.rand(1, H, W) < 0.2] = 254                               # only 255 skips
        ps, gs = _stats(1, cap_p, nl, rs), _stats(1, cap_g, nl, rs)
        for odd in (False, True):
            _both(ops, pids, gids, cap_p, cap_g, nl, H * W, H * W, (H, W, rep, odd, "plain"), odd=odd)
            got, want = _both(ops, pids, gids, cap_p, cap_g, nl, H * W, H * W, (H, W, rep, odd, "stats and skip"), odd=odd,
                              pstats=ps, gstats=gs, skip=skip)
            assert want["n"][0, 0] == want["n"][0, 1] and want["n"][0, 2] == want["n"][0, 3]
    if which >= 3 and W > P - 6:
        k = mr.keys(pids[0], gids[0], cap_p, cap_g)
        assert k[P - 1] == k[P] != 0 if W > P else k[P - 2] != 0         # the record does lie across the border
    # nothing but background: no record, no pair, zeros everywhere
    zero = np.zeros((1, H, W), np.int32)
    got, _ = _both(ops, zero, zero, 3, 3, 1, H * W, H * W, (H, W, "background"))
    assert not any(got[k].any() for k in TABLES)
    # one object on either side over the whole map: one record over every block, one pair, one TP of IoU 1
    got, _ = _both(ops, zero + 2, zero + 3, 3, 3, 1, H * W, H * W, (H, W, "one object"))
    assert got["n"].tolist() == [[1, 1, 1, 1]] and got["pairs"][0, 0].tolist() == [2, 3, H * W]
    assert got["pq"][0, 1].tolist() == [1, 0, 0, 1 << 32] and got["match"][0, 1].tolist() == [3, H * W, H * W]


def _components(ops, labels, conn, cap):
    lab = torch.from_numpy(labels).cuda()
    B, H, W = lab.shape
    ids = torch.empty(B, H, W, dtype=torch.int32, device="cuda")
    n = torch.empty(B, 2, dtype=torch.int32, device="cuda")
    stats = torch.empty(B, cap, 8, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.seg_components_workspace(B, H, W), dtype=torch.uint8, device="cuda")
    ops.seg_components(lab, ids, n, ws, stats=stats, connectivity=conn)
    return ids.cpu().numpy(), stats.cpu().numpy(), n.cpu().numpy()


@pytest.mark.parametrize("conn", [4, 8])
def test_ids_of_seg_components_three_independent_images(ops, block, conn):
    """A prediction of random blobs and a perturbed ground truth (shifted, pixels flipped, some ignored), both through
    ops.seg_components; classes from its stats tables, skip = the ground-truth label map."""
    P, R = block
    rs = np.random.RandomState(40 + conn)
    H, W, nl = 45, 2 * P // 45 + 7, 3
    labs = np.stack([mr.blobs(H, W, rs, nl, count=40) for _ in range(3)])
    gts = np.stack([mr.perturb(l, rs) for l in labs])
    gts[2] = labs[2]                                                      # one image is predicted perfectly
    cap_p, cap_g = 300, 1000
    pids, pstats, pn = _components(ops, labs, conn, cap_p)
    gids, gstats, gn = _components(ops, gts, conn, cap_g)
    assert 3 < pn[:, 0].min() and pn[:, 0].max() <= cap_p and gn[:, 0].max() <= cap_g
    got, want = _both(ops, pids, gids, cap_p, cap_g, nl, H * W, H * W, ("components", conn), pstats=pstats, gstats=gstats,
                      skip=gts)
    assert (want["n"][:, 0] == want["n"][:, 1]).all() and want["pq"][:, 1:, 0].sum() > 3
    assert want["pq"][2, :, 1:3].sum() == 0 and want["pq"][2, :, 0].sum() == pn[2, 0]      # all TP, every IoU exactly 1
    assert want["pq"][2, :, 3].sum() == int(pn[2, 0]) << 32
    assert want["pq"][:2, :, 1:3].sum() > 0
    for b in range(3):
        one, _ = _launch(ops, pids[b:b + 1], gids[b:b + 1], cap_p, cap_g, nl, H * W, H * W, pstats=pstats[b:b + 1],
                         gstats=gstats[b:b + 1], skip=gts[b:b + 1], odd=True)
        for k in TABLES:
            assert np.array_equal(one[k][0], got[k][b]), (k, b)
        kept = one["n"][0, 0]
        assert np.array_equal(one["pairs"][0, :kept], got["pairs"][b, :kept])
    # without skip the ignored pixels count, without stats every object has class 1
    _both(ops, pids, gids, cap_p, cap_g, 1, H * W, H * W, ("components, no stats", conn))


@pytest.mark.parametrize("caps", [(15, 15), (255, 255), (4095, 4095), (32767, 65535)], ids=["1 pass", "2 passes", "3 passes", "4 passes"])
def test_hand_made_ids_across_the_sort_digits(ops, block, caps):
    """40 x 50, ids at the top of the range (the cap itself, the cap less a few, above it), at the bottom and in between:
    every digit of the key takes its extreme values, and the highest key of the last case is 2^31 - 1."""
    cap_p, cap_g = caps
    rs = np.random.RandomState(cap_p)
    pool_p = np.array([-3, 0, 1, 2, cap_p // 2, cap_p - 2, cap_p - 1, cap_p, cap_p + 1])
    pool_g = np.array([0, 1, 3, cap_g // 3, cap_g // 2 + 1, cap_g - 1, cap_g, cap_g + 1, 2 * cap_g])
    n = 2 * 40 * 50
    pids = pool_p[rs.randint(0, 9, n)][np.cumsum(rs.rand(n) < 0.6) - 1].astype(np.int32).reshape(2, 40, 50)
    gids = pool_g[rs.randint(0, 9, n)][np.cumsum(rs.rand(n) < 0.6) - 1].astype(np.int32).reshape(2, 40, 50)
    pids[0, 7, 3:30], gids[0, 7, 3:30] = cap_p, cap_g
    want = mr.match(pids, gids, cap_p, cap_g, 1, 2000, 100)
    assert want["n"][:, 3].min() > 1000 and want["n"][:, 1].min() > 40
    assert want["pairs"][0][-1, :2].tolist() == [cap_p, cap_g]
    got, _ = _launch(ops, pids, gids, cap_p, cap_g, 1, 2000, 100)
    _same(got, want, caps)


def test_more_records_than_one_and_than_three_sort_chunks(ops, block):
    P, R = block
    rs = np.random.RandomState(7)
    for H, W, least, most in ((37, R // 37 + 25, R, 2 * R), (61, 3 * R // 61 + 30, 3 * R, 4 * R), (96, 96, 4 * R, 96 * 96)):
        pids = rs.randint(0, 8, (1, H, W)).astype(np.int32)
        gids = rs.randint(0, 8, (1, H, W)).astype(np.int32)
        want = mr.match(pids, gids, 7, 7, 1, H * W, 100)
        assert least < want["n"][0, 2] < most and want["n"][0, 0] == 63, want["n"]
        got, _ = _launch(ops, pids, gids, 7, 7, 1, H * W, 100)
        _same(got, want, (H, W))
        cut = int(want["n"][0, 2]) - 5                                     # the records cut inside the last chunk
        got, _ = _launch(ops, pids, gids, 7, 7, 1, cut, 100)
        _same(got, mr.match(pids, gids, 7, 7, 1, cut, 100), (H, W, "cut"))
        for M in (R, R + 1, 3 * R, 3 * R - 1):                             # and at the chunk borders
            if M < cut:
                got, _ = _launch(ops, pids, gids, 7, 7, 1, M, 100)
                _same(got, mr.match(pids, gids, 7, 7, 1, M, 100), (H, W, M))
    # more pairs than one chunk of heads: 4 x R records, each a pair of its own
    H, W = 64, 4 * R // 64
    pids = (np.arange(H * W) // 89 + 1).astype(np.int32).reshape(1, H, W)
    gids = (np.arange(H * W) % 89 + 1).astype(np.int32).reshape(1, H, W)
    want = mr.match(pids, gids, 100, 89, 1, H * W, H * W)
    assert want["n"][0, 0] == want["n"][0, 2] == H * W
    got, _ = _launch(ops, pids, gids, 100, 89, 1, H * W, H * W)
    _same(got, want, "every pixel a pair")


def test_both_truncations(ops, block):
    rs = np.random.RandomState(13)
    H, W = 33, 45
    pids, gids = _runs_map(2, H, W, 20, rs, 3), _runs_map(2, H, W, 25, rs, 3)
    ps, gs = _stats(2, 20, 2, rs), _stats(2, 25, 2, rs)
    full = mr.match(pids, gids, 20, 25, 2, H * W, H * W, pstats=ps, gstats=gs)
    rfound, pfound = int(full["n"][:, 3].min()), int(full["n"][:, 1].min())
    assert rfound > 300 and pfound > 100
    for M, MP in ((1, 1), (rfound - 1, H * W), (rfound, pfound), (rfound + 1, pfound - 1), (H * W, 1), (H * W, 37), (50, 20), (50, 49)):
        want = mr.match(pids, gids, 20, 25, 2, M, MP, pstats=ps, gstats=gs)
        got, _ = _launch(ops, pids, gids, 20, 25, 2, M, MP, pstats=ps, gstats=gs)
        _same(got, want, (M, MP))                                          # rows from kept on keep the sentinel
        for b in range(2):
            n = got["n"][b]
            assert n[2] == min(M, n[3]) and n[0] == min(MP, n[1]) and got["pair_off"][b, -1] == n[0]
            assert got["area"][b, :21].sum() == got["area"][b, 21:].sum() == got["pairs"][b, :n[0], 2].sum()
    want = mr.match(pids, gids, 20, 25, 2, H * W, 37, pstats=ps, gstats=gs)
    assert (want["n"][:, 0] < want["n"][:, 1]).all() and (want["n"][:, 2] == want["n"][:, 3]).all()
    # the first records: a prefix of the map; the first pairs: a prefix of the full pair list
    assert np.array_equal(want["pairs"][0], full["pairs"][0][:37])
    cutmap = mr.match(pids, gids, 20, 25, 2, 50, H * W, pstats=ps, gstats=gs)
    assert cutmap["n"][0].tolist()[2:] == [50, int(full["n"][0, 3])]


def test_a_skipped_object_is_absent_and_classes_must_agree(ops, block):
    H, W = 12, 20
    pids, gids = np.zeros((1, H, W), np.int32), np.zeros((1, H, W), np.int32)
    skip = np.zeros((1, H, W), np.uint8)
    pids[0, 0:4, 0:5], gids[0, 0:4, 0:5] = 1, 1                           # a perfect pair of class 1
    pids[0, 0:4, 8:12], gids[0, 0:4, 8:12] = 2, 2                         # a perfect overlap of classes 2 and 3: no match
    pids[0, 6:9, 0:4] = 3                                                 # a prediction wholly under skip: absent
    skip[0, 6:9, 0:4] = 255
    gids[0, 6:9, 8:12] = 3                                                # a ground truth wholly under skip: absent
    skip[0, 6:9, 8:12] = 255
    pids[0, 10:12, 0:6], gids[0, 10:12, 0:6] = 4, 4                       # a perfect overlap of class 5 > nlabels: no bin
    pids[0, 10:12, 10:16], gids[0, 10:12, 10:16] = 5, 5                   # a perfect overlap of class 0: no bin
    pids[0, 5, 15:19] = 9                                                 # an id above cap: background
    ps = np.zeros((1, 5, 8), np.int32)
    gs = np.zeros((1, 6, 8), np.int32)
    ps[0, :, 0] = (1, 2, 1, 5, 0)
    gs[0, :, 0] = (1, 3, 1, 5, 0, 2)
    got, want = _both(ops, pids, gids, 5, 6, 4, H * W, 50, "hand-made", pstats=ps, gstats=gs, skip=skip)
    assert got["pq"][0].tolist() == [[0, 0, 0, 0], [1, 0, 0, 1 << 32], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert got["match"][0].tolist() == [[1, 20, 20], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert got["gmatch"][0].tolist() == [1, 0, 0, 0, 0, 0]
    assert got["area"][0].tolist() == [0, 20, 16, 0, 12, 12] + [0, 20, 16, 0, 12, 12, 0]      # (0, 0) is no pair
    # without skip both are there: one more FP and one more FN of class 1; without stats all five overlaps match
    got, _ = _both(ops, pids, gids, 5, 6, 4, H * W, 50, "no skip", pstats=ps, gstats=gs)
    assert got["pq"][0, 1].tolist() == [1, 1, 1, 1 << 32]
    got, _ = _both(ops, pids, gids, 5, 6, 4, H * W, 50, "no stats", skip=skip)
    assert got["pq"][0, 1].tolist() == [4, 0, 0, 4 << 32] and got["gmatch"][0].tolist() == [1, 2, 0, 4, 5, 0]
    # stats on one side only: the other side's objects all have class 1
    got, _ = _both(ops, pids, gids, 5, 6, 4, H * W, 50, "gstats only", gstats=gs, skip=skip)
    assert got["pq"][0, 1].tolist() == [1, 3, 0, 1 << 32]


def test_thresholds_are_strict(ops, block):
    """p = 1 covers 2k pixels of a row, g = 1 the second half of them and nothing else: IoU = k / 2k, exactly one half --
    no match at 1/2; one more shared pixel and it matches.  The same at 3/4 and at 65534/65535."""
    W = 64
    for num, den, a, i in ((1, 2, 20, 10), (3, 4, 20, 15), (2, 3, 30, 20), (65534, 65535, 65535, 65534), (1, 1, 40, 40)):
        H = -(-(a + 2) // W) + 1
        pids, gids = np.zeros((1, H * W), np.int32), np.zeros((1, H * W), np.int32)
        pids[0, 1:1 + a] = 1
        gids[0, 1 + a - i:1 + a] = 1                                       # inter = i, union = a: i / a == num / den
        pids, gids = pids.reshape(1, H, W), gids.reshape(1, H, W)
        got, _ = _both(ops, pids, gids, 1, 1, 1, 100, 10, (num, den, "at"), iou=(num, den))
        assert got["pq"][0, 1].tolist() == [0, 1, 1, 0] and not got["match"].any()
        if num < den:
            gids.reshape(-1)[1 + a - i - 1] = 1                            # inter = i + 1 of the same union
            got, _ = _both(ops, pids, gids, 1, 1, 1, 100, 10, (num, den, "above"), iou=(num, den))
            assert got["pq"][0, 1].tolist() == [1, 0, 0, ((i + 1) << 32) // a] and got["match"][0, 0].tolist() == [1, i + 1, a]
            if 2 * (i + 1) > a and (num, den) != (1, 2):
                lower, _ = _both(ops, pids, gids, 1, 1, 1, 100, 10, (num, den, "at 1/2"))
                assert np.array_equal(lower["match"], got["match"])


def test_poisoned_and_repeated_launches_give_the_same_bits(ops, block):
    """Outputs and workspace pre-filled with 0xFF and with 0x7B, two launches back to back into the same buffers, and the
    same buffers on other maps: the reference's bits every time -- nothing is read before it is written, nothing accumulates
    across launches, and the rows behind kept still hold the fill."""
    P, R = block
    rs = np.random.RandomState(29)
    H, W = 67, 2 * P // 67 + 4
    pids, gids = _runs_map(2, H, W, 40, rs, 4), _runs_map(2, H, W, 30, rs, 5)
    op, og = _runs_map(2, H, W, 40, rs, 2), _runs_map(2, H, W, 30, rs, 9)
    ps, gs = _stats(2, 40, 3, rs), _stats(2, 30, 3, rs)
    skip = (rs.rand(2, H, W) < 0.1).astype(np.uint8) * 255
    for M, MP in ((H * W, 1500), (700, 300)):
        kw = dict(pstats=ps, gstats=gs, skip=skip, iou=(2, 3))
        want = mr.match(pids, gids, 40, 30, 3, M, MP, **kw)
        for fill in (0xFF, 0x7B):
            got, bufs = _launch(ops, pids, gids, 40, 30, 3, M, MP, fill=fill, **kw)
            _same(got, want, (M, hex(fill)), rest=_word(fill))
        again, _ = _launch(ops, pids, gids, 40, 30, 3, M, MP, bufs=bufs, repeat=2, **kw)
        _same(again, want, "back to back", rest=_word(0x7B))
        got, _ = _launch(ops, op, og, 40, 30, 3, M, MP, bufs=bufs, **kw)
        _same(got, mr.match(op, og, 40, 30, 3, M, MP, **kw), "another map", rest=None)


def test_captured_launch_follows_its_input_tensors(ops, hip_lib, block):
    """seg_components of both label maps and seg_match in one torch.cuda.graph: no memset node, the node count of the
    header's formula, and each replay matches whatever the two label tensors hold."""
    from diffews_amd.objects import ComponentBuffers, MatchBuffers
    rs = np.random.RandomState(31)
    B, H, W, cap, nl = 2, 41, 72, 300, 3
    labs = [np.stack([mr.blobs(H, W, rs, nl, count=25) for _ in range(B)]) for _ in range(3)]
    pb, gb = ComponentBuffers(B, H, W, cap), ComponentBuffers(B, H, W, cap)
    mb = MatchBuffers(B, H, W, cap, cap, nl, max_records=3000, max_pairs=900)
    lab = torch.zeros(B, H, W, dtype=torch.uint8, device="cuda")
    gt = torch.zeros(B, H, W, dtype=torch.uint8, device="cuda")

    def call():
        ops.seg_components(lab, pb.ids, pb.n, pb.ws, stats=pb.stats, connectivity=8)
        ops.seg_components(gt, gb.ids, gb.n, gb.ws, stats=gb.stats, connectivity=8)
        ops.seg_match(pb.ids, gb.ids, mb.pairs, mb.pair_off, mb.area, mb.match, mb.gmatch, mb.pq, mb.n, mb.ws, mb.max_records,
                      pstats=pb.stats, gstats=gb.stats, skip=gt)
    call()                                                                 # modules loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    nodes = C.c_int32()
    assert hip_lib.dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(nodes)) == 0
    assert nodes.value == 8 + 8 + 14 + 3 * 3                               # 301 * 301 keys: three digit passes
    graph.instantiate()
    for i in (0, 1, 2, 0):
        g = mr.perturb(labs[i], rs) if i else labs[i].copy()
        lab.copy_(torch.from_numpy(labs[i]))
        gt.copy_(torch.from_numpy(g))
        graph.replay()
        torch.cuda.synchronize()
        want = mr.match(pb.ids.cpu().numpy(), gb.ids.cpu().numpy(), cap, cap, nl, 3000, 900, pstats=pb.stats.cpu().numpy(),
                        gstats=gb.stats.cpu().numpy(), skip=g)
        got = {k: getattr(mb, k).cpu().numpy() for k in TABLES + ("pairs",)}
        _same(got, want, ("replay", i), rest=None)
        assert want["pq"][:, :, 0].sum() > 0 and (i or want["pq"][:, :, 1:3].sum() == 0)


# ------------------------------------------------------------------------------------------------ objects.py

def _host_same(host, want, b=None):
    for k in TABLES:
        assert np.array_equal(host[k], want[k] if b is None else want[k][b]), k
    pairs = want["pairs"] if b is None else want["pairs"][b]
    assert host["pairs"].dtype == np.int32 and np.array_equal(host["pairs"], pairs)


def test_match_objects_on_a_list_of_native_size_maps(hip_lib):
    """label_objects on two maps of different sizes, prediction and ground truth, then match_objects on the two results:
    one call per item, every value a list; matches_to_host against the reference; buffers reused and aliased; a batch, one
    map, tuples with explicit caps; wrong arguments refused."""
    from diffews_amd.metrics import panoptic_quality
    from diffews_amd.objects import MatchBuffers, label_objects, match_objects, matches_to_host
    rs = np.random.RandomState(37)
    sizes, nl = [(37, 53), (20, 64)], 3
    labs = [mr.blobs(h, w, rs, nl, count=12) for h, w in sizes]
    gts = [mr.perturb(l, rs) for l in labs]
    dev = lambda xs: [torch.from_numpy(x).cuda() for x in xs]  # noqa: E731
    op = label_objects(dev(labs), connectivity=8, max_components=64)
    og = label_objects(dev(gts), connectivity=8, max_components=128)
    m = match_objects(op, og, skip=dev(gts), nlabels=nl)
    assert all(isinstance(m[k], list) and len(m[k]) == 2 for k in TABLES + ("pairs",))
    host, truncated = matches_to_host(m)
    assert not truncated
    total = np.zeros((nl + 1, 4), np.int64)
    for i, (h, w) in enumerate(sizes):
        assert m["pairs"][i].shape == (h * w, 3) and m["pair_off"][i].shape == (66,) and m["pq"][i].shape == (nl + 1, 4)
        want = mr.match_image(op["ids"][i].cpu().numpy(), og["ids"][i].cpu().numpy(), 64, 128, nl, h * w, h * w,
                              op["stats"][i].cpu().numpy(), og["stats"][i].cpu().numpy(), gts[i])
        _host_same({k: v[i] for k, v in host.items()}, want)
        total += want["pq"]
    assert total[:, 0].sum() > 0
    q = panoptic_quality(m["pq"])
    tp, fp, fn, s = (total[1:, j].astype(np.float64) for j in range(4))
    seen = tp + fp + fn > 0
    ref = np.where(tp > 0, s / 2.0 ** 32 / np.maximum(tp, 1), 0) * np.where(seen, tp / np.maximum(tp + fp / 2 + fn / 2, 0.5), 0)
    assert np.array_equal(q["pq"][1:].cpu().numpy(), ref)
    # the mean adds at most three doubles, in an order the device chooses, and divides once: three roundings of at most
    # eps / 2 each, relative to a sum of non-negative terms
    assert abs(q["mean_pq"] - float(ref[seen].mean())) <= 1.5 * np.finfo(np.float64).eps * float(ref[seen].mean())
    # a batch with a small pair table: truncated, and the tables hold what the reference keeps
    lab = np.stack([mr.blobs(24, 31, rs, nl, count=9) for _ in range(2)])
    gt = np.stack([mr.perturb(l, rs) for l in lab])
    op = label_objects(torch.from_numpy(lab).cuda(), connectivity=4, max_components=32)
    og = label_objects(torch.from_numpy(gt).cuda(), connectivity=4, max_components=48)
    mb = MatchBuffers(2, 24, 31, 32, 48, nl, max_pairs=7)
    assert mb.max_records == 24 * 31
    args = (op["ids"].cpu().numpy(), og["ids"].cpu().numpy(), 32, 48, nl, 24 * 31)
    stats = dict(pstats=op["stats"].cpu().numpy(), gstats=og["stats"].cpu().numpy())
    for _ in range(2):
        m = match_objects(op, og, buffers=mb, iou=(3, 4))
        assert m["pairs"].data_ptr() == mb.pairs.data_ptr() and m["pq"].data_ptr() == mb.pq.data_ptr()
        host, truncated = matches_to_host(m)
        assert truncated and host["n"][:, 0].tolist() == [7, 7]
        want = mr.match(*args, 7, iou=(3, 4), **stats)
        for b in range(2):
            _host_same({k: v[b] for k, v in host.items()}, want, b)
    # one [H, W] map: no batch axis; tuples with and without stats
    one = match_objects((op["ids"][1], op["stats"][1]), (og["ids"][1], None, 48), nlabels=nl)
    assert one["pairs"].dim() == 2 and one["n"].shape == (4,) and one["pq"].shape == (nl + 1, 4)
    h1, t1 = matches_to_host(one)
    assert not t1
    _host_same(h1, mr.match_image(args[0][1], args[1][1], 32, 48, nl, 24 * 31, 24 * 31, pstats=stats["pstats"][1]))
    with pytest.raises(ValueError):
        match_objects(op, og)                                              # neither nlabels nor buffers
    with pytest.raises(ValueError):
        match_objects(op, og, buffers=mb, nlabels=nl + 1)                  # made for another class count
    with pytest.raises(ValueError):
        match_objects(op, (og["ids"], None, 47), buffers=mb)               # made for another cap
    with pytest.raises(ValueError):
        match_objects(op, (og["ids"][:1], None, 48), nlabels=nl)           # shapes differ
    with pytest.raises(ValueError):
        match_objects(op, og, nlabels=nl, skip=op["ids"])                  # skip is bytes
    with pytest.raises(RuntimeError):
        match_objects(op, og, nlabels=nl, iou=(1, 3))                      # below one half: DFW_EINVAL


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


def test_pipe_match_objects_on_the_n_way_route(pipe):
    """pipe.match_objects(pipe.objects(r), objects of a ground truth) on segment_classes' result (b = 2): the reference run
    on the ids and stats the route returned.  The ground truth is the route's own label map, perturbed."""
    from diffews_amd.objects import label_objects, matches_to_host
    from test_support_bank_gpu import _queries, _support_set
    sets = [_support_set(s, 64, seed=910 + 10 * c) for c, s in enumerate((1, 3, 2))]
    library = pipe.prepare_support_classes([a.cuda() for a, _ in sets], [m.cuda() for _, m in sets])
    r = pipe.segment_classes(library, _queries(2, 64, 77).cuda(), captured=False)
    o = pipe.objects(r, connectivity=8, max_components=256)
    labels = r["labels"].cpu().numpy()
    assert labels.shape == (2, 64, 64)
    gt = np.stack([mr.perturb(l, np.random.RandomState(5 + i)) for i, l in enumerate(labels)])
    gt_dev = torch.from_numpy(gt).cuda()
    og = label_objects(gt_dev, connectivity=8, max_components=512)
    args = (o["ids"].cpu().numpy(), og["ids"].cpu().numpy(), 256, 512, 3, 64 * 64, 64 * 64)
    stats = dict(pstats=o["stats"].cpu().numpy(), gstats=og["stats"].cpu().numpy())
    for kw, ref in ((dict(skip=gt_dev), dict(skip=gt)), (dict(iou=(3, 4)), dict(iou=(3, 4)))):
        m = pipe.match_objects(o, og, nlabels=3, **kw)
        assert m["pairs"].shape == (2, 64 * 64, 3) and m["pair_off"].shape == (2, 258) and m["pq"].shape == (2, 4, 4)
        want = mr.match(*args, **stats, **ref)
        got = {k: m[k].cpu().numpy() for k in TABLES + ("pairs",)}
        _same(got, want, kw.keys(), rest=None)
        host, truncated = matches_to_host(m)
        assert not truncated
        for b in range(2):
            _host_same({k: v[b] for k, v in host.items()}, want, b)
    # the route's labels against themselves: every object a TP of IoU 1
    m = pipe.match_objects(o, o, nlabels=3)
    n = o["n"][:, 0].cpu()
    pq = m["pq"].cpu()
    assert (n <= 256).all() and pq[:, :, 0].sum(1).tolist() == n.tolist() and pq[:, :, 1:3].sum() == 0
    assert pq[:, :, 3].sum(1).tolist() == [int(v) << 32 for v in n]
