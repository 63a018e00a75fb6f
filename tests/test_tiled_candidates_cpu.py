"""CPU tests of per-window candidate classes in tiled segmentation: the host plan helpers TilePlan.candidate_table and
TilePlan.candidates_from_labels, the host reference tests/tiles_cand_ref.py against the dense references it is stated
through, and the C ABI of dfw_tiles_labels_cand (header, ctypes mirror, host-side validation: no launch, no GPU).  Every
comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nway_ref
import tiles_cand_ref as tcr
import tiles_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ERANGE = -1, -3


def _plan(*a, **k):
    from diffews_amd.input_pipeline import TilePlan
    return TilePlan(*a, **k)


# ------------------------------------------------------------------------------------------------ candidate_table

def test_candidate_table_layout_and_sorting():
    p = _plan((88, 150), (64, 64), 8)
    assert p.T == 6
    ct = p.candidate_table([(2, 0), [1], (), torch.tensor([2, 0, 1]), np.array([2]), []], 3)
    assert ct["sets"] == ((0, 2), (1,), (), (0, 1, 2), (2,), ())
    assert ct["E"] == 7
    assert ct["tab"].dtype == torch.int32 and ct["tab"].tolist() == [0, 2, 3, 3, 6, 7, 7] + [0, 2, 1, 0, 1, 2, 2]
    # no entry at all: E = 0, and the table still holds one (unread) class word, E_cap = max(E, 1)
    ct = p.candidate_table([()] * 6, 3)
    assert ct["E"] == 0 and ct["tab"].tolist() == [0] * 7 + [0] and ct["sets"] == ((),) * 6
    # every class everywhere, at the largest library
    ct = p.candidate_table([range(254)] * 6, 254)
    assert ct["E"] == 6 * 254 and ct["tab"].numel() == 7 + 6 * 254
    assert ct["tab"][:7].tolist() == [254 * t for t in range(7)] and ct["tab"][7:].tolist() == list(range(254)) * 6


def test_candidate_table_rejects():
    p = _plan((88, 150), (64, 64), 8)
    with pytest.raises(ValueError, match="5 candidate lists for 6 windows"):
        p.candidate_table([()] * 5, 3)
    with pytest.raises(ValueError, match="7 candidate lists for 6 windows"):
        p.candidate_table([()] * 7, 3)
    with pytest.raises(ValueError, match="twice"):
        p.candidate_table([(1, 1), (), (), (), (), ()], 3)
    for bad in (3, -1):
        with pytest.raises(ValueError, match="names set"):
            p.candidate_table([(), (), (0, bad), (), (), ()], 3)
    with pytest.raises(ValueError, match="byte"):
        p.candidate_table([()] * 6, 255)
    with pytest.raises(ValueError, match="byte"):
        p.candidate_table([()] * 6, 0)


# ------------------------------------------------------------------------------------------------ candidates_from_labels

def _label_map(hw, N, seed, ignore=0.05):
    rs = np.random.RandomState(seed)
    m = np.zeros(hw, np.uint8)
    for _ in range(6):                                    # a few rectangles of classes on background
        y, x = rs.randint(0, hw[0]), rs.randint(0, hw[1])
        m[y:y + rs.randint(1, hw[0] // 3), x:x + rs.randint(1, hw[1] // 3)] = 1 + rs.randint(0, N)
    m[rs.rand(*hw) < ignore] = 255
    return m


def _brute(p, m, min_pixels, ya_yb_xa_xb):
    out = []
    for t in range(p.T):
        ya, yb, xa, xb = ya_yb_xa_xb(t)
        crop = m[ya:yb, xa:xb]
        out.append([c for c in range(254) if int((crop == c + 1).sum()) >= min_pixels])
    return out


@pytest.mark.parametrize("hw,tile,ov", [((88, 150), (64, 64), 8), ((19, 37), (8, 16), 3), ((13, 13), (8, 8), 4)])
def test_candidates_from_a_full_size_map_are_the_crops_classes(hw, tile, ov):
    p = _plan(hw, tile, ov)
    m = _label_map(hw, 5, hw[1])
    for min_pixels in (1, 4, 30):
        want = _brute(p, m, min_pixels, lambda t: (p.origin(t)[0], p.origin(t)[0] + tile[0], p.origin(t)[1], p.origin(t)[1] + tile[1]))
        assert p.candidates_from_labels(m, min_pixels=min_pixels) == want
        assert p.candidates_from_labels(torch.from_numpy(m), min_pixels=min_pixels) == want
    assert any(p.candidates_from_labels(m)) and all(c == sorted(c) for c in p.candidates_from_labels(m))
    # 255 is ignored, like 0: a map of nothing else proposes nothing
    only = np.where(m == 255, m, 0).astype(np.uint8)
    assert (only == 255).any() and p.candidates_from_labels(only) == [[] for _ in range(p.T)]
    # min_pixels counts pixels of the class inside the footprint
    one = np.zeros(hw, np.uint8)
    one[0:2, 0:3] = 4
    assert p.candidates_from_labels(one, min_pixels=6)[0] == [3] and p.candidates_from_labels(one, min_pixels=7)[0] == []


def test_candidates_from_a_coarser_map_and_margin():
    """A map 4x coarser than the 96 x 160 image: window t's footprint is rows (y0 * lh) // h .. ceil((y0 + th) * lh / h)
    (columns alike), grown by `margin` and clipped; compared against that formula spelt out, and on hand-placed pixels."""
    hw, tile = (96, 160), (64, 64)
    p = _plan(hw, tile, 8)
    assert (p.ys, p.xs) == ([0, 32], [0, 48, 96])
    lh, lw = 24, 40
    m = _label_map((lh, lw), 4, 3)
    for margin in (0, 1, 3):
        def foot(t, margin=margin):
            y0, x0 = p.origin(t)
            ya, yb = (y0 * lh) // 96, -(-((y0 + 64) * lh) // 96)
            xa, xb = (x0 * lw) // 160, -(-((x0 + 64) * lw) // 160)
            return max(0, ya - margin), min(lh, yb + margin), max(0, xa - margin), min(lw, xb + margin)
        for min_pixels in (1, 5):
            assert p.candidates_from_labels(m, min_pixels=min_pixels, margin=margin) == _brute(p, m, min_pixels, foot)
    # window 1 = rows 0..63, columns 48..111 -> map rows 0..15, columns 12..27; a pixel just outside needs margin 1
    z = np.zeros((lh, lw), np.uint8)
    z[16, 28] = 2
    z[0, 12] = 3
    assert p.candidates_from_labels(z)[1] == [2]
    assert p.candidates_from_labels(z, margin=1)[1] == [1, 2]
    assert p.candidates_from_labels(z) == [[2], [2], [], [], [], [1]]         # window 5: rows 8..23, columns 24..39
    # a map smaller than the window grid still gives every window at least one pixel
    tiny = np.full((1, 2), 7, np.uint8)
    assert p.candidates_from_labels(tiny) == [[6]] * 6
    with pytest.raises(ValueError, match="uint8"):
        p.candidates_from_labels(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="margin"):
        p.candidates_from_labels(z, margin=-1)


# ------------------------------------------------------------------------------------------------ the reference

def test_reference_with_every_pair_listed_is_the_dense_reference():
    """tiles_cand_ref on the entries of a full table = tiles_ref.merge + nway_ref.seg_labels on the same bytes, class-major;
    dropping a pair equals zeroing it; a class listed nowhere has maximum 0 and no pixel."""
    hw, tile, ov, N = (13, 29), (8, 8), 2, 3
    p = _plan(hw, tile, ov)
    rs = np.random.RandomState(1)
    win = rs.randint(0, 256, (N, p.T, 3) + tile).astype(np.uint8)
    gt = rs.randint(0, N + 1, hw).astype(np.uint8)
    ct = p.candidate_table([range(N)] * p.T, N)
    ent = np.ascontiguousarray(win.transpose(1, 0, 2, 3, 4)).reshape(-1, 3, *tile)       # window-major entries
    assert np.array_equal(tcr.dense(ent, ct["tab"], N, p.T), win)
    lab, cnt, mx, area = tcr.labels_cand(ent, ct["tab"], N, hw, p.ys, p.xs, p.ramp, gt)
    merged, want_mx = tr.merge(win, hw, p.ys, p.xs, p.ramp)
    want_lab, want_cnt = nway_ref.seg_labels(torch.from_numpy(merged)[:, None], torch.from_numpy(gt)[None])
    assert torch.equal(lab, want_lab[0]) and torch.equal(cnt, want_cnt[0]) and mx.tolist() == want_mx.tolist()
    assert area[:, 1].tolist() == [int((lab == c + 1).sum()) for c in range(N)] and (area[:, 0] >= area[:, 1]).all()
    lists = [[c for c in range(N) if c != 1 and (t + c) % 3] for t in range(p.T)]
    ct = p.candidate_table(lists, N)
    ent2 = np.stack([win[c, t] for t, cs in enumerate(lists) for c in cs])
    zeroed = win.copy()
    for t in range(p.T):
        for c in range(N):
            if c not in lists[t]:
                zeroed[c, t] = 0
    lab2, _, mx2, area2 = tcr.labels_cand(ent2, ct["tab"], N, hw, p.ys, p.xs, p.ramp)
    merged2, want_mx2 = tr.merge(zeroed, hw, p.ys, p.xs, p.ramp)
    assert torch.equal(lab2, nway_ref.labels(torch.from_numpy(merged2)[:, None])[0]) and mx2.tolist() == want_mx2.tolist()
    assert mx2[1] == 0 and area2[1].tolist() == [0, 0] and not (lab2 == 2).any()


# ------------------------------------------------------------------------------------------------ the C ABI

def test_header_ctypes_and_symbol(hip_lib):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int dfw_tiles_labels_cand(const dfw_tile_plan* plan, const uint8_t* ent, const int32_t* tab, "
            "const int32_t* tab_host, const uint8_t* gt, uint8_t* labels, uint32_t* mx, int64_t* counts, int64_t* area, "
            "int32_t E_cap, int32_t N, float r_threshold, float threshold, dfw_stream_t stream);") in flat
    i32, f32, vp = C.c_int32, C.c_float, C.c_void_p
    assert L.SYMBOLS["dfw_tiles_labels_cand"] == (i32, [C.POINTER(L.TilePlan), vp, vp, C.POINTER(i32), vp, vp, vp, vp, vp, i32,
                                                        i32, f32, f32, vp])
    assert hip_lib.dfw_tiles_labels_cand is not None and hip_lib.dfw_version() >= 113


def _valid(N=3, E_cap=None):
    """A fully valid dfw_tiles_labels_cand call on host memory (never launched: every test below breaks one thing): tile
    8 x 16 on 19 x 37, nine windows, two entries in windows 0 and 4, one in window 8."""
    p = _plan((19, 37), (8, 16), 2)
    ct = p.candidate_table([(0, 2), (), (), (), (1, 2), (), (), (), (0,)], N)
    E_cap = ct["E"] if E_cap is None else E_cap
    tab = np.zeros(p.T + 1 + E_cap, np.int32)
    tab[:p.T + 1 + ct["E"]] = ct["tab"].numpy()
    keep = dict(tab=tab, ent=np.zeros((E_cap, 3, 8, 16), np.uint8), gt=np.zeros((19, 37), np.uint8),
                labels=np.zeros((19, 37), np.uint8), mx=np.zeros(N, np.uint32), counts=np.zeros((2, N + 1), np.int64),
                area=np.zeros((N, 2), np.int64))
    a = dict(plan=p.c_struct(), ent=keep["ent"].ctypes.data, tab=tab.ctypes.data, tab_host=tab, gt=keep["gt"].ctypes.data,
             labels=keep["labels"].ctypes.data, mx=keep["mx"].ctypes.data, counts=keep["counts"].ctypes.data,
             area=keep["area"].ctypes.data, E_cap=E_cap, N=N, r=0.25, t=0.0)
    return a, keep, p


def _call(lib, a):
    host = None if a["tab_host"] is None else a["tab_host"].ctypes.data_as(C.POINTER(C.c_int32))
    return lib.dfw_tiles_labels_cand(C.byref(a["plan"]) if a["plan"] is not None else None, a["ent"], a["tab"], host, a["gt"],
                                     a["labels"], a["mx"], a["counts"], a["area"], a["E_cap"], a["N"], a["r"], a["t"], None)


def test_labels_cand_validates_on_the_host_before_any_launch(hip_lib):
    """Each break of one thing of an otherwise valid call returns DFW_EINVAL from the host-side checks (the buffers are
    host memory and the stream is null: nothing may be launched)."""
    for field in ("plan", "tab", "tab_host", "labels", "mx", "ent"):
        a, keep, p = _valid()
        a[field] = None
        assert _call(hip_lib, a) == DFW_EINVAL, field
    T = 9

    def broken(f, **kw):
        a, keep, p = _valid(**kw)
        f(a, a["tab_host"])
        return _call(hip_lib, a), keep

    def set_(i, v):
        def f(a, tab):
            tab[i] = v
        return f
    assert broken(set_(0, 1))[0] == DFW_EINVAL                        # offsets do not start at 0
    assert broken(set_(3, 1))[0] == DFW_EINVAL                        # offsets descend: 0 2 2 1 2 ...
    assert broken(set_(T, 6))[0] == DFW_EINVAL                        # off[T] above E_cap = 5
    assert broken(set_(T + 1 + 1, 3))[0] == DFW_EINVAL                # a class outside 0..N-1
    assert broken(set_(T + 1 + 0, -1))[0] == DFW_EINVAL
    assert broken(set_(T + 1 + 1, 0))[0] == DFW_EINVAL                # (0, 0): not strictly ascending
    assert broken(set_(T + 1 + 2, 2))[0] == DFW_EINVAL                # window 4: (2, 2)
    assert broken(set_(T + 1 + 0, 2))[0] == DFW_EINVAL                # window 0: (2, 2)
    for N in (0, -1, 255):
        assert broken(lambda a, tab, N=N: a.update(N=N))[0] == DFW_EINVAL, N
    assert broken(lambda a, tab: a.update(E_cap=0))[0] == DFW_EINVAL
    assert broken(lambda a, tab: a.update(gt=None))[0] == DFW_EINVAL                       # counts without gt
    assert broken(lambda a, tab: a.update(r=0.0, t=0.0))[0] == DFW_EINVAL                  # neither threshold > 0
    assert broken(lambda a, tab: a.update(r=-1.0, t=-0.5))[0] == DFW_EINVAL
    assert broken(lambda a, tab: setattr(a["plan"], "ramp", 0))[0] == DFW_EINVAL           # a bad plan
    assert broken(lambda a, tab: a["plan"].ys.__setitem__(1, 0))[0] == DFW_EINVAL


def test_labels_cand_refuses_a_plan_whose_sums_are_not_proven_to_fit(hip_lib):
    """dfw_tiles_merge's 32-bit proof and its answer: three 4096-row windows 1024 apart with ramp 2048 are refused with
    DFW_ERANGE on the host; with ramp 1024 the bound holds and the next check is reached (a null mx: DFW_EINVAL comes
    first, so this call cannot launch either).  img_h above 65535 is DFW_ERANGE as well."""
    from diffews_amd import _lib as L
    p = L.TilePlan()
    p.img_h, p.img_w, p.tile_h, p.tile_w, p.ny, p.nx, p.ramp = 6144, 4096, 4096, 4096, 3, 1, 2048
    p.ys[:3] = [0, 1024, 2048]
    buf = np.zeros(16, np.uint8).ctypes.data
    tab = np.zeros(3 + 1 + 1, np.int32)                               # three windows, no entry, E_cap = 1
    host = tab.ctypes.data_as(C.POINTER(C.c_int32))

    def call(mx=buf):
        return hip_lib.dfw_tiles_labels_cand(C.byref(p), None, tab.ctypes.data, host, None, buf, mx, None, None, 1, 1, 0.25,
                                             0.0, None)
    assert call() == DFW_ERANGE
    p.ramp = 1024
    assert call(mx=None) == DFW_EINVAL
    q = L.TilePlan()
    q.img_h, q.img_w, q.tile_h, q.tile_w, q.ny, q.nx, q.ramp = 65536, 8, 65536, 8, 1, 1, 1
    tab1 = np.zeros(1 + 1 + 1, np.int32)
    assert hip_lib.dfw_tiles_labels_cand(C.byref(q), None, tab1.ctypes.data, tab1.ctypes.data_as(C.POINTER(C.c_int32)), None,
                                         buf, buf, None, None, 1, 1, 0.25, 0.0, None) == DFW_ERANGE
