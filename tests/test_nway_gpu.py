"""GPU tests of N-way segmentation: ops.fsa_attention_sets against the unshared launch on the bank materialised per entry
(exact), per element against the fp64 bound of tests/attention_bound.py, with the stack at the very end of its allocation;
ops.seg_labels bit-exact against tests/nway_ref.py on both paths of the kernel; pipe.prepare_support_classes /
segment_classes on the tiny config against the fp32 oracle per class, against segment_queries on .bank(c), chunked,
captured, with stale and stacked handles.

The oracle side relies on test_nway_cpu.test_oracle_definition_of_nway: the class-major batch is, per class, the reference's
call with that class' supports replicated per query; the label rule is nway_ref's, checked there against the reference's
binary prediction."""
import contextlib
import ctypes as C

import pytest
import torch

import nway_ref
import test_attention_plans_gpu as plans
from test_model_gpu import TOL_EP
from test_support_bank_gpu import models, ops, rel, _bank, _qkv, _queries, _rep, _support_set  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


# ------------------------------------------------------------------------------------------------ grouped attention

@contextlib.contextmanager
def sets_names(ops, L):
    """Record dfw_fsa_sets_kernel_name of every dfw_fsa_attention_sets call ops makes (and launch it)."""
    names, orig = [], ops._fsa_sets_call

    def rec(a, group):
        buf = C.create_string_buffer(96)
        L.check(L.lib().dfw_fsa_sets_kernel_name(C.byref(a), group, buf, 96), "dfw_fsa_sets_kernel_name")
        names.append(buf.value.decode())
        orig(a, group)

    ops._fsa_sets_call = rec
    try:
        yield names
    finally:
        ops._fsa_sets_call = orig


def _materialise(t, sets, b, s):
    """full[e*s + j] = bank[(e // b)*s + j] for the sets * b entries of a class-major batch."""
    idx = torch.tensor([(e // b) * s + j for e in range(sets * b) for j in range(s)], device=t.device)
    return t.index_select(0, idx)


SETS_CASES = [   # (id, sets, b, s, heads, n_q, n_bank)
    ("nw8_ragged", 3, 2, 2, 1, 1100, 1100),
    ("nw4_nbank321", 2, 3, 1, 2, 256, 321),
    ("split", 2, 1, 5, 2, 2048, 2048),
    ("xcd", 2, 2, 1, 4, 1024, 1024),
    ("sd21_64x64", 3, 2, 1, 5, 4096, 4096),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", SETS_CASES, ids=[c[0] for c in SETS_CASES])
def test_sets_equal_materialised_bank_exactly(ops, case, dtype):
    """fsa_attention_sets(..., group=b) is torch.equal to the unshared launch on the bank materialised per entry: same
    kernel, same key order, same split plan (both calls share every field) -- only the bank image index differs.  The sets
    are random and distinct, so an entry that read another set cannot pass.  Key split off and by default."""
    from diffews_amd import _lib as L
    cid, sets, b, s, heads, n_q, n_bank = case
    g = torch.Generator(device="cuda").manual_seed(21)
    B = sets * b
    q, k, v = _qkv(B, n_q, heads, dtype, g)
    kb, vb = _bank(sets * s, n_bank, heads, dtype, g)
    kf, vf = _materialise(kb, sets, b, s), _materialise(vb, sets, b, s)
    for key_split in (False, True):
        with sets_names(ops, L) as got:
            y = ops.fsa_attention_sets(q, k, v, heads, kb, vb, s, b, q_prescaled=True, key_split=key_split)
        with plans.fsa_names(ops, L) as want:
            ref = ops.fsa_attention(q, k, v, heads, kf, vf, nshot=s, q_prescaled=True, key_split=key_split)
        assert got[0] == want[0] + "+sets", (cid, key_split, got, want)
        assert ("+split" in got[0]) == (cid == "split" and key_split), (cid, key_split, got)
        if cid == "xcd":
            assert "+xcd" in got[0], got
        assert (",8,1," if n_q > 1024 else ",4,1,") in got[0], got
        assert torch.equal(y, ref), (cid, key_split, got, rel(y, ref))
    # a wrong divisor is visible in this data: the same call with the sets rotated differs
    if sets > 1:
        rot = ops.fsa_attention_sets(q, k, v, heads, kb.roll(s, 0), vb.roll(s, 0), s, b, q_prescaled=True)
        assert not torch.equal(rot, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_sets_group_one_and_group_batch(ops, dtype):
    """group == 1 is the ordinary two-pass read launch on the same bank; group == batch with one set is the +shared
    launch (every entry reads the same nshot images)."""
    g = torch.Generator(device="cuda").manual_seed(22)
    B, heads, N, s = 4, 2, 320, 2
    q, k, v = _qkv(B, N, heads, dtype, g)
    kb, vb = _bank(B * s, N, heads, dtype, g)
    one = ops.fsa_attention_sets(q, k, v, heads, kb, vb, s, 1, q_prescaled=True)
    assert torch.equal(one, ops.fsa_attention(q, k, v, heads, kb, vb, nshot=s, q_prescaled=True))
    al = ops.fsa_attention_sets(q, k, v, heads, kb[:s], vb[:s], s, B, q_prescaled=True)
    assert torch.equal(al, ops.fsa_attention(q, k, v, heads, kb[:s], vb[:s], nshot=s, q_prescaled=True, bank_shared=True))
    assert not torch.equal(al, one)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", SETS_CASES[:3], ids=[c[0] for c in SETS_CASES[:3]])
def test_sets_per_element_bound(ops, case, dtype):
    """Every output element and every lse of the sets launch against the fp64 reference and error allowance of
    tests/attention_bound.py, the key segments built from the materialised bank."""
    from diffews_amd import _lib as L
    cid, sets, b, s, heads, n_q, n_bank = case
    g = torch.Generator(device="cuda").manual_seed(23)
    B = sets * b
    q, k, v = _qkv(B, n_q, heads, dtype, g)
    kb, vb = _bank(sets * s, n_bank, heads, dtype, g)
    lse = torch.empty(B, heads, n_q, dtype=torch.float32, device="cuda")
    with sets_names(ops, L) as names:
        y = ops.fsa_attention_sets(q, k, v, heads, kb, vb, s, b, q_prescaled=True, lse=lse)
    name = names[0]
    assert name.endswith("+sets") and ("+split" in name) == (cid == "split"), name
    fcase = plans.Fsa(cid, B, heads, n_q, n_q, name, nshot=s, n_plain=0, n_bank=n_bank)
    inp = dict(q=q, k=k, v=v, kb=_materialise(kb, sets, b, s), vb=_materialise(vb, sets, b, s), lse=lse)
    w, wl = plans.fsa_check(fcase, dtype, inp, y, name.replace("+sets", ""), f"sets {cid}")
    print(f"[nway] {cid} {dtype}: {name}: worst out {w:.3f}, worst lse {wl:.3f} of the allowance")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_sets_bank_at_the_end_of_its_allocation(ops, dtype):
    """The bank descriptor spans (batch / group) * nshot images, not batch * nshot: a stack that is the LAST bytes of its
    allocation gives the result of the materialised bank."""
    g = torch.Generator(device="cuda").manual_seed(24)
    sets, b, s, heads, N = 2, 3, 2, 5, 1024
    C_ = heads * 64
    q, k, v = _qkv(sets * b, N, heads, dtype, g)
    big = torch.randn(3 * sets * s * N * 2 * C_, generator=g, device="cuda").to(dtype)
    kv = big[-sets * s * N * 2 * C_:].view(sets * s, N, 2 * C_)          # ends exactly where the allocation ends
    assert kv.data_ptr() + kv.numel() * kv.element_size() == big.data_ptr() + big.numel() * big.element_size()
    kb, vb = kv[..., :C_], kv[..., C_:]
    y = ops.fsa_attention_sets(q, k, v, heads, kb, vb, s, b, q_prescaled=True)
    ref = ops.fsa_attention(q, k, v, heads, _materialise(kb, sets, b, s), _materialise(vb, sets, b, s), nshot=s,
                            q_prescaled=True)
    assert torch.equal(y, ref)


# ------------------------------------------------------------------------------------------------ label fusion

def _masks(N, B, H, W, seed):
    """uint8 [N, B, 3, H, W] on the host: noise whose level differs per class and image (so maxima, thresholds and the
    winning class all vary), plus a smooth ramp that puts some pixels of every class below its threshold."""
    g = torch.Generator().manual_seed(seed)
    lvl = 0.6 + 0.4 * torch.rand(N, B, 1, 1, 1, generator=g)
    ramp = torch.linspace(0.0, 1.0, H * W).view(1, 1, 1, H, W)
    x = torch.rand(N, B, 3, H, W, generator=g) * lvl * (0.15 + 0.85 * ramp)
    return (x * 255).to(torch.uint8)


def _gt(N, B, H, W, seed):
    """uint8 [B, H, W]: labels 0..N, some ignore pixels (255) and some of a value above N (dropped as well)."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, N + 1, (B, H, W), generator=g).to(torch.uint8)
    r = torch.rand(B, H, W, generator=g)
    gt[r > 0.9] = 255
    gt[r < 0.05] = N + 1
    return gt


def _dev_labels(ops, u8, gt, flags, offset=0):
    """ops.seg_labels on the device copy of u8 (optionally placed `offset` bytes into its buffer), maxima computed from the
    bytes; returns host tensors."""
    N, B = u8.shape[:2]
    flat = torch.empty(u8.numel() + 16, dtype=torch.uint8, device="cuda")
    d = flat[offset:offset + u8.numel()].view(u8.shape)
    d.copy_(u8)
    assert d.is_contiguous() and d.data_ptr() % 4 == offset % 4
    mx = nway_ref.maxima(u8).cuda()
    lab, cnt = ops.seg_labels(d, mx, None if gt is None else gt.cuda(), *flags)
    return lab.cpu(), (None if cnt is None else cnt.cpu())


FLAGS = [(0.25, 0.0, False), (0.25, 0.0, True), (0.0, 0.3, False)]      # per-image dynamic, batch_max, fixed threshold


@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_seg_labels_bit_exact(ops, N, B):
    """labels and counts equal tests/nway_ref.py exactly: the word path (64 x 64), the scalar path (37 x 53: HW % 4 != 0)
    and the pointer fallback (64 x 64 one byte into its buffer), the three threshold modes, with and without gt."""
    for (H, W), offset in (((64, 64), 0), ((37, 53), 0), ((64, 64), 1)):
        u8, gt = _masks(N, B, H, W, seed=100 * N + B), _gt(N, B, H, W, seed=7 * N + B)
        for flags in FLAGS:
            want_l, want_c = nway_ref.seg_labels(u8, gt, *flags)
            lab, cnt = _dev_labels(ops, u8, gt, flags, offset)
            what = (N, B, H, W, offset, flags)
            assert torch.equal(lab, want_l), (what, int((lab != want_l).sum()))
            assert torch.equal(cnt, want_c), (what, cnt.tolist(), want_c.tolist())
            assert want_l.min() == 0 and want_l.max() >= 1, what                    # foreground and background both occur
            lab2, cnt2 = _dev_labels(ops, u8, None, flags, offset)
            assert cnt2 is None and torch.equal(lab2, want_l), what
        kept = (gt <= N).view(B, -1).sum(1)
        # every kept pixel is in exactly one pred bin and one gt bin: sum(union) + sum(inter) == 2 * kept
        assert torch.equal(want_c.sum((1, 2)), 2 * kept)


def test_seg_labels_ties_and_background(ops):
    """Class 0's planes copied into class 2: wherever they win, the label is 1, never 3 (lowest class on a tie).  Every
    class below the threshold: the label map is all background and the counts are the gt histogram."""
    N, B, H, W = 5, 3, 64, 64
    u8, gt = _masks(N, B, H, W, seed=9), _gt(N, B, H, W, seed=10)
    u8[2] = u8[0]
    for flags in FLAGS:
        want_l, want_c = nway_ref.seg_labels(u8, gt, *flags)
        lab, cnt = _dev_labels(ops, u8, gt, flags)
        assert torch.equal(lab, want_l) and torch.equal(cnt, want_c), flags
        assert (lab == 1).any() and not (lab == 3).any(), flags
    flags = (0.0, 1.0, False)                        # no score exceeds 1.0
    lab, cnt = _dev_labels(ops, u8, gt, flags)
    assert not lab.any()
    want_l, want_c = nway_ref.seg_labels(u8, gt, *flags)
    assert torch.equal(lab, want_l) and torch.equal(cnt, want_c)
    kept = (gt <= N).view(B, -1).sum(1)
    hist = torch.stack([torch.bincount(gt[i][gt[i] <= N].long(), minlength=N + 1) for i in range(B)])
    assert torch.equal(cnt[:, 0, 0], hist[:, 0]) and not cnt[:, 0, 1:].any()
    assert torch.equal(cnt[:, 1, 0], kept) and torch.equal(cnt[:, 1, 1:], hist[:, 1:])


@pytest.mark.parametrize("hw", [(64, 64), (37, 53)])
def test_seg_labels_one_class_is_seg_postprocess(ops, hw):
    """N == 1, on seg_postprocess' own output and the maxima it left in its scratch: counts[b] flattened is its
    {inter0, inter1, union0, union1} and labels is its prediction, in the three threshold modes; a second run into the same
    output buffers gives the same answer (counts are re-zeroed by the call)."""
    H, W = hw
    B = 3
    g = torch.Generator().manual_seed(4)
    x = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    x[1] *= 0.3
    gt = (torch.rand(B, H, W, generator=g) > 0.5).to(torch.uint8)
    gt[0][torch.rand(H, W, generator=g) > 0.9] = 255
    for flags in FLAGS:
        mx = torch.empty(B, dtype=torch.int32, device="cuda")
        u8, c4 = ops.seg_postprocess(x.cuda(), gt.cuda(), *flags, scratch=mx)
        labels = torch.full((B, H, W), 77, dtype=torch.uint8, device="cuda")
        counts = torch.full((B, 2, 2), -5, dtype=torch.int64, device="cuda")
        for _ in range(2):
            lab, cnt = ops.seg_labels(u8.view(1, B, 3, H, W), mx, gt.cuda(), *flags, labels_out=labels, counts_out=counts)
            assert lab is labels and cnt is counts
            assert torch.equal(cnt.view(B, 4), c4), (flags, cnt.tolist(), c4.tolist())
            pred = nway_ref.foreground(u8.cpu().view(1, B, 3, H, W), *flags)[0]
            assert torch.equal(lab.cpu().bool(), pred) and int(lab.max()) <= 1, flags
        assert torch.equal(mx.cpu(), nway_ref.maxima(u8.cpu().view(1, B, 3, H, W))[0])


# ------------------------------------------------------------------------------------------------ pipeline

N_CLS, B_Q, RES = 3, 2, 64


def _classes(s, seed):
    """N_CLS support sets: images and masks [N, s, 3, H, W] in [-1, 1]."""
    sets = [_support_set(s, RES, seed=seed + 10 * c) for c in range(N_CLS)]
    return torch.stack([a for a, _ in sets]), torch.stack([m for _, m in sets])


def _check_labels(r, gt):
    """labels / counts of a segment_classes result against nway_ref on the engine's OWN seg_u8, exactly."""
    want_l, want_c = nway_ref.seg_labels(r["seg_u8"].cpu(), None if gt is None else gt.cpu())
    assert r["labels"].dtype == torch.uint8 and torch.equal(r["labels"].cpu(), want_l)
    if gt is None:
        assert r["counts"] is None
    else:
        assert r["counts"].dtype == torch.int64 and torch.equal(r["counts"].cpu(), want_c)


@pytest.mark.parametrize("s", [1, 2])
def test_segment_classes_vs_oracle(models, s):
    """segment_classes(prepare_support_classes(sup, msk), qry) at 64 x 64, N = 3, b = 2.  Per class against
    oracle.pipeline.pipeline_call with that class' supports replicated: the bounds of test_segment_queries_vs_oracle (z0 <
    TOL_EP, mean |delta| of the decoded [0, 255] image < 1.0 fp16 / 4.0 bf16), and against segment_queries on .bank(c)
    within 1.5 x TOL_EP (two independently rounded evaluations).  labels and counts are nway_ref's on the engine's own seg_u8,
    exactly.  max_batch = 2 sends the classes through one at a time: z0 within 1.5 x TOL_EP of the unchunked call, labels
    exact against its own seg_u8."""
    from oracle import pipeline as op
    pipe, dt = models["pipe"], models["dt"]
    sup, msk = _classes(s, seed=200 + s)
    qry = _queries(B_Q, RES, seed=210 + s)
    gt = _gt(N_CLS, B_Q, RES, RES, seed=3).cuda()
    bankset = pipe.prepare_support_classes(sup.cuda(), msk.cuda())
    assert bankset.nsets == N_CLS and bankset.nshot == s
    h, w = bankset.hw
    r = pipe.segment_classes(bankset, qry.cuda(), gt)
    assert set(r) == {"z0", "dec", "seg_u8", "labels", "counts"}
    assert r["z0"].shape == (N_CLS, B_Q, 4, h, w) and r["dec"].shape == (N_CLS, B_Q, 3, RES, RES)
    assert r["seg_u8"].shape == (N_CLS, B_Q, 3, RES, RES) and r["labels"].shape == (B_Q, RES, RES)
    assert r["counts"].shape == (B_Q, 2, N_CLS + 1)
    for c in range(N_CLS):
        _, ref = op.pipeline_call(models["ou"], models["ov"], [_rep(sup[c], B_Q), qry, _rep(msk[c], B_Q)], models["te"])
        e_z0 = rel(r["z0"][c], ref["z0"])
        d_seg = float(((r["dec"][c].cpu() * 0.5 + 0.5) * 255 - ref["seg"]).abs().mean())
        one = pipe.segment_queries(bankset.bank(c), qry.cuda())
        e_one = rel(r["z0"][c], one["z0"])
        print(f"[nway] segment_classes s={s} class {c} {dt}: z0 vs oracle {e_z0:.3e}, decoded mean |d| {d_seg:.3f}, "
              f"z0 vs segment_queries {e_one:.3e}")
        assert e_z0 < TOL_EP[dt], e_z0
        assert d_seg < (1.0 if dt == torch.float16 else 4.0), d_seg
        assert e_one < 1.5 * TOL_EP[dt], e_one
    _check_labels(r, gt)
    assert pipe.segment_classes(bankset, qry.cuda())["counts"] is None
    z0 = r["z0"].clone()
    ch = pipe.segment_classes(bankset, qry.cuda(), gt, max_batch=2)
    e_ch = rel(ch["z0"], z0)
    print(f"[nway] segment_classes s={s} {dt}: chunked (max_batch 2) vs unchunked z0 {e_ch:.3e}")
    assert ch["z0"].shape == z0.shape and e_ch < 1.5 * TOL_EP[dt], e_ch
    _check_labels(ch, gt)
    for flags in (dict(batch_max=True), dict(r_threshold=0.0, threshold=0.3)):
        rf = pipe.segment_classes(bankset, qry.cuda(), gt, **flags)
        want_l, want_c = nway_ref.seg_labels(rf["seg_u8"].cpu(), gt.cpu(), flags.get("r_threshold", 0.25),
                                             flags.get("threshold", 0.0), flags.get("batch_max", False))
        assert torch.equal(rf["labels"].cpu(), want_l) and torch.equal(rf["counts"].cpu(), want_c), flags


def test_segment_classes_captured_equals_eager(models):
    """captured=True replays the same kernels: identical bits on every output, with and without ground truth; a second
    replay with other queries is that input's eager result; two sets of equal shape used alternately each give their own
    result (the set's uid is part of the graph key, its tensors are read in place); chunked capture too."""
    pipe = models["pipe"]
    pipe._graphs = {}
    gt = _gt(N_CLS, B_Q, RES, RES, seed=5).cuda()
    sets = [pipe.prepare_support_classes(*(t.cuda() for t in _classes(1, seed=300 + 50 * i))) for i in range(2)]
    keys = ("z0", "dec", "seg_u8", "labels", "counts")
    for use_gt in (gt, None):
        for seed in (1, 2):
            qry = _queries(B_Q, RES, 310 + seed).cuda()
            for st in (sets[seed % 2], sets[1 - seed % 2]):
                e = {k: (None if v is None else v.clone()) for k, v in pipe.segment_classes(st, qry, use_gt, captured=False).items()}
                c = pipe.segment_classes(st, qry, use_gt, captured=True)
                for k in keys:
                    assert (e[k] is None and c[k] is None) or torch.equal(e[k], c[k]), (seed, k, use_gt is None)
    assert len(pipe._graphs) == 4            # 2 sets x (gt, no gt), each captured once
    qry = _queries(B_Q, RES, 320).cuda()
    r0 = pipe.segment_classes(sets[0], qry, gt, captured=True)["z0"].clone()
    r1 = pipe.segment_classes(sets[1], qry, gt, captured=True)["z0"].clone()
    assert not torch.equal(r0, r1)
    pipe._graphs = {}
    e = {k: v.clone() for k, v in pipe.segment_classes(sets[0], qry, gt, max_batch=2, captured=False).items()}
    c = pipe.segment_classes(sets[0], qry, gt, max_batch=2, captured=True)
    for k in keys:
        assert torch.equal(e[k], c[k]), k
    # the query graphs of segment_queries and segment_classes share one bounded cache
    for i in range(pipe.MAX_QUERY_GRAPHS):
        pipe.segment_queries(sets[0].bank(i % N_CLS), _queries(1 + i, RES, 330 + i).cuda(), captured=True)
    assert sum(1 for k in pipe._graphs if k[0] == "queries") == pipe.MAX_QUERY_GRAPHS
    pipe._graphs = {}


def test_stale_set_raises(models):
    """A set used after the test timestep changed, or with queries of another H x W, raises ValueError on the host, eager
    and captured; back under its conditions it is valid again."""
    pipe = models["pipe"]
    sup, msk = _classes(1, seed=400)
    qry = _queries(B_Q, RES, 401).cuda()
    st = pipe.prepare_support_classes(sup.cuda(), msk.cuda())
    pipe.segment_classes(st, qry)
    try:
        pipe.test_timestep = 3
        for cap in (False, True):
            with pytest.raises(ValueError, match="fold key"):
                pipe.segment_classes(st, qry, captured=cap)
    finally:
        pipe.test_timestep = 1
    st = pipe.prepare_support_classes(sup.cuda(), msk.cuda())
    for cap in (False, True):
        with pytest.raises(ValueError, match=r"\(h, w\)"):
            pipe.segment_classes(st, _queries(1, 128, 402).cuda(), captured=cap)
    with pytest.raises(TypeError):
        pipe.segment_classes(st.bank(0), qry)
    assert torch.isfinite(pipe.segment_classes(st, qry)["z0"]).all()
    pipe._graphs = {}


def test_stacked_banks_equal_prepared_classes(models):
    """SupportBankSet.stack of per-class prepare_support banks against prepare_support_classes (one support pass over all
    N * s images): z0 within 1.5 x TOL_EP (two independently rounded evaluations), same shapes and bytes."""
    from diffews_amd.unet import SupportBankSet
    pipe, dt = models["pipe"], models["dt"]
    s = 2
    sup, msk = _classes(s, seed=500)
    qry = _queries(B_Q, RES, 501).cuda()
    whole = pipe.prepare_support_classes(sup.cuda(), msk.cuda())
    stacked = SupportBankSet.stack([pipe.prepare_support(sup[c].cuda(), msk[c].cuda()) for c in range(N_CLS)])
    assert stacked.nsets == whole.nsets and stacked.nshot == whole.nshot and stacked.nbytes() == whole.nbytes()
    a, b_ = pipe.segment_classes(whole, qry), pipe.segment_classes(stacked, qry)
    e = rel(b_["z0"], a["z0"])
    print(f"[nway] stacked banks vs prepare_support_classes {dt}: z0 {e:.3e}")
    assert e < 1.5 * TOL_EP[dt], e
    _check_labels(b_, None)
