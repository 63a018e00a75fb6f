"""GPU tests of ragged class banks -- N-way with a shot count of its own per class.

Attention: ops.fsa_attention_ragged per set against ops.fsa_attention on that set's slice of the stack (exact, key split
off), against ops.fsa_attention_sets with equal counts (exact, key split off and on), per element against the fp64 bound
of tests/attention_bound.py under the default plan, with the stack at the very end of its allocation.

Pipeline (tiny config, 64 x 64, N = 3, b = 2, shots (1, 3, 2)): prepare_support_classes(list, list) / segment_classes per
class against the fp32 oracle and against segment_queries on .bank(c), labels and counts exactly against tests/nway_ref.py,
chunked, captured, stacked from banks, at native sizes, and through evaluate_stream with unequal lists.

The oracle side relies on test_ragged_sets_cpu.test_oracle_definition_of_ragged_nway: the class-major batch of a ragged
set is, entry by entry, the reference's call with that class' own supports."""
import contextlib
import ctypes as C

import pytest
import torch

import nway_native_ref as nn
import nway_ref
import test_attention_plans_gpu as plans
from test_model_gpu import TOL_EP
from test_nway_gpu import sets_names, _check_labels, _gt
from test_nway_native_gpu import _gts, _same
from test_support_bank_gpu import models, ops, rel, _bank, _qkv, _queries, _rep, _support_set  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


# ------------------------------------------------------------------------------------------------ ragged attention

@contextlib.contextmanager
def ragged_names(ops, L):
    """Record dfw_fsa_ragged_kernel_name of every dfw_fsa_attention_ragged call ops makes (and launch it)."""
    names, orig = [], ops._fsa_ragged_call

    def rec(a, shots, nsets, group):
        buf = C.create_string_buffer(96)
        L.check(L.lib().dfw_fsa_ragged_kernel_name(C.byref(a), shots, nsets, group, buf, 96), "dfw_fsa_ragged_kernel_name")
        names.append(buf.value.decode())
        orig(a, shots, nsets, group)

    ops._fsa_ragged_call = rec
    try:
        yield names
    finally:
        ops._fsa_ragged_call = orig


RAGGED_CASES = [   # (id, shots, b, heads, n_q, n_bank)
    ("nw8_tail", (1, 3, 2), 2, 1, 1100, 1100),          # ragged last query block and key tile
    ("nw4_nbank321", (2, 1), 3, 2, 256, 321),           # 4-wave form, ragged bank tile
    ("xcd", (1, 2), 2, 4, 1024, 1024),                  # the XCD re-map
    ("split", (5, 3), 1, 2, 2048, 2048),                # must take a key split with unequal counts
    ("sd21_64x64", (1, 2, 1), 2, 5, 4096, 4096),        # the UNet's 64^2-level shape
]
CASE_IDS = [c[0] for c in RAGGED_CASES]


def _offsets(shots):
    off = [0]
    for s in shots:
        off.append(off[-1] + s)
    return off


def _inputs(case, dtype, seed):
    cid, shots, b, heads, n_q, n_bank = case
    g = torch.Generator(device="cuda").manual_seed(seed)
    q, k, v = _qkv(len(shots) * b, n_q, heads, dtype, g)
    kb, vb = _bank(sum(shots), n_bank, heads, dtype, g)       # random and distinct sets
    return q, k, v, kb, vb


def _per_set(ops, q, k, v, heads, kb, vb, shots, b):
    """The unsplit reference: every set's entries through ops.fsa_attention on that set's slice of the stack."""
    off, out = _offsets(shots), []
    for j, s in enumerate(shots):
        e = slice(j * b, (j + 1) * b)
        out.append(ops.fsa_attention(q[e], k[e], v[e], heads, kb[off[j]:off[j] + s], vb[off[j]:off[j] + s], nshot=s,
                                     q_prescaled=True, bank_shared=True, key_split=False))
    return torch.cat(out)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", RAGGED_CASES, ids=CASE_IDS)
def test_ragged_equals_per_set_launches_exactly(ops, case, dtype):
    """key_split=False: every set's entries of the ragged launch are torch.equal to fsa_attention on that set's slice
    (bank_shared, unsplit) -- same kernel arithmetic, key order and tile sequence.  The same call with the counts in
    another order (same total, so only a wrong `first` or count shows) must differ."""
    from diffews_amd import _lib as L
    cid, shots, b, heads, n_q, n_bank = case
    q, k, v, kb, vb = _inputs(case, dtype, 31)
    with ragged_names(ops, L) as got:
        y = ops.fsa_attention_ragged(q, k, v, heads, kb, vb, shots, b, q_prescaled=True, key_split=False)
    assert got[0].endswith("+ragged") and "+split" not in got[0], got
    assert (",8,1," if n_q > 1024 else ",4,1,") in got[0], got
    if cid == "xcd":
        assert "+xcd" in got[0], got
    ref = _per_set(ops, q, k, v, heads, kb, vb, shots, b)
    for j in range(len(shots)):
        e = slice(j * b, (j + 1) * b)
        assert torch.equal(y[e], ref[e]), (cid, j, got, rel(y[e], ref[e]))
    other = tuple(reversed(shots))
    if other == shots:                       # a palindrome: rotate instead
        other = shots[1:] + shots[:1]
    assert other != shots and sum(other) == sum(shots)
    wrong = ops.fsa_attention_ragged(q, k, v, heads, kb, vb, other, b, q_prescaled=True, key_split=False)
    assert not torch.equal(wrong, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", [("nw8_tail", 3, 2, 2, 1, 1100, 1100), ("nw4_nbank321", 2, 3, 1, 2, 256, 321),
                                  ("split", 2, 1, 5, 2, 2048, 2048), ("xcd", 2, 2, 1, 4, 1024, 1024)],
                         ids=["nw8_tail", "nw4_nbank321", "split", "xcd"])
def test_ragged_with_equal_counts_is_the_sets_launch(ops, case, dtype):
    """With equal counts fsa_attention_ragged is torch.equal to fsa_attention_sets, key split off and on (the same plan);
    the names differ only in the suffix."""
    from diffews_amd import _lib as L
    cid, sets, b, s, heads, n_q, n_bank = case
    g = torch.Generator(device="cuda").manual_seed(32)
    q, k, v = _qkv(sets * b, n_q, heads, dtype, g)
    kb, vb = _bank(sets * s, n_bank, heads, dtype, g)
    for key_split in (False, True):
        with ragged_names(ops, L) as got:
            y = ops.fsa_attention_ragged(q, k, v, heads, kb, vb, (s,) * sets, b, q_prescaled=True, key_split=key_split)
        with sets_names(ops, L) as want:
            ref = ops.fsa_attention_sets(q, k, v, heads, kb, vb, s, b, q_prescaled=True, key_split=key_split)
        assert want[0].endswith("+sets") and got[0] == want[0][:-len("+sets")] + "+ragged", (cid, key_split, got, want)
        assert ("+split" in got[0]) == (cid == "split" and key_split), (cid, key_split, got)
        assert torch.equal(y, ref), (cid, key_split, got, rel(y, ref))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", RAGGED_CASES[:4], ids=CASE_IDS[:4])
def test_ragged_per_element_bound(ops, case, dtype):
    """Default plan (key_split=True): every output element and every lse, per set on that set's entries, against the fp64
    reference and error allowance of tests/attention_bound.py with that set's bank materialised per entry.  `split` takes
    a key split with unequal counts: its result is not bit-equal to the unsplit one, and both pass the bound."""
    from diffews_amd import _lib as L
    cid, shots, b, heads, n_q, n_bank = case
    q, k, v, kb, vb = _inputs(case, dtype, 33)
    B, off = len(shots) * b, _offsets(shots)

    def run(key_split):
        lse = torch.empty(B, heads, n_q, dtype=torch.float32, device="cuda")
        with ragged_names(ops, L) as names:
            y = ops.fsa_attention_ragged(q, k, v, heads, kb, vb, shots, b, q_prescaled=True, lse=lse, key_split=key_split)
        return y, lse, names[0]

    def bound(y, lse, name, what):
        worst = [0.0, 0.0]
        for j, s in enumerate(shots):
            e = slice(j * b, (j + 1) * b)
            fcase = plans.Fsa(cid, b, heads, n_q, n_q, name, nshot=s, n_plain=0, n_bank=n_bank)
            inp = dict(q=q[e], k=k[e], v=v[e], kb=kb[off[j]:off[j] + s].repeat(b, 1, 1),
                       vb=vb[off[j]:off[j] + s].repeat(b, 1, 1), lse=lse[e])
            w, wl = plans.fsa_check(fcase, dtype, inp, y[e], name.replace("+ragged", ""), f"ragged {cid} set {j} {what}")
            worst = [max(worst[0], w), max(worst[1], wl)]
        print(f"[ragged] {cid} {dtype} {what}: {name}: worst out {worst[0]:.3f}, worst lse {worst[1]:.3f} of the allowance")

    y, lse, name = run(True)
    assert name.endswith("+ragged") and ("+split" in name) == (cid == "split"), name
    bound(y, lse, name, "default plan")
    if cid == "split":
        nsplit = int(name.split("+split")[1].split("+")[0])
        assert 2 <= nsplit <= 1 + min(shots), name
        y0, lse0, name0 = run(False)
        assert "+split" not in name0 and not torch.equal(y, y0), (name, name0)
        bound(y0, lse0, name0, "unsplit")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_ragged_stack_at_the_end_of_its_allocation(ops, dtype):
    """The bank descriptor spans exactly sum(shots) images: a stack that is the LAST bytes of its allocation gives the
    unsplit per-set result (a read past it would fault, an index past it would read zeros)."""
    from diffews_amd import _lib as L
    g = torch.Generator(device="cuda").manual_seed(34)
    shots, b, heads, N = (1, 3, 2), 3, 5, 1024
    C_, tot = heads * 64, sum(shots)
    q, k, v = _qkv(len(shots) * b, N, heads, dtype, g)
    big = torch.randn(3 * tot * N * 2 * C_, generator=g, device="cuda").to(dtype)
    kv = big[-tot * N * 2 * C_:].view(tot, N, 2 * C_)          # ends exactly where the allocation ends
    assert kv.data_ptr() + kv.numel() * kv.element_size() == big.data_ptr() + big.numel() * big.element_size()
    kb, vb = kv[..., :C_], kv[..., C_:]
    with ragged_names(ops, L) as names:
        y = ops.fsa_attention_ragged(q, k, v, heads, kb, vb, shots, b, q_prescaled=True)
    assert names[0].endswith("+ragged") and "+split" not in names[0], names       # short rows: the default plan is unsplit
    assert torch.equal(y, _per_set(ops, q, k, v, heads, kb, vb, shots, b))


# ------------------------------------------------------------------------------------------------ pipeline

SHOTS, B_Q, RES = (1, 3, 2), 2, 64
N_CLS = len(SHOTS)
FLAGS = [dict(), dict(batch_max=True), dict(r_threshold=0.0, threshold=0.3)]     # the three threshold modes


def _classes(seed, shots=SHOTS):
    """One support set per class: two lists of [s_c, 3, H, W] images and masks in [-1, 1] (host)."""
    sets = [_support_set(s, RES, seed=seed + 10 * c) for c, s in enumerate(shots)]
    return [a for a, _ in sets], [m for _, m in sets]


def _cuda(ts):
    return [t.cuda() for t in ts]


def _labels_exact(r, gt, flags):
    want_l, want_c = nway_ref.seg_labels(r["seg_u8"].cpu(), gt.cpu(), flags.get("r_threshold", 0.25),
                                         flags.get("threshold", 0.0), flags.get("batch_max", False))
    assert torch.equal(r["labels"].cpu(), want_l) and torch.equal(r["counts"].cpu(), want_c), flags


def test_segment_classes_ragged_vs_oracle(models):
    """segment_classes(prepare_support_classes(list, list), qry).  Per class against oracle.pipeline.pipeline_call with that
    class' own supports replicated: the bounds of test_segment_classes_vs_oracle (z0 < TOL_EP, mean |delta| of the decoded
    [0, 255] image < 1.0 fp16 / 4.0 bf16), and against segment_queries on .bank(c) within 1.5 x TOL_EP.  labels and counts
    are nway_ref's on the engine's own seg_u8, exactly, in the three threshold modes, unchunked and one class per chunk."""
    from oracle import pipeline as op
    pipe, dt = models["pipe"], models["dt"]
    sup, msk = _classes(seed=800)
    qry = _queries(B_Q, RES, seed=810)
    gt = _gt(N_CLS, B_Q, RES, RES, seed=3).cuda()
    bankset = pipe.prepare_support_classes(_cuda(sup), _cuda(msk))
    assert bankset.ragged and bankset.shots == SHOTS and bankset.nsets == N_CLS and bankset.nshot is None
    assert bankset.k[0].shape[0] == sum(SHOTS)
    h, w = bankset.hw
    r = pipe.segment_classes(bankset, qry.cuda(), gt)
    assert set(r) == {"z0", "dec", "seg_u8", "labels", "counts"}
    assert r["z0"].shape == (N_CLS, B_Q, 4, h, w) and r["dec"].shape == (N_CLS, B_Q, 3, RES, RES)
    assert r["seg_u8"].shape == (N_CLS, B_Q, 3, RES, RES) and r["labels"].shape == (B_Q, RES, RES)
    for c in range(N_CLS):
        _, ref = op.pipeline_call(models["ou"], models["ov"], [_rep(sup[c], B_Q), qry, _rep(msk[c], B_Q)], models["te"])
        e_z0 = rel(r["z0"][c], ref["z0"])
        d_seg = float(((r["dec"][c].cpu() * 0.5 + 0.5) * 255 - ref["seg"]).abs().mean())
        bank = bankset.bank(c)
        assert bank.nshot == SHOTS[c]
        one = pipe.segment_queries(bank, qry.cuda())
        e_one = rel(r["z0"][c], one["z0"])
        print(f"[ragged] segment_classes class {c} (s = {SHOTS[c]}) {dt}: z0 vs oracle {e_z0:.3e}, decoded mean |d| "
              f"{d_seg:.3f}, z0 vs segment_queries {e_one:.3e}")
        assert e_z0 < TOL_EP[dt], e_z0
        assert d_seg < (1.0 if dt == torch.float16 else 4.0), d_seg
        assert e_one < 1.5 * TOL_EP[dt], e_one
    _check_labels(r, gt)
    assert pipe.segment_classes(bankset, qry.cuda())["counts"] is None
    z0 = r["z0"].clone()
    for max_batch in (16, 2):
        for flags in FLAGS:
            rf = pipe.segment_classes(bankset, qry.cuda(), gt, max_batch=max_batch, **flags)
            _labels_exact(rf, gt, flags)
            e_ch = rel(rf["z0"], z0)
            assert rf["z0"].shape == z0.shape and e_ch < 1.5 * TOL_EP[dt], (max_batch, e_ch)


def test_ragged_captured_equals_eager(models):
    """captured=True replays the same kernels: identical bits on every output, unchunked and chunked; a ragged set and a
    uniform set of the same number of images, used alternately, each give their own result (the uid is in the graph key and
    the table of counts rides in the captured kernel arguments)."""
    pipe = models["pipe"]
    pipe._graphs = {}
    gt = _gt(N_CLS, B_Q, RES, RES, seed=5).cuda()
    sup, msk = _classes(seed=820)
    ragged = pipe.prepare_support_classes(_cuda(sup), _cuda(msk))
    flat_s, flat_m = torch.cat(sup).cuda(), torch.cat(msk).cuda()              # the same 6 images as 3 classes of 2
    uniform = pipe.prepare_support_classes(flat_s.view(N_CLS, 2, *flat_s.shape[1:]), flat_m.view(N_CLS, 2, *flat_m.shape[1:]))
    assert ragged.ragged and not uniform.ragged and uniform.nshot == 2
    assert ragged.k[0].shape == uniform.k[0].shape and ragged.nbytes() == uniform.nbytes()
    keys = ("z0", "dec", "seg_u8", "labels", "counts")
    try:
        for max_batch in (16, 2):
            eager = {}
            for seed in (1, 2):
                qry = _queries(B_Q, RES, 830 + seed).cuda()
                for st in ((ragged, uniform) if seed == 1 else (uniform, ragged)):
                    e = {k: v.clone() for k, v in pipe.segment_classes(st, qry, gt, max_batch=max_batch, captured=False).items()}
                    c = pipe.segment_classes(st, qry, gt, max_batch=max_batch, captured=True)
                    for k in keys:
                        assert torch.equal(e[k], c[k]), (max_batch, seed, st.ragged, k)
                    eager[(seed, st.ragged)] = e["z0"]
            for seed in (1, 2):
                assert not torch.equal(eager[(seed, True)], eager[(seed, False)])
            assert len(pipe._graphs) == 2            # each set captured once, replayed for the second batch of queries
            pipe._graphs = {}
    finally:
        pipe._graphs = {}


def test_stacked_ragged_banks_equal_prepared_classes(models):
    """SupportBankSet.stack of per-class prepare_support banks, ragged=True, against the one support pass over all
    sum(shots) images: z0 within 1.5 x TOL_EP (two independently rounded evaluations), equal bytes."""
    from diffews_amd.unet import SupportBankSet
    pipe, dt = models["pipe"], models["dt"]
    sup, msk = _classes(seed=840)
    qry = _queries(B_Q, RES, 841).cuda()
    whole = pipe.prepare_support_classes(_cuda(sup), _cuda(msk))
    banks = [pipe.prepare_support(sup[c].cuda(), msk[c].cuda()) for c in range(N_CLS)]
    with pytest.raises(ValueError, match="nshot"):
        SupportBankSet.stack(banks)
    stacked = SupportBankSet.stack(banks, ragged=True)
    assert stacked.ragged and stacked.shots == whole.shots == SHOTS and stacked.nbytes() == whole.nbytes()
    a, b_ = pipe.segment_classes(whole, qry), pipe.segment_classes(stacked, qry)
    e = rel(b_["z0"], a["z0"])
    print(f"[ragged] stacked banks vs prepare_support_classes {dt}: z0 {e:.3e}")
    assert e < 1.5 * TOL_EP[dt], e
    _check_labels(b_, None)


def test_uniform_sets_keep_their_launch_and_ragged_sets_take_theirs(models):
    """A uniform set launches only names ending in +sets (and never the ragged entry point); a ragged set only names
    ending in +ragged (and never the sets entry point), unchunked and one class per chunk."""
    from diffews_amd import _lib as L
    from diffews_amd import ops as O
    pipe = models["pipe"]
    sup, msk = _classes(seed=850)
    ragged = pipe.prepare_support_classes(_cuda(sup), _cuda(msk))
    us, um = _classes(seed=851, shots=(2, 2, 2))
    uniform = pipe.prepare_support_classes(torch.stack(us).cuda(), torch.stack(um).cuda())
    qry = _queries(B_Q, RES, 852).cuda()
    layers = len(ragged.k)
    for max_batch, launches in ((16, layers), (2, N_CLS * layers)):
        with sets_names(O, L) as s_names, ragged_names(O, L) as r_names:
            pipe.segment_classes(uniform, qry, max_batch=max_batch, captured=False)
        assert len(s_names) == launches and not r_names and all(n.endswith("+sets") for n in s_names), (s_names, r_names)
        with sets_names(O, L) as s_names, ragged_names(O, L) as r_names:
            pipe.segment_classes(ragged, qry, max_batch=max_batch, captured=False)
        assert len(r_names) == launches and not s_names and all(n.endswith("+ragged") for n in r_names), (s_names, r_names)


def test_segment_classes_ragged_native(models):
    """segment_classes(ragged, qry, native=t, class_ids=...) at two native sizes: r["native"] equals nway_native_ref on the
    call's own seg_u8 exactly (labels, maxima, counts), eager and captured; every other entry is the call without it."""
    from diffews_amd.input_pipeline import NativeTargets
    pipe = models["pipe"]
    pipe._graphs = {}
    ids = [7, 3, 9]
    sup, msk = _classes(seed=860)
    bankset = pipe.prepare_support_classes(_cuda(sup), _cuda(msk))
    sizes = [(48, 64), (97, 131)]
    gts = _gts(N_CLS, sizes, "ids8", 61)
    t = NativeTargets((RES, RES), sizes, gt=gts, ignore_value=255)
    qry = _queries(B_Q, RES, 861).cuda()
    try:
        for captured in (False, True):
            plain = {k: (None if v is None else v.clone()) for k, v in pipe.segment_classes(bankset, qry, captured=captured).items()}
            r = pipe.segment_classes(bankset, qry, captured=captured, native=t, class_ids=ids)
            assert set(r) == set(plain) | {"native"}
            for k in plain:
                assert (plain[k] is None and r[k] is None) or torch.equal(plain[k], r[k]), (captured, k)
            ref = nn.nway_native_ref(r["seg_u8"].cpu(), sizes, gts, ids, 255, 0.25, 0.0, False)
            _same(r["native"], ref, (sizes, captured))
            assert [tuple(x.shape) for x in r["native"]["labels"]] == sizes
    finally:
        pipe._graphs = {}


def test_evaluate_stream_with_unequal_lists(models):
    """evaluate_stream with N-way lists of 1, 3 and 2 examples (decoded images in, through segment_stream, which routes the
    ragged set to segment_classes) returns the counts of evaluate_class_set under use_original_imgsize with class_ids, fed
    the list form of the hand-built tensors and the same queries."""
    from diffews_amd import _lib as L
    from diffews_amd import evaluate
    from diffews_amd import ops as O
    from diffews_amd.input_pipeline import DeviceImageTransform, NativeTargets
    import test_query_loader_gpu as ql
    pipe = models["pipe"]
    pipe._graphs = {}
    tf = DeviceImageTransform(RES)
    ids = ql.CLASS_IDS
    n, b = 5, 2
    qs = ql._host_queries(n, seed=43)
    simg, smap = ql._host_supports(ids, max(SHOTS), seed=6)
    simg = [ims[:s] for ims, s in zip(simg, SHOTS)]
    smap = [mps[:s] for mps, s in zip(smap, SHOTS)]
    sup = [torch.stack([tf.image(im) for im in ims]) for ims in simg]
    msk = [torch.stack([tf.mask(m, c - 1)[0] for m in mps]) for mps, c in zip(smap, ids)]
    assert [t.shape[0] for t in sup] == list(SHOTS)
    hand = ql._hand_batches(tf, qs, b)
    batches = [(qry, NativeTargets((RES, RES), szs, gt=gts, ignore_value=255)) for qry, _, gts, szs in hand]
    try:
        miou, iou, total = evaluate.evaluate_class_set(pipe, sup, msk, batches, captured=False, use_original_imgsize=True,
                                                       class_ids=ids)
        with sets_names(O, L) as s_names, ragged_names(O, L) as r_names:
            g_miou, g_iou, g_total = evaluate.evaluate_stream(pipe, simg, smap, class_ids=ids, queries=qs, size=RES, batch=b,
                                                              depth=1, captured=False, ignore_value=255)
        assert r_names and not s_names and all(x.endswith("+ragged") for x in r_names)
        assert g_total.dtype == torch.int64 and g_total.shape == (2, N_CLS + 1)
        assert torch.equal(g_total, total) and int(total[1].sum()) > 0
        assert torch.equal(g_iou, iou)
        assert abs(float(g_miou) - float(miou)) <= 2 * N_CLS * 2.0 ** -53 * float(miou), (g_miou, miou)
        with pytest.raises(ValueError):              # a class without examples, a class with fewer maps than images
            evaluate.evaluate_stream(pipe, [simg[0], [], simg[2]], [smap[0], [], smap[2]], class_ids=ids, queries=qs, size=RES)
        with pytest.raises(ValueError):
            evaluate.evaluate_stream(pipe, simg, [smap[0], smap[1][:2], smap[2]], class_ids=ids, queries=qs, size=RES)
    finally:
        pipe._graphs = {}
