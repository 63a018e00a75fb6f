"""CPU tests (no GPU) of ragged class banks -- N-way with a shot count of its own per class: the three entry points of
the ragged sets launch through the header, the ctypes table and the host-only queries (validation, kernel name, key-split
plan, workspace); the SupportBankSet handle with a count per set on host tensors; the definition of the feature in the
oracle's arithmetic, which tests/test_ragged_sets_gpu.py leans on."""
import ctypes as C
import os
import re

import pytest
import torch

import test_nway_cpu as nw
import test_support_bank_cpu as sb

DFW_EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shots(counts):
    return (C.c_int32 * len(counts))(*counts)


def _ragged_name(L, a, counts, group):
    buf = C.create_string_buffer(96)
    L.check(L.lib().dfw_fsa_ragged_kernel_name(C.byref(a), _shots(counts), len(counts), group, buf, 96),
            "dfw_fsa_ragged_kernel_name")
    return buf.value.decode()


def _ragged_args(L, counts, group, workspace=True, **kw):
    """Host-only arguments of a ragged launch of len(counts) sets x group entries; with `workspace`, the one the library
    asks for (so that the name shows the split plan)."""
    a = sb._fsa_args(L, batch=len(counts) * group, nshot=max(counts), **kw)
    if workspace:
        nb = L.lib().dfw_fsa_ragged_workspace_bytes(C.byref(a), _shots(counts), len(counts), group)
        if nb:
            a.workspace, a.workspace_bytes = 4096, nb
    return a


def test_header_ctypes_and_symbols(hip_lib):
    """The three entry points are declared with the issue's signatures, bound in _lib.SYMBOLS with matching argument lists
    and exported; dfw_fsa_args is untouched (bank_shared still its last field)."""
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int dfw_fsa_attention_ragged(const dfw_fsa_args* a, const int32_t* shots, int32_t nsets, int32_t group, "
            "dfw_stream_t stream);") in flat
    assert ("int dfw_fsa_ragged_kernel_name(const dfw_fsa_args* a, const int32_t* shots, int32_t nsets, int32_t group, "
            "char* buf, size_t n);") in flat
    assert ("size_t dfw_fsa_ragged_workspace_bytes(const dfw_fsa_args* a, const int32_t* shots, int32_t nsets, "
            "int32_t group);") in flat
    i32, vp, pi = C.c_int32, C.c_void_p, C.POINTER(C.c_int32)
    assert L.SYMBOLS["dfw_fsa_attention_ragged"] == (i32, [C.POINTER(L.FsaArgs), pi, i32, i32, vp])
    assert L.SYMBOLS["dfw_fsa_ragged_kernel_name"] == (i32, [C.POINTER(L.FsaArgs), pi, i32, i32, C.c_char_p, C.c_size_t])
    assert L.SYMBOLS["dfw_fsa_ragged_workspace_bytes"] == (C.c_size_t, [C.POINTER(L.FsaArgs), pi, i32, i32])
    for name in ("dfw_fsa_attention_ragged", "dfw_fsa_ragged_kernel_name", "dfw_fsa_ragged_workspace_bytes"):
        assert getattr(hip_lib, name) is not None
    assert L.FsaArgs._fields_[-1] == ("bank_shared", i32)


def test_host_validation(hip_lib):
    """Everything that is not a ragged sets launch is DFW_EINVAL from the launch and the name query (0 bytes from the
    workspace query), on the host, before any launch -- safe without a GPU."""
    from diffews_amd import _lib as L
    h = L.lib()
    buf = C.create_string_buffer(96)
    ok = dict(batch=6, heads=2, n_q=128, n_kv=128, n_bank=128, nshot=3)
    a = sb._fsa_args(L, **ok)
    assert h.dfw_fsa_ragged_kernel_name(C.byref(a), _shots([1, 3, 2]), 3, 2, buf, 96) == 0
    assert h.dfw_fsa_ragged_kernel_name(C.byref(a), _shots([3, 1]), 2, 3, buf, 96) == 0
    s64 = [1] * 63 + [2]
    a64 = sb._fsa_args(L, **dict(ok, batch=64, nshot=2))
    assert h.dfw_fsa_ragged_kernel_name(C.byref(a64), _shots(s64), 64, 1, buf, 96) == 0      # 64 sets: the most
    bad = [
        ("null shots", ok, None, 3, 2),
        ("a count of 0", ok, [1, 3, 0], 3, 2),
        ("a negative count", ok, [3, -1, 2], 3, 2),
        ("nsets != batch / group", ok, [1, 3], 2, 2),
        ("nsets != batch / group (more)", ok, [1, 3, 2, 1], 4, 2),
        ("nsets 0", ok, [1, 3, 2], 0, 2),
        ("batch % group != 0", ok, [3], 1, 4),
        ("group 0", ok, [1, 3, 2], 3, 0),
        ("group < 0", ok, [1, 3, 2], 3, -2),
        ("n_plain > 0", dict(ok, n_plain=2), [1, 3, 2], 3, 2),
        ("bank_shared", dict(ok, bank_shared=1), [1, 3, 2], 3, 2),
        ("nshot above max(shots)", dict(ok, nshot=4), [1, 3, 2], 3, 2),
        ("nshot below max(shots)", dict(ok, nshot=2), [1, 3, 2], 3, 2),
        ("nshot 0", dict(ok, nshot=0, n_bank=0), [1, 3, 2], 3, 2),
        ("65 sets", dict(ok, batch=65, nshot=2), [1] * 64 + [2], 65, 1),
    ]
    for what, fields, counts, nsets, group in bad:
        a = sb._fsa_args(L, **fields)
        sh = None if counts is None else _shots(counts)
        assert h.dfw_fsa_attention_ragged(C.byref(a), sh, nsets, group, None) == DFW_EINVAL, what
        assert h.dfw_fsa_ragged_kernel_name(C.byref(a), sh, nsets, group, buf, 96) == DFW_EINVAL, what
        assert h.dfw_fsa_ragged_workspace_bytes(C.byref(a), sh, nsets, group) == 0, what
    from diffews_amd import ops
    q = torch.zeros(4, 128, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"fsa_attention: k_bank must hold 3 images \(the sum of shots\), got 4"):     # ops: the stack holds exactly sum(shots) images
        ops.fsa_attention_ragged(q, q, q, 2, q[:4], q[:4], shots=(1, 2), group=2)
    with pytest.raises(ValueError):
        ops.fsa_attention_ragged(q, q, q, 2, q[:3], q[:3], shots=(3, 0), group=2)
    with pytest.raises(ValueError):
        ops.fsa_attention_ragged(q, q, q, 2, q[:3], q[:3], shots=(1, 1, 1), group=2)


def test_equal_counts_are_the_sets_plan(hip_lib):
    """With all counts equal the ragged launch is the sets launch: for every bank-reading n_plain == 0 key of the recorded
    parent names and every group that divides its batch, the name is the sets name with +ragged for +sets and the
    workspace is dfw_fsa_workspace_bytes."""
    from diffews_amd import _lib as L
    seen, n = set(), 0
    for key, want in sb.PARENT_NAMES.items():
        dtype, pre, batch, heads, ntok, nshot, n_plain, ws = key
        if n_plain or not nshot:
            continue
        for group in (1, 2, 4, batch):
            if batch % group or batch // group > 64:
                continue
            for dt in (L.BF16, L.F16):
                a = sb._args_of(L, (dt,) + key[1:])
                counts = [nshot] * (batch // group)
                name = _ragged_name(L, a, counts, group)
                sets = nw._sets_name(L, a, group)
                assert name.endswith("+ragged") and name == sets[:-len("+sets")] + "+ragged", (key, group, name, sets)
                assert L.lib().dfw_fsa_ragged_workspace_bytes(C.byref(a), _shots(counts), len(counts), group) == \
                    L.lib().dfw_fsa_workspace_bytes(C.byref(a)), (key, group)
                seen.add(name)
                n += 1
    assert n >= 40
    assert any("+split" in s for s in seen) and any("+xcd" in s for s in seen)
    assert any(",8,1," in s for s in seen) and any(",4,1," in s for s in seen)


def _nsplit(name):
    return int(re.search(r"\+split(\d+)", name).group(1)) if "+split" in name else 1


def test_split_plan_is_clamped_to_the_shortest_set(hip_lib):
    """The split never exceeds 1 + min(shots): (5, 5) at 2048 tokens takes the sets plan (more than two splits), (5, 1) at
    most +split2, (5, 3) at most +split4 and still a split (the GPU test's `split` case); the workspace is 0 exactly when
    the name has no +split, and is the partial buffer of the split the name shows."""
    from diffews_amd import _lib as L
    shape = dict(heads=2, n_q=2048, n_kv=2048, n_bank=2048)
    for dt in (L.BF16, L.F16):
        uni = _ragged_name(L, _ragged_args(L, [5, 5], 1, dtype=dt, **shape), [5, 5], 1)
        a = _ragged_args(L, [5, 5], 1, dtype=dt, **shape)
        assert uni == nw._sets_name(L, a, 1)[:-len("+sets")] + "+ragged" and _nsplit(uni) > 2, uni
        assert 1 <= _nsplit(_ragged_name(L, _ragged_args(L, [5, 1], 1, dtype=dt, **shape), [5, 1], 1)) <= 2
        assert 1 <= _nsplit(_ragged_name(L, _ragged_args(L, [1, 5], 1, dtype=dt, **shape), [1, 5], 1)) <= 2
        assert 2 <= _nsplit(_ragged_name(L, _ragged_args(L, [5, 3], 1, dtype=dt, **shape), [5, 3], 1)) <= 4
    cases = [([5, 3], 1, shape), ([5, 1], 1, shape), ([1, 1], 2, shape), ([1, 3, 2], 2, dict(heads=1, n_q=1100, n_kv=1100, n_bank=1100)),
             ([7, 7, 2], 1, dict(heads=5, n_q=4096, n_kv=4096, n_bank=4096)), ([2, 1], 3, dict(heads=2, n_q=256, n_kv=256, n_bank=321))]
    some = set()
    for counts, group, shp in cases:
        a = _ragged_args(L, counts, group, workspace=False, **shp)
        nb = L.lib().dfw_fsa_ragged_workspace_bytes(C.byref(a), _shots(counts), len(counts), group)
        assert "+split" not in _ragged_name(L, a, counts, group)            # no workspace passed: unsplit
        a = _ragged_args(L, counts, group, **shp)
        name = _ragged_name(L, a, counts, group)
        assert (nb == 0) == ("+split" not in name), (counts, name, nb)
        assert _nsplit(name) <= 1 + min(counts), (counts, name)
        if nb:
            assert nb == a.batch * _nsplit(name) * a.heads * a.n_q * 68 * 4, (counts, name, nb)
        some.add(nb != 0)
    assert some == {True, False}


def test_ragged_support_bank_set_handle():
    """SupportBankSet with a count per set, on host tensors: shots / offsets / ragged, nshot is None, .bank(c) slices the
    stack at the prefix sums (zero-copy, the same handle on every call, its own nshot), nbytes; a count list of the wrong
    length and a stack of another image count raise; stack(banks) keeps its nshot error, stack(banks, ragged=True) accepts
    differing nshot and names the first other mismatch; a uniform set gains the same fields."""
    from diffews_amd import config
    from diffews_amd.unet import SupportBank, SupportBankSet, bank_layout
    cfg = config.get("tiny_unet")
    dt, hw, shots = torch.bfloat16, (8, 8), (1, 3, 2)
    N, tot = len(shots), sum(shots)
    layout = bank_layout(cfg, *hw)
    key = (1.0, "folded", 1)

    def kv(n_img, layout=layout, dtype=dt):
        return [torch.randn(n_img, n, c).to(dtype) for n, c in layout]

    k, v = kv(tot), kv(tot)
    st = SupportBankSet(k, v, N, shots, hw, dt, dt, key, 1, layout)
    assert st.nsets == N and st.shots == (1, 3, 2) and isinstance(st.shots, tuple) and st.offsets == (0, 1, 4, 6)
    assert st.ragged is True and st.nshot is None
    assert st.nbytes() == 2 * 2 * tot * sum(n * c for n, c in layout)
    assert SupportBankSet(k, v, N, list(shots), hw, dt, dt, key, 1, layout).shots == shots
    st.check(hw=hw, dtype=dt, residual_dtype=dt, fold_key=key, weights_id=1)
    with pytest.raises(ValueError, match="fold key"):
        st.check(fold_key=(3.0, "folded", 2))
    with pytest.raises(AttributeError):
        st.shots = (2, 2, 2)
    uids = {st.uid}
    for c in range(N):
        bk = st.bank(c)
        lo = st.offsets[c]
        assert isinstance(bk, SupportBank) and bk is st.bank(c) and bk.nshot == shots[c] and bk.hw == hw
        for i in range(len(layout)):
            assert bk.k[i].data_ptr() == k[i][lo].data_ptr() and bk.v[i].data_ptr() == v[i][lo].data_ptr()
            assert bk.k[i].shape[0] == shots[c] and torch.equal(bk.k[i], k[i][lo:lo + shots[c]])
            assert torch.equal(bk.v[i], v[i][lo:lo + shots[c]])
        uids.add(bk.uid)
    assert len(uids) == N + 1
    with pytest.raises(IndexError):
        st.bank(N)
    for bad in ((1, 3), (1, 3, 2, 1)):                           # a count list of the wrong length
        with pytest.raises(ValueError, match="shot counts"):
            SupportBankSet(k, v, N, bad, hw, dt, dt, key, 1, layout)
    with pytest.raises(ValueError):
        SupportBankSet(k, v, N, (1, 5, 0), hw, dt, dt, key, 1, layout)
    with pytest.raises(ValueError, match="images"):              # the stack does not hold sum(shots) images
        SupportBankSet(kv(tot + 1), kv(tot + 1), N, shots, hw, dt, dt, key, 1, layout)
    with pytest.raises(ValueError, match="images"):
        SupportBankSet(k, v, N, (1, 3, 1), hw, dt, dt, key, 1, layout)
    # a uniform set: the same fields, nshot kept
    u = SupportBankSet(kv(6), kv(6), 3, 2, hw, dt, dt, key, 1, layout)
    assert u.nshot == 2 and u.shots == (2, 2, 2) and u.offsets == (0, 2, 4, 6) and u.ragged is False
    # stack()
    banks = [SupportBank(kv(s), kv(s), s, hw, dt, dt, key, 1, layout) for s in shots]
    with pytest.raises(ValueError, match="bank 1 differs from bank 0 in nshot"):
        SupportBankSet.stack(banks)
    st2 = SupportBankSet.stack(banks, ragged=True)
    assert st2.ragged and st2.shots == shots and st2.nshot is None and st2.nbytes() == st.nbytes()
    for c in range(N):
        for i in range(len(layout)):
            assert torch.equal(st2.bank(c).k[i], banks[c].k[i]) and torch.equal(st2.bank(c).v[i], banks[c].v[i])
            assert st2.bank(c).k[i].data_ptr() != banks[c].k[i].data_ptr()
    same = SupportBankSet.stack([banks[1], banks[1]], ragged=True)       # equal counts, still the caller's choice of route
    assert same.ragged and same.shots == (3, 3) and same.nshot is None
    other = SupportBank(kv(2, dtype=torch.float16), kv(2, dtype=torch.float16), 2, hw, torch.float16, dt, key, 1, layout)
    with pytest.raises(ValueError, match="bank 2 differs from bank 0 in storage dtype"):
        SupportBankSet.stack([banks[0], banks[1], other], ragged=True)
    with pytest.raises(ValueError, match="bank 1 differs from bank 0 in weights"):
        SupportBankSet.stack([banks[0], SupportBank(kv(2), kv(2), 2, hw, dt, dt, key, 7, layout)], ragged=True)


def test_oracle_definition_of_ragged_nway():
    """The definition of the feature, in the reference's own arithmetic (fp32 oracle, tiny config, shots (1, 3, 2), b = 2):
    z0[c] is oracle.pipeline.pipeline_call for class c with ITS OWN s_c supports replicated per query.  The entries of such
    a call are independent of each other -- entry i of the b-query call is the one-query call on query i -- so the
    class-major batch whose entry c*b + i reads the s_c supports of class c is defined entry by entry although no single
    reference call can hold classes of different s.  And padding a class by repeating an example is NOT that class: the
    repeated keys weigh double in the softmax (what the ragged route exists to avoid)."""
    from oracle import pipeline as op
    ou, ov, te = nw._oracle()
    g = torch.Generator().manual_seed(17)
    shots, b, H = (1, 3, 2), 2, 64
    sup = [torch.rand(s, 3, H, H, generator=g) * 2 - 1 for s in shots]
    msk = [(torch.rand(s, 1, H, H, generator=g) > 0.5).float().repeat(1, 3, 1, 1) * 2 - 1 for s in shots]
    qry = torch.rand(b, 3, H, H, generator=g) * 2 - 1
    rep = lambda t, n: t.repeat(n, 1, 1, 1)
    for c, s in enumerate(shots):
        masks, whole = op.pipeline_call(ou, ov, [rep(sup[c], b), qry, rep(msk[c], b)], te)
        assert whole["z0"].shape[0] == b and len(masks) == b
        scale = float(whole["z0"].abs().max())
        for i in range(b):
            m1, one = op.pipeline_call(ou, ov, [sup[c], qry[i:i + 1], msk[c]], te)
            assert torch.allclose(one["z0"][0], whole["z0"][i], rtol=1e-5, atol=1e-5 * scale), (c, i)
            assert (abs(m1[0].astype(int) - masks[i].astype(int)) > 1).mean() < 1e-3, (c, i)
    # class 0 (one example) padded to two by repetition is another function of the query
    _, one = op.pipeline_call(ou, ov, [rep(sup[0], b), qry, rep(msk[0], b)], te)
    _, pad = op.pipeline_call(ou, ov, [rep(sup[0].repeat(2, 1, 1, 1), b), qry, rep(msk[0].repeat(2, 1, 1, 1), b)], te)
    d = float((pad["z0"] - one["z0"]).norm() / one["z0"].norm())
    assert d > 1e-4, d          # ten times the tolerance of the equalities above
