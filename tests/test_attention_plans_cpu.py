"""CPU tests (no GPU) of the attention checker (tests/attention_bound.py) and of the plan coverage of
tests/test_attention_plans_gpu.py: dfw_fsa_kernel_name follows dfw_fsa_attention's launch rules, every case plans the
launch it names, and together the cases reach every forward instantiation and every split / combine / fold / remap
variant -- evaluated through the host-only queries, no device call."""
import ctypes as C

import pytest
import torch

import attention_bound as ab

BF16, F16 = torch.bfloat16, torch.float16


def _rnd(shape, g, scale=1.0):
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


# ---- the checker

def _lockstep_forward(g, dtype, nshot, heads, N):
    """Lock-step batch (nshot support images, then one query image) of pre-scaled q: 16-bit q, k, v and the fp64
    reference (r, e, lse, e_lse) of every image and head."""
    Bt, Cc = nshot + 1, heads * 64
    q = (_rnd((Bt, N, Cc), g) * ab.LN2 ** -1 * 64 ** -0.5 * 2).to(dtype)
    k, v = _rnd((Bt, N, Cc), g).to(dtype), _rnd((Bt, N, Cc), g).to(dtype)
    r = torch.empty(Bt, N, Cc, dtype=ab.F64)
    e = torch.empty_like(r)
    lse = torch.empty(Bt, heads, N, dtype=ab.F64)
    el = torch.empty_like(lse)
    for b in range(Bt):
        segs = ab.key_segments(k, v, b, nshot, nshot, k, v)
        for h in range(heads):
            sl = slice(h * 64, (h + 1) * 64)
            K, V = torch.cat([s[1][:, sl] for s in segs]), torch.cat([s[2][:, sl] for s in segs])
            r[b, :, sl], e[b, :, sl], lse[b, h], el[b, h] = ab.fwd_ref(q[b][:, sl], K, V, dtype)
    return q, k, v, r, e, lse, el


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_checker_accepts_correctly_rounded_results(dtype):
    g = torch.Generator().manual_seed(1)
    q, k, v, r, e, lse, el = _lockstep_forward(g, dtype, 2, 2, 200)
    assert ab.check(r.to(dtype), r, e, dtype, label="out") <= 1.0
    assert ab.check(lse.float(), lse, el, torch.float32, label="lse") <= 1.0
    # backward from the correctly rounded forward
    out, lse32 = r.to(dtype), lse.float()
    do = _rnd(out.shape, g).to(dtype)
    accs = [[ab.BwdAcc(200, 64, "cpu") for _ in range(2)] for _ in range(3)]
    for b in range(3):
        segs = ab.key_segments(k, v, b, 2, 2, k, v)
        for h in range(2):
            sl = slice(h * 64, (h + 1) * 64)
            dq, edq = ab.bwd_ref(q[b][:, sl], [(K[:, sl], V[:, sl], accs[i][h]) for i, K, V in segs], out[b][:, sl],
                                 do[b][:, sl], lse32[b, h], dtype)
            assert ab.check(dq.to(dtype), dq, edq, dtype, label="dq") <= 1.0
    for b in range(3):
        for h in range(2):
            dk, edk, dv, edv = accs[b][h].finish()
            assert ab.check(dk.to(dtype), dk, edk, dtype, label="dk") <= 1.0
            assert ab.check(dv.to(dtype), dv, edv, dtype, label="dv") <= 1.0
    dq, edq, dk, edk, dv, edv = ab.xattn_bwd_ref(q[0][:, :64], k[0][:77, :64], v[0][:77, :64], do[0][:, :64])
    for y, ee in ((dq, edq), (dk, edk), (dv, edv)):
        assert ab.check(y.to(dtype), y, ee, dtype, label="xattn bwd") <= 1.0


def test_forward_fault_in_one_key_tile_of_one_shot_passes_global_l2_and_fails_the_bound():
    """Query image 7 of a 7-shot lock-step batch, head 5, query block 1 (rows 128..255) loses key tile 3 of shot 2: the
    existing forward criterion (test_ops_gpu: rel < 1.5 TOL) accepts it, the per-element bound names the block."""
    from test_ops_gpu import TOL, rel
    g = torch.Generator().manual_seed(2)
    nshot, heads, N = 7, 8, 512
    q, k, v, r, e, lse, el = _lockstep_forward(g, BF16, nshot, heads, N)
    bq, h, rows = nshot, 5, slice(128, 256)
    sl = slice(h * 64, (h + 1) * 64)
    K = torch.cat([k[bq]] + [k[s] for s in range(nshot)])[:, sl].double()
    V = torch.cat([v[bq]] + [v[s] for s in range(nshot)])[:, sl].double()
    keep = torch.ones(K.shape[0], dtype=torch.bool)
    keep[N + 2 * N + 192:N + 2 * N + 256] = False                    # shot 2, keys 192..255 of that image
    P = torch.softmax((q[bq][rows, sl].double() @ K[keep].t()) * ab.LN2, 1)     # q pre-scaled: exp2 exponents
    bad = r.clone()
    bad[bq, rows, sl] = P @ V[keep]
    y, y_bad = r.to(BF16), bad.to(BF16)
    assert ab.check(y, r, e, BF16) <= 1.0
    assert rel(y_bad, r) < 1.5 * TOL[BF16], rel(y_bad, r)          # the gap: global L2 passes
    with pytest.raises(AssertionError, match=r"image 7, head 5, query row \d+ \(query block 1\)"):
        ab.check(y_bad, r, e, BF16, where=ab.Where(N, heads, 128), label="dropped key tile")


def test_backward_fault_in_one_support_key_tile_passes_global_l2_and_fails_the_bound():
    """Support image 2, head 1, key tile 1 (keys 64..127) misses the query pass' contribution to its dK: the existing
    backward criterion (test_backward_gpu: rel < 2 TOL) accepts it, the per-element bound names the tile."""
    from test_backward_gpu import TOL, rel
    g = torch.Generator().manual_seed(3)
    nshot, heads, N = 7, 8, 256
    q, k, v, r, e, lse, el = _lockstep_forward(g, BF16, nshot, heads, N)
    out, lse32 = r.to(BF16), lse.float()
    do = _rnd(out.shape, g).to(BF16)
    Bt, Cc = nshot + 1, heads * 64
    accs = [[ab.BwdAcc(N, 64, "cpu") for _ in range(heads)] for _ in range(Bt)]
    for b in range(Bt):
        segs = ab.key_segments(k, v, b, nshot, nshot, k, v)
        for hh in range(heads):
            sl = slice(hh * 64, (hh + 1) * 64)
            ab.bwd_ref(q[b][:, sl], [(K[:, sl], V[:, sl], accs[i][hh]) for i, K, V in segs], out[b][:, sl],
                       do[b][:, sl], lse32[b, hh], BF16)
    dk, edk = torch.empty(Bt, N, Cc, dtype=ab.F64), torch.empty(Bt, N, Cc, dtype=ab.F64)
    for b in range(Bt):
        for hh in range(heads):
            sl = slice(hh * 64, (hh + 1) * 64)
            dk[b, :, sl], edk[b, :, sl], _, _ = accs[b][hh].finish()
    # the query pass' share of support image 2, head 1 alone
    s_img, h = 2, 1
    sl = slice(h * 64, (h + 1) * 64)
    qpass = {i: ab.BwdAcc(N, 64, "cpu") for i in range(Bt)}
    segs = ab.key_segments(k, v, nshot, nshot, nshot, k, v)
    ab.bwd_ref(q[nshot][:, sl], [(K[:, sl], V[:, sl], qpass[i]) for i, K, V in segs], out[nshot][:, sl],
               do[nshot][:, sl], lse32[nshot, h], BF16)
    bad = dk.clone()
    bad[s_img, 64:128, sl] -= qpass[s_img].finish()[0][64:128]
    y, y_bad = dk.to(BF16), bad.to(BF16)
    assert ab.check(y, dk, edk, BF16) <= 1.0
    assert rel(y_bad, dk) < 2 * TOL[BF16], rel(y_bad, dk)          # the gap: global L2 passes
    with pytest.raises(AssertionError, match=r"image 2, head 1, key \d+ \(key tile 1\)"):
        ab.check(y_bad, dk, edk, BF16, where=ab.Where(N, heads, 64, what="key"), label="dropped query pass")


# ---- the plan query and the plan coverage

def _fsa_args(L, **kw):
    a = L.FsaArgs()
    a.q = a.k = a.v = a.out = a.k_bank = a.v_bank = 4096
    a.dtype, a.q_prescaled = L.BF16, 1
    for key, val in kw.items():
        setattr(a, key, val)
    a.ldq = a.ldk = a.ldv = a.ldo = a.ldkb = a.ldvb = a.heads * 64
    return a


def _name(L, a):
    buf = C.create_string_buffer(96)
    L.check(L.lib().dfw_fsa_kernel_name(C.byref(a), buf, 96), "dfw_fsa_kernel_name")
    return buf.value.decode()


def test_fsa_kernel_name_follows_the_launch_rules(hip_lib):
    from diffews_amd import _lib as L
    from test_attention_plans_gpu import configured
    a = _fsa_args(L, batch=1, heads=1, n_q=1024, n_kv=1024)
    assert _name(L, a) == "fsa_ring_kernel<bf16,4,1,pre>"
    a.n_q, a.q_prescaled, a.dtype = 1025, 0, L.F16
    assert _name(L, a) == "fsa_ring_kernel<f16,8,1,scale>"
    a = _fsa_args(L, batch=8, heads=2, n_q=1024, n_kv=1024, n_bank=1024, nshot=7, n_plain=7)
    nbytes = L.lib().dfw_fsa_workspace_bytes(C.byref(a))
    assert nbytes > 0
    unsplit = "fsa_ring_kernel<bf16,4,1,pre>+xcd"                             # heads * 8 images = 16
    assert _name(L, a) == unsplit                                             # no workspace
    a.workspace, a.workspace_bytes = 4096, nbytes - 4
    assert _name(L, a) == unsplit                                             # too short
    a.workspace, a.workspace_bytes = 4096 + 8, nbytes
    assert _name(L, a) == unsplit                                             # not 16-byte aligned
    a.workspace = 4096
    assert _name(L, a) == "fsa_ring_kernel<bf16,4,1,pre>+split8"             # heads * (7 + 8) = 30: no remap
    with configured(L, dict(fsa_force_splits=3)):
        a.workspace_bytes = L.lib().dfw_fsa_workspace_bytes(C.byref(a))
        assert _name(L, a) == "fsa_ring_kernel<bf16,4,1,pre>+split3"
        a.heads = 4
        a.ldq = a.ldk = a.ldv = a.ldo = a.ldkb = a.ldvb = 256
        a.workspace_bytes = L.lib().dfw_fsa_workspace_bytes(C.byref(a))
        assert _name(L, a) == "fsa_ring_kernel<bf16,4,1,pre>+xcd+split3"     # 4 * (7 + 3) = 40
    a.ldk = 100
    with pytest.raises(RuntimeError, match="dfw_fsa_kernel_name"):            # the launch's argument checks
        _name(L, a)


FWD_INSTANTIATIONS = {f"fsa_ring_kernel<T,{nw},1,{m}>" for nw in (4, 8) for m in ("pre", "scale")} | {"fsa_combine_kernel<T>"}


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_every_case_plans_its_launch_and_the_cases_reach_every_variant(hip_lib, dtype):
    from diffews_amd import _lib as L, ops
    import test_attention_plans_gpu as plans
    code = L.BF16 if dtype == BF16 else L.F16
    tname = plans.TNAME[dtype]
    reached, wrong, variants = set(), [], set()
    fwd = [(c, plans.expected(c, dtype), c.cfg) for c in plans.FSA_CASES]
    fwd += [(plans._fsa_case_of(c), None, c.cfg) for c in plans.FSA_BWD_CASES]     # the backward cases' forwards
    for case, want, cfg in fwd:
        with plans.configured(L, cfg), plans.fsa_names(ops, L, launch=False) as names:
            plans.run_fsa(ops, case, plans.make_fsa_inputs(case, dtype, "cpu", fill=False))
        if want is not None and names != [want]:
            wrong.append((case.id, names, want))
            continue
        name = names[0]
        base = name.partition("+")[0]
        reached.add(base.replace(tname, "T", 1))
        if "+split" in name:
            ns = int(name.split("+split")[1])
            reached.add("fsa_combine_kernel<T>")
            nseg = 1 + case.nshot
            variants.add(("split", "+xcd" in name))
            variants.add(("forced" if cfg.get("fsa_force_splits") else "default", nseg % ns == 0))
            if ns < nseg:
                variants.add("instance over several segments")
    assert not wrong, "\n" + "\n".join(f"{cid}: planned {got}, expected {want}" for cid, got, want in wrong)
    assert reached == FWD_INSTANTIATIONS, (FWD_INSTANTIATIONS - reached, reached - FWD_INSTANTIATIONS)
    assert {("split", True), ("split", False), ("default", True), ("forced", False),
            "instance over several segments"} <= variants, variants
    # backward: dQ key split by the default rule, forced, and off; dK/dV query split on and off; the cross-attention fold
    dq = set()
    for c in plans.FSA_BWD_CASES:
        with plans.configured(L, c.cfg):
            ns = plans.fsa_bwd_splits(L, c, code)
        assert ns == c.splits, (c.id, ns, c.splits)
        dq.add("off" if ns == 1 else ("forced" if c.cfg else "default"))
    assert dq == {"off", "default", "forced"}, dq
    assert all(c.splits == 1 for c in plans.FSA_BWD_CASES if not c.key_split)
    qs = {plans.attn_bwd_qsplit(L, c, code) for c in plans.ATTN_BWD_CASES}
    for c in plans.ATTN_BWD_CASES:
        assert plans.attn_bwd_qsplit(L, c, code) == c.qsplit, c.id
    assert 1 in qs and max(qs) > 1
    chunks = {-(-c.n_q // 64) for c in plans.XB_CASES}
    assert 1 in chunks and max(chunks) > 1
    assert {c.L for c in plans.XA_CASES} >= {1, 2, 63, 64, 65, 77, 128}
    assert {c.L for c in plans.XB_CASES} >= {1, 2, 16, 17, 77, 80}
    assert max(c.B for c in plans.VA_CASES) >= 9 and any(c.spike and c.spike[0] >= 8 for c in plans.VA_CASES)
