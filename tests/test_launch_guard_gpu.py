"""The plan matrices under guard: every compute kernel launched three times on the same inputs -- plain, with every
allocation of its wrapper pattern-filled with 0xFF (NaN in the three float types), and with 0x7B (large and finite) -- inside
1 MiB guards (tests/launch_guard.py).  Everything the op returns (lse, the fused GroupNorm sums, dgamma / dbeta, in/out
tensors) must be bit-equal across the three launches, every guard byte intact, every input unchanged.  No tolerance, no
reference: an element never written differs between the patterns, a read of uninitialised scratch or past an input is NaN
in one run and something else in the other, a race or an atomic shows as a difference.

The cases are the tables of the plan tests (the smallest shapes that reach every kernel instantiation), imported, in both
storage dtypes and under the same ids; each case declares which wrapper functions must appear among the recorded
allocations.  tests/test_launch_guard_cpu.py proves the harness on planted faults and that every allocating function of
ops.py / ops_bwd.py is declared here (ALL_DECLARED) or guarded by an older test.

Exemptions from the bit comparison (regions a wrapper documents as unwritten): none.  ops._u8_buf's pad belongs to the
native-size kernels, which run under 0xA5 guards of their own and are not launched here.

Model level (tiny UNet / VAE of tests/test_model_gpu.py, built fresh inside every launch so that no cached buffer keeps a
pattern from an earlier one; the proxy also stands in for torch in unet, vae, pipeline and train): one run_episodes
episode and one prepare_support + segment_queries pass with nshot 1, one segment_classes call, one UNetTrainer step
(loss, prediction, every gradient, the updated master weights, both moments and the 16-bit shadow).

LDS: in the two pattern launches check_launches also fills every CU's LDS with the pattern in front of every launching
library call (tests/lds_poison.py); the model-level cases declare, as `dfw_` names, entry points that must have been poisoned.
"""
import pytest
import torch

import launch_guard as lg
import test_attention_plans_gpu as ap
import test_boundary_plans_gpu as bp
import test_conv_epilogue_gpu as ce
import test_gemm_plans_gpu as gp
import test_norm_plans_gpu as npg
import test_up2x_fold_gpu as up
from test_nway_gpu import SETS_CASES, sets_names
from test_ragged_sets_gpu import RAGGED_CASES, ragged_names
from test_routed_gpu import ROUTED_CASES, routed_names, _table
from test_support_bank_gpu import _bank, _qkv

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
F32 = torch.float32
SENTINEL = 3.0

ALL_DECLARED = set()


def D(*names):
    """Wrapper functions a case declares: they must show in the call chains of the allocations its launches record."""
    ALL_DECLARED.update(names)
    return names


def params_of(test, name):
    """The values a plan test is parametrised with under `name` (its shapes live in the decorator, not in a table)."""
    for m in test.pytestmark:
        if m.name == "parametrize" and m.args[0] == name:
            return list(m.args[1])
    raise KeyError(name)


@pytest.fixture(scope="module")
def env(hip_lib):
    from diffews_amd import ops, ops_bwd, _lib
    return ops, ops_bwd, _lib


def seed_of(text):
    return sum(map(ord, text))


# ------------------------------------------------------------------------------------------------ the harness on the device

def test_harness_reports_broken_contracts_on_the_device(env):
    """What tests/test_launch_guard_cpu.py proves on fake ops, once with the real kernels and device memory, through calls
    that break a documented contract on purpose (every access stays inside the guarded buffers): an accumulate target
    nobody initialised, a dpred destination that is not zero-initialised (backward.hip: channels C..7 are the caller's),
    one element written behind a wrapper's output, an input overwritten after the launch.  lds=False: the messages pinned here
    are the memory-only ones (tests/test_lds_poison_gpu.py pins those of the LDS poison)."""
    ops, ob, _ = env
    g = npg.gen(1)
    x, pred, tgt = npg.randn((64, 24), g, torch.bfloat16), npg.randn((2, 4, 16, 16), g), npg.randn((2, 4, 16, 16), g)
    lg.check_launches([ob], lambda run: ob.colsum(run.place(x), out=run.full((1, 24), 1.5, dtype=F32, device="cuda"), accumulate=True),
                      lds=False)

    def stale(run):
        return ob.colsum(run.place(x), out=run.empty(1, 24, dtype=F32, device="cuda"), accumulate=True)

    with pytest.raises(lg.GuardError, match="result 0 .* differs from the plain launch .* allocated by stale"):
        lg.check_launches([ob], stale, lds=False)

    def unzeroed(run):
        return ob.mse_loss(run.place(pred), run.place(tgt), torch.bfloat16,
                           dpred_out=run.empty(2, 16, 16, 8, dtype=torch.bfloat16, device="cuda"))

    with pytest.raises(lg.GuardError, match=r"result 1 .* first at element 4, .* allocated by unzeroed"):
        lg.check_launches([ob], unzeroed, lds=False)

    def torn(run):
        y = ob.silu(run.place(x))
        if run.pattern is not None:
            y.as_strided((1,), (1,), y.storage_offset() + y.numel()).fill_(0.0)
        return y

    with pytest.raises(lg.GuardError, match=r"store past the end \(first damaged guard byte \+0\) of the buffer of 3072 bytes allocated by silu"):
        lg.check_launches([ob], torn, lds=False)

    def clobbered(run):
        px = run.place(x)
        y = ob.silu(px)
        px[3, 3] += 1.0
        return y

    with pytest.raises(lg.GuardError, match="input modified at byte 15[01]: buffer of 3072 bytes placed by clobbered"):
        lg.check_launches([ob], clobbered, lds=False)


# ------------------------------------------------------------------------------------------------ dfw_gemm, dfw_gemm_tn

D_FWD = {"linear": D("linear"), "bmm": D("bmm_nt"), "conv": D("conv3x3")}
D_SPLITK = D("_gemm_launch")
D_TN, D_WS = D("gemm_tn"), D("_ws")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", gp.FWD_CASES, ids=[c.id for c in gp.FWD_CASES])
def test_forward_plan_guarded(env, case, dtype):
    ops, _, L = env
    want = gp.expected(case, dtype)
    inp = gp.make_fwd_inputs(case, dtype, "cuda", seed=seed_of(case.id))
    names = []

    def call(run):
        p = {k: (run.inout(v) if k == "wide" else run.place(v)) for k, v in inp.items()}
        return gp.run_fwd(ops, case, p), p.get("wide")

    declared = D_FWD[case.op] if not case.view else ()
    with gp.configured(L, case.cfg):
        ops.gemm_hook = lambda name, *a: names.append(name)
        try:
            lg.check_launches([ops], call, declared + (D_SPLITK if "+splitk" in want else ()))
        finally:
            ops.gemm_hook = None
    assert names == [want] * 3, names


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", gp.TN_CASES, ids=[c.id for c in gp.TN_CASES])
def test_tn_plan_guarded(env, case, dtype):
    _, ob, L = env
    want = gp.expected(case, dtype)
    inp = gp.make_tn_inputs(case, dtype, "cuda", seed=seed_of(case.id))
    N = case.shape[1] if case.op == "lin" else case.shape[4]
    Kc = case.shape[2] if case.op == "lin" else case.shape[3]

    def call(run):     # gp.run_tn, with the accumulated-into output inside the guards
        out = run.inout(inp["out"]) if case.accumulate else None
        return ob.gemm_tn(run.place(inp["dy"]), run.place(inp["x"]), n=N, kc=Kc, out=out, taps=inp["taps"], geom=inp["geom"],
                          accumulate=case.accumulate, scale=case.scale)

    with gp.tn_names(L) as names:
        lg.check_launches([ob], call, D_WS + (() if case.accumulate else D_TN))
    assert len(names) == 3 and len(set(names)) == 1 and gp.name_matches(names[0], want), (names, want)


# ------------------------------------------------------------------------------------------------ residual as a column view

@pytest.mark.parametrize("M,N,K,kernel", params_of(ce.test_linear_epilogue_operands, "M,N,K,kernel"))
def test_linear_residual_column_view(env, M, N, K, kernel):
    """ops.linear passes residual.stride(0) as ldr and the residual's buffer descriptor is sized from it: a residual that
    is wide[:, 64:64 + N] of a NaN-filled [M, N + 128] buffer plans the same kernel and gives the same bits as the
    contiguous one (nothing outside the view is read into the result).  wide[:, 4:4 + N] of [M, N + 12] (rows 8 bytes past a
    16-byte boundary, ldr % 8 == 4): the same bits where the planner keeps the kernel, else every element within the
    bound of tests/elementwise_bound.py, as test_forward_plan checks it."""
    import elementwise_bound as eb
    ops = env[0]
    x, w = ce._rand((M, K), 1), ce._rand((N, K), 2, K ** -0.5)
    bias, res = ce._rand((N,), 3, dtype=F32), ce._rand((M, N), 4)
    out = []
    assert ce._kernel_name(ops, lambda: out.append(ops.linear(x, w, bias=bias, residual=res))) == [kernel]
    for left, extra in ((64, 128), (4, 12)):
        wide = torch.full((M, N + extra), float("nan"), dtype=ce.DT, device="cuda")
        view = wide[:, left:left + N]
        view.copy_(res)
        got = []
        names = ce._kernel_name(ops, lambda: got.append(ops.linear(x, w, bias=bias, residual=view)))
        assert torch.equal(view, res) and bool(torch.isnan(wide[:, :left]).all()) and bool(torch.isnan(wide[:, left + N:]).all())
        if left == 64:
            assert names == [kernel], names
        if names == [kernel]:
            assert torch.equal(got[0], out[0]), (left, names)
        else:
            S, A = eb.gemm_ref(x, w)
            r, e = eb.epilogue_ref(S, A, K, bias=bias, residual=res)
            bm, bn = gp.tile_of(names[0])
            eb.check(got[0], r, e, ce.DT, where=eb.Where(N, tile=(bm, bn)), label=f"residual view ldr {N + extra} {names[0]}")
        print(f"residual view [{M}, {left}:{left + N}] of {N + extra} columns: {names[0]}")


# ------------------------------------------------------------------------------------------------ attention, forward

D_FSA, D_FSA_SPLIT = D("_fsa_args"), D("_fsa_launch")
D_XA, D_VA = D("cross_attention"), D("vae_attention")


def _place_fsa(run, case, inp):
    p = {k: run.place(inp[k]) for k in ("q", "k", "v")}
    if case.nshot:
        if case.n_bank:
            p["kb"], p["vb"] = run.place(inp["kb"]), run.place(inp["vb"])
        else:
            p["kb"], p["vb"] = p["k"][:case.n_plain], p["v"][:case.n_plain]
    p["lse"] = run.empty(case.B, case.heads, case.n_q, dtype=F32, device="cuda")
    return p


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ap.FSA_CASES, ids=[c.id for c in ap.FSA_CASES])
def test_fsa_plan_guarded(env, case, dtype):
    ops, _, L = env
    want = ap.expected(case, dtype)
    inp = ap.make_fsa_inputs(case, dtype, "cuda", seed=seed_of(case.id))

    def call(run):
        p = _place_fsa(run, case, inp)
        return ap.run_fsa(ops, case, p), p["lse"]

    with ap.configured(L, case.cfg), ap.fsa_names(ops, L) as names:
        lg.check_launches([ops], call, D_FSA + (D_FSA_SPLIT if "+split" in want else ()))
    assert names == [want] * 3, names


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ap.XA_CASES, ids=[c.id for c in ap.XA_CASES])
def test_cross_attention_plan_guarded(env, case, dtype):
    ops = env[0]
    q, k, v, _ = ap.make_xa_inputs(case, dtype, "cuda", seed=seed_of(case.id))
    lg.check_launches([ops], lambda run: ops.cross_attention(run.place(q), run.place(k), run.place(v), case.heads), D_XA)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ap.VA_CASES, ids=[c.id for c in ap.VA_CASES])
def test_vae_attention_plan_guarded(env, case, dtype):
    ops = env[0]
    q, k, v = ap.make_va_inputs(case, dtype, "cuda", seed=seed_of(case.id))
    lg.check_launches([ops], lambda run: ops.vae_attention(run.place(q), run.place(k), run.place(v)), D_VA)


def _names_agree(names, suffix, must_split, recorded):
    """The three launches took one plan of the expected form; a key split asked the wrapper for its scratch."""
    assert len(names) == 3 and len(set(names)) == 1 and names[0].endswith(suffix), names
    assert "+split" in names[0] or not must_split, names
    assert ("+split" in names[0]) == (D_FSA_SPLIT[0] in recorded), (names, sorted(recorded))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", SETS_CASES, ids=[c[0] for c in SETS_CASES])
def test_sets_guarded(env, case, dtype):
    ops, _, L = env
    cid, sets, b, s, heads, n_q, n_bank = case
    g = torch.Generator(device="cuda").manual_seed(21)
    q, k, v = _qkv(sets * b, n_q, heads, dtype, g)
    kb, vb = _bank(sets * s, n_bank, heads, dtype, g)

    def call(run):
        lse = run.empty(sets * b, heads, n_q, dtype=F32, device="cuda")
        return ops.fsa_attention_sets(run.place(q), run.place(k), run.place(v), heads, run.place(kb), run.place(vb), s, b,
                                      q_prescaled=True, lse=lse), lse

    with sets_names(ops, L) as names:
        recorded = lg.check_launches([ops], call, D_FSA)
    _names_agree(names, "+sets", cid == "split", recorded)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", RAGGED_CASES, ids=[c[0] for c in RAGGED_CASES])
def test_ragged_guarded(env, case, dtype):
    ops, _, L = env
    cid, shots, b, heads, n_q, n_bank = case
    g = torch.Generator(device="cuda").manual_seed(31)
    q, k, v = _qkv(len(shots) * b, n_q, heads, dtype, g)
    kb, vb = _bank(sum(shots), n_bank, heads, dtype, g)

    def call(run):
        lse = run.empty(len(shots) * b, heads, n_q, dtype=F32, device="cuda")
        return ops.fsa_attention_ragged(run.place(q), run.place(k), run.place(v), heads, run.place(kb), run.place(vb), shots, b,
                                        q_prescaled=True, lse=lse), lse

    with ragged_names(ops, L) as names:
        recorded = lg.check_launches([ops], call, D_FSA)
    _names_agree(names, "+ragged", cid == "split", recorded)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ROUTED_CASES, ids=[c[0] for c in ROUTED_CASES])
def test_routed_guarded(env, case, dtype):
    ops, _, L = env
    cid, shots, route, heads, n_q, n_bank = case
    g = torch.Generator(device="cuda").manual_seed(41)
    q, k, v = _qkv(len(route), n_q, heads, dtype, g)
    kb, vb = _bank(sum(shots), n_bank, heads, dtype, g)
    host = _table(shots, route)
    table = host.cuda()

    def call(run):
        return ops.fsa_attention_routed(run.place(q), run.place(k), run.place(v), heads, run.place(kb), run.place(vb),
                                        run.place(table), host, max(shots), min(shots), q_prescaled=True)

    with routed_names(ops, L) as names:
        recorded = lg.check_launches([ops], call, D_FSA)
    _names_agree(names, "+routed", cid == "split", recorded)


# ------------------------------------------------------------------------------------------------ attention, backward

D_FSA_BWD, D_ATTN_BWD, D_XA_BWD = D("fsa_attention_bwd"), D("attention_bwd"), D("cross_attention_bwd")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ap.FSA_BWD_CASES, ids=[c.id for c in ap.FSA_BWD_CASES])
def test_fsa_attention_bwd_plan_guarded(env, case, dtype):
    ops, ob, L = env
    g = torch.Generator().manual_seed(seed_of(case.id))
    H, N, Cc = case.heads, case.N, case.heads * 64
    n_plain = case.b * case.nshot
    Bt = n_plain + case.b
    qkv = torch.randn(Bt, N, 3 * Cc, generator=g)
    qkv[..., :Cc] *= ap.QSCALE * 2
    qkv = qkv.to(dtype).cuda()
    dout = torch.randn(Bt, N, Cc, generator=g).to(dtype).cuda()
    fcase = ap._fsa_case_of(case)

    def call(run):
        pq = run.place(qkv)
        q, k, v = pq[..., :Cc], pq[..., Cc:2 * Cc], pq[..., 2 * Cc:]
        p = {"q": q, "k": k, "v": v, "lse": run.empty(Bt, H, N, dtype=F32, device="cuda")}
        if case.nshot:
            p["kb"], p["vb"] = k[:n_plain], v[:n_plain]
        out = ap.run_fsa(ops, fcase, p)
        dqkv = ob.fsa_attention_bwd(pq, out, run.place(dout), p["lse"], H, nshot=case.nshot, n_plain=n_plain,
                                    key_split=case.key_split)
        return out, p["lse"], dqkv

    with ap.configured(L, case.cfg):
        assert ap.fsa_bwd_splits(L, case, L.BF16 if dtype == torch.bfloat16 else L.F16) == case.splits
        lg.check_launches([ops, ob], call, D_FSA + D_FSA_BWD)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ap.ATTN_BWD_CASES, ids=[c.id for c in ap.ATTN_BWD_CASES])
def test_attention_bwd_plan_guarded(env, case, dtype):
    ops, ob, L = env
    g = torch.Generator().manual_seed(seed_of(case.id))
    H, Cc = case.heads, case.heads * 64
    assert ap.attn_bwd_qsplit(L, case, L.BF16 if dtype == torch.bfloat16 else L.F16) == case.qsplit
    qb = ap._strided(case.B, case.n_q, Cc + 64, 64, F32, "cpu", g)
    qb[..., :Cc] *= ap.QSCALE * 2
    qd = torch.zeros(case.B * (case.n_q * (Cc + 64) + 64), dtype=dtype, device="cuda").as_strided(qb.shape, qb.stride())
    qd.copy_(qb.to(dtype))
    kv = torch.randn(case.B, case.n_kv, 2 * Cc + 64, generator=g).to(dtype).cuda()
    dout = torch.randn(case.B, case.n_q, Cc, generator=g).to(dtype).cuda()
    fcase = ap.Fsa(case.id, case.B, H, case.n_q, case.n_kv, "")

    def call(run):
        pkv = run.place(kv)
        p = {"q": run.place(qd)[..., :Cc], "k": pkv[..., :Cc], "v": pkv[..., Cc:2 * Cc],
             "lse": run.empty(case.B, H, case.n_q, dtype=F32, device="cuda")}
        out = ap.run_fsa(ops, fcase, p)
        dkv = run.full(tuple(kv.shape), SENTINEL, dtype=dtype, device="cuda")
        dq = ob.attention_bwd(p["q"], p["k"], p["v"], out, run.place(dout), p["lse"], H, dkv[..., :Cc], dkv[..., Cc:2 * Cc],
                              q_split=case.q_split)
        return out, p["lse"], dq, dkv

    lg.check_launches([ops, ob], call, D_FSA + D_ATTN_BWD)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ap.XB_CASES, ids=[c.id for c in ap.XB_CASES])
def test_cross_attention_bwd_plan_guarded(env, case, dtype):
    _, ob, _ = env
    q, k, v, do = ap.make_xa_inputs(case, dtype, "cuda", seed=seed_of(case.id))
    Cc = case.heads * 64

    def call(run):
        dkv = run.full((case.B, case.L, 2 * Cc + 64), SENTINEL, dtype=dtype, device="cuda")
        dq = ob.cross_attention_bwd(run.place(q), run.place(k), run.place(v), run.place(do), case.heads, dkv[..., :Cc],
                                    dkv[..., Cc:2 * Cc])
        return dq, dkv

    lg.check_launches([ob], call, D_XA_BWD + D_WS)


# ------------------------------------------------------------------------------------------------ GroupNorm, LayerNorm

D_GN, D_GN_BWD, D_LN, D_LN_BWD = D("groupnorm"), D("groupnorm_bwd"), D("layernorm"), D("layernorm_bwd")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", npg.GN_CASES, ids=lambda c: c.id)
def test_groupnorm_forward_and_backward_guarded(env, c, dtype):
    """The operands of test_groupnorm_forward_and_backward.  Cases whose x / y / dy / dx are column views, and the one
    without dgamma / dbeta, go through that module's own argument builders (their scratch is allocated there: the proxy
    stands in for its torch as well)."""
    ops, ob, L = env
    g = npg.gen(len(c.id) * 1000 + c.C + c.HW)
    x = npg.gn_input(c, dtype, g)
    gamma = npg.randn((c.C,), g, F32, 0.2, 1.0) if c.affine else None
    beta = npg.randn((c.C,), g, F32, 0.2) if c.affine else None
    shape = (c.B, c.HW, c.C)
    if c.pad:
        _, xv = npg.wide(shape, c.C + c.pad, g, x.dtype)
        xv.copy_(x)
        x = xv
    full = c.bwd == "full"
    dg0 = npg.randn((c.C,), g) if full else None
    db0 = npg.randn((c.C,), g) if full else None
    gs = 0.5 if full else 1.0
    if not c.xf32:
        dy = npg.wide(shape, c.C + c.pad, g, dtype)[1] if c.pad else npg.randn(shape, g, dtype)
        add = (npg.wide(shape, c.C + c.pad + 8, g, dtype)[1] if c.pad else npg.randn(shape, g, dtype)) if full else None

    def call(run):
        px, pg, pb = run.place(x), run.place(gamma), run.place(beta)
        if c.pad:
            yb = run.full((c.B, c.HW, c.C + c.pad + 8), SENTINEL, dtype=dtype, device="cuda")
            mr = npg.gn_forward(L, px, yb[..., :c.C], pg, pb, c.groups, npg.EPS, c.silu)
            y = yb
        else:
            y, mr = ops.groupnorm(px, pg, pb, c.groups, npg.EPS, silu=c.silu, return_stats=True, out_dtype=dtype if c.xf32 else None)
        if c.xf32:
            return y, mr
        if c.bwd == "null":
            dg = db = None
        elif full:
            dg, db = run.inout(dg0), run.inout(db0)
        else:
            dg, db = (run.full((c.C,), SENTINEL, dtype=F32, device="cuda") for _ in range(2))
        pdy, padd = run.place(dy), run.place(add)
        if c.pad:
            dxb = run.full((c.B, c.HW, c.C + c.pad + 8), SENTINEL, dtype=dtype, device="cuda")
            npg.gn_backward(L, px, pdy, dxb[..., :c.C], mr, pg, pb, c.groups, c.silu, dg, db, full, gs, padd)
            dx = dxb
        elif c.bwd == "null":
            dx = run.empty(*shape, dtype=dtype, device="cuda")
            npg.gn_backward(L, px, pdy, dx, mr, pg, pb, c.groups, c.silu, None, None, False, 1.0, None)
        else:
            dx = ob.groupnorm_bwd(px, pdy, mr, pg, pb, c.groups, c.silu, dg, db, accumulate=full, grad_scale=gs, dx_add=padd)
        return y, mr, dx, dg, db

    declared = () if c.pad else D_GN + (() if c.xf32 or c.bwd == "null" else D_GN_BWD + D_WS)
    lg.check_launches([ops, ob, npg], call, declared)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_groupnorm_from_fused_statistics_guarded(env, dtype):
    """test_groupnorm_with_statistics_fused_into_the_producing_conv: the conv's epilogue emits the chunk sums, groupnorm
    folds them -- 16-bit and fp32 output."""
    ops, _, _ = env
    from diffews_amd.packing import pack_conv3x3
    g = npg.gen(7)
    B, H, W, Cin, Cout = 3, 128, 128, 64, 256
    x = npg.randn((B, H, W, Cin), g, dtype)
    w = pack_conv3x3(npg.randn((Cout, Cin, 3, 3), g, dtype, (9 * Cin) ** -0.5).cpu()).cuda()
    bias, gamma, beta = npg.randn((Cout,), g), npg.randn((Cout,), g, F32, 0.2, 1.0), npg.randn((Cout,), g, F32, 0.2)
    res = npg.randn((B, H, W, Cout), g)

    def call(run):
        px, pw, pbias, pg, pb = (run.place(t) for t in (x, w, bias, gamma, beta))
        y16 = ops.conv3x3(px, pw, Cout, bias=pbias, gn_groups=32)
        y32 = ops.conv3x3(px, pw, Cout, bias=pbias, residual=run.place(res), out_f32=True, gn_groups=32)
        assert getattr(y16, "_gn_stats", None) is not None and getattr(y32, "_gn_stats", None) is not None
        return (y16, y32, ops.groupnorm(y16, pg, pb, 32, 1e-6, silu=True, return_stats=True),
                ops.groupnorm(y32, pg, pb, 32, 1e-6, silu=True, return_stats=True, out_dtype=dtype))

    lg.check_launches([ops], call, D_FWD["conv"] + D_GN)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,Cc,pad,xf32", npg.LN_CASES)
def test_layernorm_forward_and_backward_guarded(env, rows, Cc, pad, xf32, dtype):
    ops, ob, _ = env
    g = npg.gen(rows * 7 + Cc)
    xb = npg.randn((rows, Cc + pad), g, F32, 3.0, 1.0)
    x = (xb if xf32 else xb.to(dtype))[:, :Cc]
    gamma, beta = npg.randn((Cc,), g, F32, 0.5, 1.0), npg.randn((Cc,), g, F32, 0.2)
    dy = npg.randn((rows, Cc + pad), g, dtype)[:, :Cc]
    dg0, db0, add = npg.randn((Cc,), g), npg.randn((Cc,), g), npg.randn((rows, Cc), g, dtype)

    def call(run):
        px, pg, pb = run.place(x), run.place(gamma), run.place(beta)
        y = ops.layernorm(px, pg, pb, npg.EPS, out_dtype=dtype if xf32 else None)
        if xf32:
            return y
        pdy = run.place(dy)
        dg, db = (run.full((Cc,), SENTINEL, dtype=F32, device="cuda") for _ in range(2))
        dx = ob.layernorm_bwd(px, pdy, pg, dg, db, npg.EPS)
        dg2, db2 = run.inout(dg0), run.inout(db0)
        dx2 = ob.layernorm_bwd(px, pdy, pg, dg2, db2, npg.EPS, accumulate=True, grad_scale=0.5, dx_add=run.place(add))
        return y, dx, dg, db, dx2, dg2, db2

    lg.check_launches([ops, ob], call, D_LN + (() if xf32 else D_LN_BWD + D_WS))


# ------------------------------------------------------------------------------------------------ column sums

D_COLSUM, D_FLUSH = D("colsum"), D("flush")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_colsum_single_calls_and_one_queue_flush_guarded(env, dtype):
    """Every case and variant of test_colsum_single_calls_and_one_queue_flush through colsum(out=), through ONE
    ColsumQueue.flush(), and -- where nothing is accumulated -- through colsum() allocating its own result."""
    _, ob, _ = env
    items = npg.colsum_operands(dtype, npg.gen(11))
    twins = [out0.clone() for _, _, out0, _, _ in items]

    def call(run):
        q, res = ob.ColsumQueue(), []
        for ((rps, segs, N), x, out0, scale, accum), twin in zip(items, twins):
            px, o1, o2 = run.place(x), run.inout(out0), run.inout(twin)
            ob.colsum(px, segs=segs, out=o1[:, :N], accumulate=accum, scale=scale)
            q.add(px, o2[:, :N], segs=segs, accumulate=accum, scale=scale)
            res += [o1, o2]
            if not accum:
                res.append(ob.colsum(px, segs=segs, scale=scale))
        q.flush()
        return res

    lg.check_launches([ob], call, D_COLSUM + D_WS + D_FLUSH)


# ------------------------------------------------------------------------------------------------ softmax, pointwise, loss

D_SOFTMAX = D("softmax_rows", "softmax_groups")
D_GEGLU = D("geglu_fwd", "geglu_bwd")
D_EW = D("add", "pool2x2_sum", "slice_channels", "zero_stuff2x", "silu")
D_LOSS = D("mse_loss", "loss_grad")
D_SUMSQ = D("sumsq")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Lr", npg.SOFTMAX_L)
def test_softmax_rows_guarded(env, Lr, dtype):
    ops = env[0]
    x = npg.randn((37, Lr), npg.gen(Lr), F32, 4.0)
    x[5, :], x[6, :] = -30.0, 1.75
    x[5, Lr - 1] = 25.0
    x[7, :Lr // 2] -= 200.0
    lg.check_launches([ops], lambda run: ops.softmax_rows(run.place(x), dtype, scale=0.3), D_SOFTMAX[:1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,ld,groups,Lg", npg.SOFTMAX_GROUPS)
def test_softmax_groups_guarded(env, rows, ld, groups, Lg, dtype):
    ops = env[0]
    x = npg.randn((rows, ld), npg.gen(rows), F32, 3.0)
    lg.check_launches([ops], lambda run: ops.softmax_groups(run.place(x), groups, Lg, dtype), D_SOFTMAX[1:])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,H", npg.GEGLU_CASES)
def test_geglu_guarded(env, rows, H, dtype):
    ob = env[1]
    g = npg.gen(rows + H)
    pre, dout = npg.randn((rows, 2 * H), g, dtype, 1.5), npg.randn((rows, H), g, dtype)

    def call(run):
        p = run.place(pre)
        return ob.geglu_fwd(p), ob.geglu_bwd(p, run.place(dout))

    lg.check_launches([ob], call, D_GEGLU)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_elementwise_modes_guarded(env, dtype):
    """The operands of test_elementwise_modes: more 16-byte pieces than threads (the grid-stride loop runs)."""
    ob = env[1]
    g = npg.gen(3)
    a, b = npg.randn((2, 96, 96, 512), g, dtype), npg.randn((2, 96, 96, 512), g, dtype)
    big = npg.randn((2, 192, 192, 320), g, dtype)
    small = a[:, :8, :8].contiguous()
    s, d = npg.randn((3, 1000, 320), g, dtype, 3.0), npg.randn((3, 1000, 320), g, dtype)

    def call(run):
        pa, ps = run.place(a), run.place(s)
        return (ob.add(pa, run.place(b)), ob.pool2x2_sum(run.place(big)), ob.slice_channels(pa, 64, 128),
                ob.zero_stuff2x(run.place(small)), ob.silu(ps), ob.silu(ps, run.place(d)))

    lg.check_launches([ob], call, D_EW)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", params_of(npg.test_loss_kernels, "shape"))
def test_loss_kernels_guarded(env, shape, dtype):
    """mse_loss and loss_grad allocate dpred with torch.zeros (backward.hip: the caller passes a zero-initialised buffer,
    the kernels leave channels C..7 alone): the whole [B, H, W, 8] tensor is compared, padding included."""
    ob = env[1]
    g = npg.gen(sum(shape))
    pred, tgt = npg.randn(shape, g), npg.randn(shape, g)

    def call(run):
        pp = run.place(pred)
        nchw, nchw2 = (run.empty(*shape, dtype=F32, device="cuda") for _ in range(2))
        loss, dpred = ob.mse_loss(pp, run.place(tgt), dtype, loss_scale=8.0, dpred_nchw_out=nchw)
        return loss, dpred, nchw, ob.loss_grad(pp, dtype, scale=0.37, dpred_nchw_out=nchw2), nchw2

    lg.check_launches([ob], call, D_LOSS)


@pytest.mark.parametrize("n,off", params_of(npg.test_sumsq, "n,off"))
def test_sumsq_guarded(env, n, off):
    ob = env[1]
    x = npg.randn((n + off,), npg.gen(n), F32, 3.0)[off:]
    lg.check_launches([ob], lambda run: ob.sumsq(run.place(x)), D_SUMSQ)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_adamw_guarded(env, dtype):
    """test_adamw_per_element's three fused steps (two clipped), every state tensor in/out and the shadow a pure output."""
    ob = env[1]
    n = 100_003
    g = npg.gen(5)
    p0, gr = npg.randn((n,), g), npg.randn((n,), g, F32, 3.0)
    gr[::97] = 0.0
    m0, v0 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    grads = [gr * step * (0.01 if step == 3 else 1.0) for step in (1, 2, 3)]

    def call(run):
        p, m, v = run.inout(p0), run.inout(m0), run.inout(v0)
        shadow = run.empty(n, dtype=dtype, device="cuda")
        sums = []
        for step, gc in zip((1, 2, 3), grads):
            pg = run.place(gc)
            ss = ob.sumsq(pg)
            ob.adamw(p, pg, m, v, step, 3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_sumsq=ss, max_grad_norm=1.0,
                     shadow=shadow)
            sums.append(ss)
        return p, m, v, shadow, sums

    lg.check_launches([ob], call, D_SUMSQ)


# ------------------------------------------------------------------------------------------------ boundary convs, folded upsample

D_CONV_SMALL, D_UP2X = D("conv_small"), D("conv3x3_up2x")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", bp.CASES, ids=[c.id for c in bp.CASES])
def test_conv_small_guarded(env, case, dtype):
    """test_boundary_plans_gpu.run builds the destination views (a channel slice of a wider NCHW tensor, a batch slice, a
    slice of a larger partial-sum buffer) with torch.full: the proxy stands in for that module's torch too, so they are
    guarded and returned whole."""
    ops, _, L = env
    chunks = bp.planned(case, dtype, L)[3]
    xs, w, bias = bp.make_inputs(case, 1000 + bp.CASES.index(case))

    def call(run):
        return bp.run(ops, case, dtype, [run.place(x) for x in xs], run.place(w), run.place(bias), chunks)

    lg.check_launches([ops, bp], call, () if (case.wide or case.batch_slice) else D_CONV_SMALL)


UP2X_GN = params_of(up.test_groupnorm_partial_sums_feed_groupnorm, "shape,groups")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,groups", [(s, 0) for s in up.SHAPES] + UP2X_GN,
                         ids=["x".join(map(str, s)) for s in up.SHAPES] + [f"gn{g_}-" + "x".join(map(str, s)) for s, g_ in UP2X_GN])
def test_conv3x3_up2x_guarded(env, shape, groups, dtype):
    ops = env[0]
    x, _, wf, bias = up._case(shape, dtype, seed=2 if groups else 0)

    def call(run):
        y = ops.conv3x3_up2x(run.place(x), run.place(wf), shape[4], bias=run.place(bias), gn_groups=groups)
        assert y is not None and (not groups or getattr(y, "_gn_stats", None) is not None)
        return y

    lg.check_launches([ops], call, D_UP2X)


# ------------------------------------------------------------------------------------------------ relayouts and glue

D_RELAYOUT = D("linear_wt", "conv3x3_wd")
D_GLUE = D("transpose", "concat_channels", "to_storage", "split_storage", "zeros", "timestep_embedding", "nchw_to_nhwc")
D_SEG = D("seg_postprocess", "seg_labels", "seg_labels_cand")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_weight_relayouts_guarded(env, dtype):
    """linear_wt, conv3x3_wd and the one-launch table form (its destinations pattern-filled) on dims that are and are not
    multiples of the 64 x 64 block."""
    ob = env[1]
    from test_glue_exact_gpu import pattern16
    lins = [pattern16((N, K), dtype, N * 10000 + K).cuda() for N, K in ((8, 56), (64, 72), (136, 1288), (1288, 64))]
    convs = [pattern16((co, 9 * ci), dtype, co * 7 + ci).cuda() for co, ci in ((8, 56), (72, 136), (320, 64), (8, 1288))]

    def call(run):
        pl, pc = [run.place(w) for w in lins], [run.place(w) for w in convs]
        single = [ob.linear_wt(w) for w in pl] + [ob.conv3x3_wd(w, w.shape[0]) for w in pc]
        entries = [("T", w, run.empty(w.shape[1], w.shape[0], dtype=dtype, device="cuda")) for w in pl]
        entries += [("D", w, run.empty(w.shape[1] // 9, 9 * w.shape[0], dtype=dtype, device="cuda")) for w in pc]
        ob.weight_relayout_batch(ob.relayout_table(entries, "cuda"))
        batch = [y for _, _, y in entries]
        torch.cuda.synchronize()
        for a, b in zip(single, batch):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        return single, batch

    lg.check_launches([ob], call, D_RELAYOUT)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layout_and_convert_kernels_guarded(env, dtype):
    """transpose, concat_channels (16-bit and the fp32 byte copy), to_storage / split_storage, the kernel-filled zeros
    (sizes that need padding to 16 bytes), timestep_embedding and nchw_to_nhwc (channels zero-padded to cp): odd sizes, more
    than one block."""
    ops, ob, _ = env
    from test_glue_exact_gpu import pattern16
    xt = [pattern16((3, R, Cc), dtype, R * 1000 + Cc).cuda() for R, Cc in ((1, 63), (65, 130), (130, 64))]
    ca, cb = torch.randn(140000, 24).to(dtype).cuda(), torch.randn(140000, 40).to(dtype).cuda()
    fa, fb = torch.randn(5, 12).cuda(), torch.randn(5, 20).cuda()
    f32 = torch.randn(3, 1000, 8 * 33, generator=torch.Generator().manual_seed(1)).cuda()
    t = torch.tensor([0.0, 0.5, 1.0, 500.0, 999.0], dtype=F32).cuda()
    img = torch.randn(3, 4, 7, 5, generator=torch.Generator().manual_seed(2)).cuda()

    def call(run):
        p32 = run.place(f32)
        return ([ops.transpose(run.place(x)) for x in xt], ops.concat_channels(run.place(ca), run.place(cb)),
                ops.concat_channels(run.place(fa), run.place(fb)), ops.to_storage(p32, dtype), ops.split_storage(p32, dtype),
                [ops.zeros(s, dt) for s, dt in (((3, 5), torch.bfloat16), ((1,), F32), ((7, 3, 1), torch.int64), ((257, 5), dtype))],
                [ops.timestep_embedding(run.place(t), dim, dtype, flip_sin_to_cos=flip) for dim, flip in ((32, True), (320, False))],
                ob.nchw_to_nhwc(run.place(img), dtype, cp=8, scale=0.5))

    lg.check_launches([ops, ob], call, D_GLUE)


@pytest.mark.parametrize("mode", [dict(r_threshold=0.25), dict(r_threshold=0.25, batch_max=True), dict(r_threshold=0.0, threshold=0.3)],
                         ids=["dyn", "batch_max", "fixed"])
def test_seg_postprocess_and_label_fusion_guarded(env, mode):
    """The three label kernels that allocate their own outputs: seg_postprocess (bytes, counts, the maxima scratch),
    seg_labels on its masks, seg_labels_cand with an empty query and padding entries (test_candidates_gpu's table) and the
    per-entry areas."""
    ops = env[0]
    from test_candidates_gpu import OFF, _entries
    from test_nway_gpu import _gt, _masks
    import nway_ref
    N, B, H, W = 3, 2, 7, 9
    dec = (torch.rand(N * B, 3, H, W, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
    gt1 = (torch.rand(N * B, H, W, generator=torch.Generator().manual_seed(6)) * 3).to(torch.uint8).cuda()
    gt1[gt1 > 1] = 255
    masks = _masks(N, B, H, W, 7)
    mx, gtn = nway_ref.maxima(masks).cuda(), _gt(N, B, H, W, 8).cuda()
    E_cap, lab = 8, [3, 3, 1, 2, 3]
    ent = torch.from_numpy(_entries(H, W, E_cap, 9))
    emx = ent.view(E_cap, -1).max(1).values.to(torch.int32).cuda()
    tab = torch.tensor(OFF + lab + [0] * (E_cap - len(lab)), dtype=torch.int32)
    gtc = _gt(3, len(OFF) - 1, H, W, 10).cuda()
    cand = {k: v for k, v in mode.items() if k != "batch_max"}

    def call(run):
        dyn = mode["r_threshold"] > 0
        return (ops.seg_postprocess(run.place(dec), run.place(gt1), **mode),
                ops.seg_labels(run.place(masks.cuda()), run.place(mx) if dyn else None, run.place(gtn), **mode),
                ops.seg_labels_cand(run.place(ent.cuda()), run.place(emx) if dyn else None, run.place(tab.cuda()), tab, 3,
                                    run.place(gtc), want_area=True, **cand))

    lg.check_launches([ops], call, D_SEG)


# ------------------------------------------------------------------------------------------------ model level

MODEL_DTYPES = [torch.float16, torch.bfloat16]
MODEL_IDS = ["fp16", "bf16"]


@pytest.fixture(scope="module")
def model_modules(hip_lib):
    from diffews_amd import ops, ops_bwd, pipeline, train, unet, vae
    return [ops, ops_bwd, unet, vae, pipeline, train]


@pytest.fixture(scope="module", params=MODEL_DTYPES, ids=MODEL_IDS)
def tiny(request, hip_lib):
    """State dicts and prompt of tests/test_model_gpu.py's tiny engines, and a builder: every launch gets engines of its
    own, built while the proxy is installed, so their buffers are that launch's."""
    from diffews_amd import config, weights
    from test_model_gpu import _kw
    dt = request.param
    ucfg, vcfg = config.get("tiny_unet"), config.get("tiny_vae")
    usd = weights.synthetic_unet_state_dict(ucfg, round_to=dt)
    vsd = weights.synthetic_vae_state_dict(vcfg, round_to=dt)
    te = weights.synthetic_text_embed(ucfg).to(dt).float()

    def build():
        from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise
        from diffews_amd.scheduler import DDIMSchedulerCustomized
        from diffews_amd.unet import MyUNet2DConditionModel
        from diffews_amd.vae import AutoencoderKL
        sched = DDIMSchedulerCustomized(**_kw(config.get("scheduler")))
        return MarigoldPipelineRGBLatentNoise(MyUNet2DConditionModel(ucfg, usd, torch_dtype=dt), AutoencoderKL(vcfg, vsd, torch_dtype=dt),
                                              sched, text_embeds=te)

    return dict(dt=dt, build=build)


def test_episode_guarded(tiny, model_modules):
    """run_episodes (the lock-step [support ; query] step) and prepare_support + segment_queries (the bank route), nshot 1,
    with a ground truth: z0, dec, seg_u8 and counts of both."""
    from test_model_gpu import _episode
    sup, qry, msk = _episode(1, 1, 64, seed=3)
    gt = (msk[:, 0] > 0).to(torch.uint8)

    def call(run):
        pipe = tiny["build"]()
        ep = pipe.run_episodes(sup, qry, msk, query_gt=gt, captured=False)
        bank = pipe.prepare_support(sup, msk)
        return ep, pipe.segment_queries(bank, qry, query_gt=gt, captured=False)

    lg.check_launches(model_modules, call, D_FWD["conv"] + D_FWD["linear"] + D_FSA + D_GN + D_LN + D_SEG[:1] +
                      ("dfw_gemm", "dfw_fsa_attention", "dfw_groupnorm", "dfw_layernorm", "dfw_seg_postprocess_ex"))


def test_segment_classes_guarded(tiny, model_modules):
    """prepare_support_classes (ragged: shots 1, 3, 2) + segment_classes on two queries with labels: z0, dec, seg_u8, labels,
    counts."""
    from test_ragged_sets_gpu import _classes
    from test_support_bank_gpu import _queries
    from test_nway_gpu import _gt
    sups, msks = _classes(71)
    qry, labels = _queries(2, 64, 72), _gt(len(sups), 2, 64, 64, 73)

    def call(run):
        pipe = tiny["build"]()
        return pipe.segment_classes(pipe.prepare_support_classes(sups, msks), qry, query_labels=labels, captured=False)

    lg.check_launches(model_modules, call, D_FSA + D_SEG[1:2] + ("dfw_gemm", "dfw_seg_labels"))


def test_trainer_step_guarded(tiny, model_modules):
    """One UNetTrainer step (b 1, nshot 2: the dQ path through the bank): loss, prediction, every gradient, then the clipped
    AdamW update -- master weights, both moments, the 16-bit shadow."""
    from test_backward_gpu import _train_setup
    dt = tiny["dt"]
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dt, 1, 2, seed=9)
    zr, zq, tg, eh = z_refcat.cuda(), z_tag.cuda(), target.cuda(), ehs.cuda()

    def call(run):
        from diffews_amd.train import UNetTrainer
        tr = UNetTrainer(ucfg, usd, torch_dtype=dt, loss_scale=1.0 if dt == torch.bfloat16 else 1024.0, dynamic_loss_scale=False)
        loss, pred = tr.forward_backward(zr, zq, tg, 1, eh)
        grads = tr.P.grad.clone()
        tr.optimizer_step(1e-4, max_grad_norm=1.0)
        return loss, pred, grads, tr.P.master, tr.P.exp_avg, tr.P.exp_avg_sq, tr.P.shadow

    lg.check_launches(model_modules, call, D_WS + D_FSA_BWD + D_GN_BWD + D_LN_BWD + D_FLUSH +
                      ("dfw_gemm", "dfw_gemm_tn", "dfw_fsa_attention_bwd", "dfw_groupnorm_bwd", "dfw_layernorm_bwd", "dfw_colsum_batch",
                       "dfw_adamw"))
