"""Every training kernel keeps an inf or a NaN non-finite on its way from the loss to the flat gradient.

One element of one operand is replaced by +inf, -inf or NaN (tests/nonfinite.py: the cases, where they plant and the set
of output elements each plant must reach; tests/test_nonfinite_cpu.py proves those sets against the fp64 references).
The kernel's output is then held to the rule of nonfinite.check_propagation: non-finite wherever the fp64 reference of the
same operation on the planted operands is non-finite, and inside the family's own per-element bound everywhere else, so
the planted value neither disappears nor leaks.  Auxiliary outputs the backward reads (GroupNorm's (mean, rstd), the fused
GroupNorm partial sums of the conv epilogues) follow the same rule.  `-s` prints one PROPAGATION line per run: how many
reference-non-finite elements there were and how many of the kernel's came out NaN / inf.

Store overflow (fp16): finite operands whose exact result exceeds 65520 must be stored as inf of the right sign, not as
65504.  DFW_ACT_CLAMP1 (the decoder's last conv, inference only) clamps by design; what it does with each plant is pinned
in test_clamp1_epilogue_clamps_by_design and is not part of the rule.

Trainer level: one poisoned step each (a NaN query pixel, +inf in the 16-bit shadow of a mid-block conv weight, -inf in
the target) must be reported, leave master, moments and shadow bit-equal and halve the loss scale; the clean step that
follows equals a fresh trainer's clean step bit for bit.
"""
import math

import pytest
import torch

import nonfinite as nf

pytestmark = pytest.mark.gpu

PARAMS, IDS = nf.params(nf.CASES)
OPARAMS, OIDS = nf.params(nf.OVERFLOW_CASES)
_made = {}


@pytest.fixture(scope="module")
def env(hip_lib):
    from diffews_amd import ops, ops_bwd, _lib
    return ops, ops_bwd, _lib


def finite_inputs(case, dtype):
    key = (case.id, dtype)
    if key not in _made:
        _made.clear()                       # one case's operands at a time
        _made[key] = case.make(dtype, "cuda")
    return _made[key]


def run_and_check(env, case, dtype, inp, planted, refs=None, sign=False, bound=True):
    outs = case.run(env, inp, dtype)
    torch.cuda.synchronize()
    refs = refs or case.ref(inp, dtype)
    stats = {}
    for key, y in outs.items():
        ref = refs[key.split("/")[0]]
        stats[key] = nf.check_propagation(y, ref.r, ref.e, ref.dtype, ref.where, f"{case.id} {key}", planted, ref.check, sign, bound)
    case.post(env, inp, dtype, outs, planted)
    return refs, stats


@pytest.mark.parametrize("case,dtype,plant,vname", PARAMS, ids=IDS)
def test_planted_value_reaches_every_dependent_output(env, case, dtype, plant, vname):
    name, index = plant
    planted = nf.describe(name, index, vname)
    inp = nf.plant(finite_inputs(case, dtype), name, index, nf.VALUES[vname])
    refs, stats = run_and_check(env, case, dtype, inp, planted, bound=case.bound_applies(name, index, nf.VALUES[vname]))
    want = case.declared(inp, name, index, nf.VALUES[vname])
    for out, ref in refs.items():           # the reference on these very operands has the declared non-finite set
        assert torch.equal(~torch.isfinite(ref.r).cpu(), want[out].reshape(ref.r.shape)), f"{case.id} {out}: {planted}"
    for key, (n, nans, infs, worst) in stats.items():
        print(f"PROPAGATION {case.family} {case.id} {nf.TNAME[dtype]} {planted} -> {key}: reference non-finite {n}, "
              f"kernel NaN {nans} inf {infs}; finite part worst err/bound {worst:.3f}")


@pytest.mark.parametrize("case,dtype,plant", OPARAMS, ids=OIDS)
def test_result_above_the_fp16_range_is_stored_as_inf(env, case, dtype, plant):
    inp = case.make(dtype, "cuda")
    refs = case.ref(inp, dtype)
    ref = refs[case.okey]
    over = ref.r.abs() > nf.F16_INF_FROM
    assert int(over.sum()) > 0 and float(ref.r.abs()[~over].max()) < nf.F16_MAX / 2
    ref.r = torch.where(over, torch.sign(ref.r) * math.inf, ref.r)
    _, stats = run_and_check(env, case, dtype, inp, "one row scaled past the fp16 range", refs, sign=True)
    n, nans, infs, worst = stats[case.okey]
    assert nans == 0 and infs == n == int(over.sum())
    print(f"PROPAGATION {case.family} {case.id} f16: {n} results above 65520 stored as inf of the reference's sign; "
          f"finite part worst err/bound {worst:.3f}")


def test_the_two_neighbours_of_the_fp16_threshold(env):
    """An exact 65504 stays finite; 65520, the first value that rounds to inf, becomes inf (both signs)."""
    ops, ob, L = env
    x, w, want = nf.threshold_operands("cuda")
    names = []
    ops.gemm_hook = lambda name, *a: names.append(name)
    try:
        y = ops.linear(x, w)
    finally:
        ops.gemm_hook = None
    torch.cuda.synchronize()
    got = y[:, 0].float().tolist()
    print(f"PROPAGATION store_overflow threshold {names}: exact {want} -> stored {got}")
    assert got == [65504.0, math.inf, -65504.0, -math.inf]
    assert bool(torch.isfinite(y[:, 1:].float()).all())


@pytest.mark.parametrize("dtype", nf.DTYPES, ids=["bf16", "f16"])
def test_clamp1_epilogue_clamps_by_design(env, dtype):
    """DFW_ACT_CLAMP1 = fminf(fmaxf(v, -1), 1), the decoder's last conv (inference only, never on the way to a gradient):
    +inf -> 1, -inf -> -1, and NaN -> -1 (fmaxf returns its other operand for a NaN).  A decision, pinned here; the
    epilogue is exempt from the propagation rule."""
    ops, ob, L = env
    g = torch.Generator().manual_seed(2)
    x = torch.randn(96, 128, generator=g).to(dtype).cuda()
    w = (torch.randn(64, 128, generator=g) * 128 ** -0.5).to(dtype).cuda()
    for vname, out in (("+inf", 1.0), ("-inf", -1.0), ("nan", -1.0)):
        bias = torch.zeros(64, device="cuda")
        bias[7] = nf.VALUES[vname]
        y = ops.linear(x, w, bias=bias, act=L.ACT_CLAMP1).float()
        assert bool((y[:, 7] == out).all()), (vname, y[:4, 7].tolist())
        assert bool((y.abs() <= 1.0).all())


@pytest.mark.parametrize("shape", [(2, 3, 16, 20), (1, 3, 5, 7)], ids=["vector", "scalar"])
def test_seg_postprocess_clamps_by_design(env, shape):
    """seg_quant = clamp to [-1, 1], then to uint8 (inference only): a pixel of +inf counts as 1, -inf and NaN as -1
    (fmaxf returns its other operand for a NaN).  Pinned as: the masks and counts equal those of the clamped input."""
    ops, ob, L = env
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(shape, generator=g) * 0.6).cuda()
    gt = (torch.rand(shape[0], shape[2], shape[3], generator=g) > 0.5).to(torch.uint8).cuda()
    at = (shape[0] - 1, 2, shape[2] - 1, shape[3] - 1)
    for vname, same in (("+inf", 1.0), ("-inf", -1.0), ("nan", -1.0)):
        xa, xb = x.clone(), x.clone()
        xa[at], xb[at] = nf.VALUES[vname], same
        (ua, ca), (ub, cb) = ops.seg_postprocess(xa, gt), ops.seg_postprocess(xb, gt)
        assert torch.equal(ua, ub) and torch.equal(ca, cb), vname


# ------------------------------------------------------------------------------------------------ AdamW's guard

@pytest.mark.parametrize("dtype", nf.DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("vname", list(nf.VALUES))
def test_adamw_skips_on_a_non_finite_sumsq_and_clears_the_flag_after(env, dtype, vname):
    ops, ob, L = env
    n = 100_003
    g = torch.Generator().manual_seed(5)
    p, gr = torch.randn(n, generator=g).cuda(), (torch.randn(n, generator=g) * 3).cuda()
    m, v = torch.rand(n, generator=g).cuda(), torch.rand(n, generator=g).cuda()
    shadow = p.to(dtype)
    found = torch.zeros(1, dtype=torch.int32, device="cuda")
    before = [t.clone() for t in (p, m, v, shadow)]
    bad = gr.clone()
    bad[n - 1] = nf.VALUES[vname]                       # the scalar tail of dfw_sumsq
    ss = ob.sumsq(bad)
    assert not bool(torch.isfinite(ss).all())
    ob.adamw(p, bad, m, v, 1, 3e-4, grad_sumsq=ss, max_grad_norm=1.0, shadow=shadow, found_inf=found)
    torch.cuda.synchronize()
    assert int(found[0]) == 1
    for a, b in zip(before, (p, m, v, shadow)):
        assert torch.equal(a, b), "a skipped step changed the optimizer state"
    ob.adamw(p, gr, m, v, 1, 3e-4, grad_sumsq=ob.sumsq(gr), max_grad_norm=1.0, shadow=shadow, found_inf=found)
    torch.cuda.synchronize()
    assert int(found[0]) == 0 and not torch.equal(before[0], p) and bool(torch.isfinite(p).all())
    assert torch.equal(shadow, p.to(dtype))


# ------------------------------------------------------------------------------------------------ trainer level

SCALE0 = 1024.0
STATE = ("master", "exp_avg", "exp_avg_sq", "shadow")


@pytest.fixture(scope="module")
def tiny_trainer(hip_lib):
    from test_backward_gpu import _train_setup
    from diffews_amd.train import UNetTrainer
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(torch.float16, 1, 2, seed=9)
    args = dict(zr=z_refcat.cuda(), zq=z_tag.cuda(), tg=target.cuda(), eh=ehs.cuda())

    def build(scale):
        return UNetTrainer(ucfg, usd, torch_dtype=torch.float16, loss_scale=scale)

    def step(tr, **over):
        a = dict(args, **over)
        loss, pred = tr.forward_backward(a["zr"], a["zq"], a["tg"], 1, a["eh"])
        grads = tr.P.grad.clone()
        tr.optimizer_step(1e-4, max_grad_norm=1.0)
        tr._resolve_overflow()
        torch.cuda.synchronize()
        return loss.clone(), pred.clone(), grads

    fresh = build(SCALE0 / 2)
    clean = step(fresh) + tuple(getattr(fresh.P, k).clone() for k in STATE)
    assert fresh.skipped_steps == 0 and all(bool(torch.isfinite(t.float()).all()) for t in clean)
    return dict(args=args, build=build, step=step, clean=clean)


@pytest.mark.parametrize("poison", ["nan_query_pixel", "inf_shadow_weight", "neg_inf_target"])
def test_trainer_reports_one_poisoned_step_and_recovers_bit_for_bit(tiny_trainer, poison):
    t = tiny_trainer
    tr = t["build"](SCALE0)
    assert tr.dynamic_loss_scale
    over = {}
    if poison == "nan_query_pixel":
        over["zq"] = t["args"]["zq"].clone()
        over["zq"][0, 1, 5, 7] = math.nan
    elif poison == "neg_inf_target":
        over["tg"] = t["args"]["tg"].clone()
        over["tg"][0, 2, 3, 11] = -math.inf
    else:
        name = next(n for n, (off, shape) in tr.P.spec.items() if n.startswith("mid_block.resnets.0.conv1") and len(shape) >= 2)
        tr.P.w(name).view(-1)[17] = math.inf              # the 16-bit shadow only: the fp32 master stays finite
        assert bool(torch.isfinite(tr.P.p(name)).all())
    before = [getattr(tr.P, k).clone() for k in STATE]
    t["step"](tr, **over)
    assert tr.skipped_steps == 1 and tr.step_count == 0, f"{poison}: the overflow was not reported"
    assert tr.loss_scale == SCALE0 / 2
    for k, a in zip(STATE, before):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                           getattr(tr.P, k).view(torch.int16 if a.dtype == torch.float16 else torch.int32)), f"{poison}: {k} changed"
    if poison == "inf_shadow_weight":
        tr.P.sync_shadow()                                # the same state again: the shadow is the rounded master
    got = t["step"](tr) + tuple(getattr(tr.P, k).clone() for k in STATE)
    assert tr.skipped_steps == 1 and tr.step_count == 1
    for label, a, b in zip(("loss", "pred", "grad") + STATE, got, t["clean"]):
        assert torch.equal(a, b), f"{poison}: {label} of the following clean step differs from a fresh trainer's"
