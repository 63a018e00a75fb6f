"""The proof, without a GPU, that the fp64 references alone satisfy what tests/test_nonfinite_gpu.py relies on.

For every case, plant position and planted value of tests/nonfinite.py, from the fp64 reference on the planted operands:
the reference's non-finite set equals the set the case declares analytically; it is non-empty (a -inf logit of a softmax
is a mask and declares the empty set: the row stays finite); outside full reductions at least one element of every output
is finite, so the containment half of the rule has something to test.  For the store-overflow cases the reference exceeds
65520 (where IEEE round-to-nearest-even to fp16 gives inf) at some elements and stays below 65504 / 2 at all others.
Operands are made in the last storage dtype of each case (the sets do not depend on the rounding of the operands); where
the set does not depend on the planted value either (everything but the softmaxes and the attention kernels), each plant
position is proved with one of the three values, rotating over the positions.

The last tests plant faults into check_propagation's own input: it must report a swallowed value (0 and 65504 in place of
a reference-non-finite element), a finite element outside its bound, and an overflow stored as the largest finite value.
"""
import math

import pytest
import torch

import elementwise_bound as eb
import nonfinite as nf

PARAMS, IDS = nf.params(nf.CASES)


def _proved(p):
    """The last storage dtype of each case; all three values where the declared set depends on the value (softmax,
    attention), otherwise one value per plant position, rotating so that each case still meets all three."""
    case, dtype, plant, vname = p
    if dtype != case.dtypes[-1]:
        return False
    return case.value_dependent or list(nf.VALUES).index(vname) == case.plants().index(plant) % 3


LAST = [(p, i) for p, i in zip(PARAMS, IDS) if _proved(p)]
_made = {}


def finite_inputs(case, dtype):
    key = (case.id, dtype)
    if key not in _made:
        _made.clear()                       # one case's operands at a time
        _made[key] = case.make(dtype, "cpu")
    return _made[key]


@pytest.mark.parametrize("case,dtype,plant,vname", [p for p, _ in LAST], ids=[i for _, i in LAST])
def test_reference_set_equals_the_declared_set(case, dtype, plant, vname):
    name, index = plant
    value = nf.VALUES[vname]
    base = finite_inputs(case, dtype)
    inp = nf.plant(base, name, index, value)
    assert inp[name] is not base[name] and bool(torch.isfinite(base[name].float()).all()), "plant() touched the original"
    refs = case.ref(inp, dtype)
    want = case.declared(inp, name, index, value)
    assert set(refs) == set(want)
    total = 0
    for out, ref in refs.items():
        got = ~torch.isfinite(ref.r)
        decl = want[out].reshape(got.shape)
        total += int(got.sum())
        if not torch.equal(got, decl):
            extra, missing = torch.nonzero((got & ~decl).flatten()).flatten(), torch.nonzero((decl & ~got).flatten()).flatten()
            pos = ref.where or (lambda i: f"element {i}")
            raise AssertionError(
                f"{case.id} {out}: plant {nf.describe(name, index, vname)}: the reference is non-finite at {int(got.sum())} "
                f"elements, declared {int(decl.sum())}; " +
                (f"first undeclared: {pos(int(extra[0]))}; " if extra.numel() else "") +
                (f"first declared but finite: {pos(int(missing[0]))}" if missing.numel() else ""))
        whole = out in case.full or out in getattr(case, "full_by_plant", {}).get(name, ())
        if not whole:
            assert bool((~got).any()), f"{case.id} {out}: no finite element left to test containment with"
        # the allowance of every finite element is finite: the family's bound applies to it as it stands
        if case.bound_applies(name, index, value):
            assert bool(torch.isfinite(ref.e.reshape(got.shape)[~got]).all()), f"{case.id} {out}: allowance of a finite element is not finite"
    if case.masked(name, index, value):
        assert total == 0, f"{case.id}: a -inf logit must leave the reference finite"
    else:
        assert total > 0, f"{case.id}: plant {nf.describe(name, index, vname)} left the reference finite"


OPARAMS, OIDS = nf.params(nf.OVERFLOW_CASES)


@pytest.mark.parametrize("case,dtype,plant", OPARAMS, ids=OIDS)
def test_overflow_cases_straddle_the_fp16_range(case, dtype, plant):
    inp = case.make(dtype, "cpu")
    for t in inp.values():
        if torch.is_tensor(t):
            assert bool(torch.isfinite(t.float()).all()), "operands of a store-overflow case are finite"
    ref = case.ref(inp, dtype)[case.okey]
    a = ref.r.abs()
    over = a > nf.F16_INF_FROM
    assert bool(torch.isfinite(a).all()) and int(over.sum()) > 0, f"{case.id}: nothing exceeds the fp16 range"
    assert float(a[~over].max()) < nf.F16_MAX / 2, f"{case.id}: an element lies between 65504 / 2 and 65520: {float(a[~over].max())}"
    print(f"{case.id}: {int(over.sum())} of {a.numel()} elements above 65520 (max {float(a.max()):.4g}), the rest below "
          f"{float(a[~over].max()):.4g}")


def test_threshold_operands_are_exact():
    x, w, want = nf.threshold_operands("cpu")
    got = (x.double() @ w.double().t())[:, 0]
    assert got.tolist() == want == [65504.0, 65520.0, -65504.0, -65520.0]
    # eight products of exactly representable operands, partial sums below 2^24: fp32 accumulation in any order is exact
    assert bool(((x.float() * w[0].float()).double() == x.double() * w[0].double()).all())
    assert torch.tensor(want).to(torch.float16).tolist() == [65504.0, math.inf, -65504.0, -math.inf]


# ------------------------------------------------------------------------------------------------ the checker itself

def _checker_input():
    g = torch.Generator().manual_seed(3)
    r = torch.randn(6, 40, generator=g, dtype=torch.float64) * 5
    r[2, :] = math.nan
    r[4, 7] = math.inf
    r[4, 8] = -math.inf
    e = 1e-6 * torch.ones_like(r)
    y = r.to(torch.float16)
    return y, r, e


def test_checker_accepts_a_faithful_output():
    y, r, e = _checker_input()
    n, nans, infs, worst = nf.check_propagation(y, r, e, torch.float16)
    assert (n, nans, infs) == (42, 40, 2) and worst <= 1.0
    y2 = y.clone()
    y2[2, 3] = math.inf          # inf and NaN are not told apart
    y2[4, 7] = math.nan
    nf.check_propagation(y2, r, e, torch.float16)


@pytest.mark.parametrize("fault", ["zero", "max_finite", "out_of_bound", "leak"])
def test_checker_reports_planted_faults(fault):
    y, r, e = _checker_input()
    y = y.clone()
    where = eb.Where(40, tile=(4, 16))
    if fault == "zero":
        y[2, 39] = 0.0
        msg = r"1 of 42 output elements finite where the reference is non-finite; first at row 2, channel 39, tile \(0, 2\)"
    elif fault == "max_finite":
        y[4, 8] = -65504.0
        msg = r"finite where the reference is non-finite; first at row 4, channel 8, tile \(1, 0\): y=-65504"
    elif fault == "out_of_bound":
        y[5, 1] = y[5, 1] * 1.01 + 0.01
        msg = r"element that does not depend on the plant: 1 of 198 elements outside the bound.*\n  row 5, channel 1, tile"
    else:
        y[0, 0] = math.nan
        msg = r"element that does not depend on the plant: 1 of 198 elements outside the bound.*\n  row 0, channel 0, tile"
    with pytest.raises(AssertionError, match=msg):
        nf.check_propagation(y, r, e, torch.float16, where=where, label="case", planted="x[2, 0] = nan")
    with pytest.raises(AssertionError, match=r"plant x\[2, 0\] = nan"):
        nf.check_propagation(y, r, e, torch.float16, where=where, label="case", planted="x[2, 0] = nan")


def test_checker_reports_a_saturated_overflow_and_a_wrong_sign():
    r = torch.tensor([[1.0, math.inf, -math.inf, 2.0]], dtype=torch.float64)
    e = torch.zeros_like(r)
    nf.check_propagation(r.to(torch.float16), r, e, torch.float16, sign=True)
    for bad in ([1.0, 65504.0, -math.inf, 2.0], [1.0, math.inf, math.inf, 2.0], [1.0, math.nan, -math.inf, 2.0]):
        with pytest.raises(AssertionError, match="not the reference's infinity"):
            nf.check_propagation(torch.tensor([bad], dtype=torch.float16), r, e, torch.float16, sign=True)
