"""The gate between a torch tensor and a raw pointer (diffews_amd/ops.py, ops_bwd.py: one checker, `_Args`) on host
tensors: no `assert` guards an address; every tensor argument of every function that takes an address is refused by name
for one defect (tests/op_args_cases.py), and a valid call on host tensors is refused last, for the device; all of it again
with both files compiled as `python -O` compiles them.  The library and the stream are replaced by a stand-in whose every
use fails the test, so a passing row shows the refusal came before either."""
import ast
import os
import sys
import types

import pytest
import torch

import op_args_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = {m: os.path.join(ROOT, "diffews_amd", m + ".py") for m in ("ops", "ops_bwd")}


class Reached(BaseException):
    """A refused call got as far as the library or the stream (not an Exception: no `raises` swallows it)."""


def _reached(*a, **k):
    raise Reached("a call that had to be refused reached the library or asked for the stream")


def _stripped():
    """ops and ops_bwd compiled with optimize=1 (`assert` stripped, as python -O does) into fresh modules; the ops_bwd copy
    imports its helpers from the ops copy."""
    mods = {}
    saved = sys.modules.get("diffews_amd.ops")
    try:
        for name in ("ops", "ops_bwd"):
            m = types.ModuleType("diffews_amd." + name)
            m.__package__, m.__file__ = "diffews_amd", PATHS[name]
            exec(compile(open(PATHS[name]).read(), PATHS[name], "exec", optimize=1), m.__dict__)
            mods[name] = m
            sys.modules["diffews_amd.ops"] = mods["ops"]
    finally:
        sys.modules["diffews_amd.ops"] = saved
    assert mods["ops_bwd"]._Args is mods["ops"]._Args and mods["ops"]._Args is not saved._Args
    return mods


@pytest.fixture(scope="module", params=["imported", "optimize=1"])
def mods(request):
    """{"ops", "ops_bwd"} with L.lib and every _stream replaced by the stand-in."""
    from diffews_amd import _lib as L, ops, ops_bwd
    m = {"ops": ops, "ops_bwd": ops_bwd} if request.param == "imported" else _stripped()
    saved = [(L, "lib", L.lib)] + [(mod, "_stream", mod._stream) for mod in m.values()]
    for obj, name, _ in saved:
        setattr(obj, name, _reached)
    yield m
    for obj, name, was in saved:
        setattr(obj, name, was)


# ------------------------------------------------------------------------------------------------ the source

def _address_takers():
    """{"ops.linear": FunctionDef, "ops_bwd.ColsumQueue.add": ...}: every function or method of the two files whose body
    takes a tensor's address (.data_ptr(), _p(...)) or makes a checker (_Args(...)); and the number of ast.Assert nodes."""
    found, asserts = {}, 0
    for mod, path in PATHS.items():
        tree = ast.parse(open(path).read())
        asserts += sum(isinstance(n, ast.Assert) for n in ast.walk(tree))
        defs = [(mod + "." + n.name, n) for n in tree.body if isinstance(n, ast.FunctionDef)]
        for cls in (n for n in tree.body if isinstance(n, ast.ClassDef)):
            defs += [(f"{mod}.{cls.name}.{n.name}", n) for n in cls.body if isinstance(n, ast.FunctionDef)]
        for name, fn in defs:
            for call in (n for n in ast.walk(fn) if isinstance(n, ast.Call)):
                f = call.func
                if (isinstance(f, ast.Attribute) and f.attr == "data_ptr") or (isinstance(f, ast.Name) and f.id in ("_p", "_Args")):
                    found[name] = fn
    return found, asserts


def test_no_assert_guards_an_address():
    found, asserts = _address_takers()
    assert asserts == 0, f"{asserts} assert statement(s) in ops.py / ops_bwd.py: python -O would strip them"
    assert len(found) > 60 and {"ops.linear", "ops.seg_match", "ops_bwd.gemm_tn", "ops_bwd.ColsumQueue.add"} <= set(found)


def test_every_tensor_parameter_has_a_row():
    """Every parameter of every address-taking function is a tensor with a row or a name in SCALARS; the functions without
    rows are the ones EXEMPT names, each with its reason."""
    found, _ = _address_takers()
    have, scalars = {}, {}
    for c in cases.CASES:
        have.setdefault(c.fn, set()).update(r.param for r in c.rows)
        scalars.setdefault(c.fn, set(cases.SCALARS)).update(c.scalars)
    assert set(cases.EXEMPT) <= set(found) and not set(cases.EXEMPT) & set(have), "an exemption that is not needed"
    missing = sorted(set(found) - set(have) - set(cases.EXEMPT))
    assert not missing, f"functions that take an address and have no rows: {missing}"
    assert set(have) <= set(found), sorted(set(have) - set(found))
    for name in have:
        a = found[name].args
        params = [p.arg for p in a.posonlyargs + a.args + a.kwonlyargs]
        bare = [p for p in params if p not in have[name] and p not in scalars[name]]
        assert not bare, f"{name}: parameter(s) {bare} have neither a row nor a place in SCALARS"
        assert not have[name] & scalars[name], (name, have[name] & scalars[name])
        assert have[name] <= set(params), (name, have[name] - set(params))


# ------------------------------------------------------------------------------------------------ the table

ROWS = [(c, r) for c in cases.CASES for r in c.rows]


@pytest.mark.parametrize("case,row", ROWS, ids=[f"{c.fn}-{r.name}-{r.defect if isinstance(r.defect, str) else 'edit'}" for c, r in ROWS])
def test_one_defect_is_refused_by_name(mods, case, row):
    kw = case.valid()
    row.spoil(kw)
    with pytest.raises(row.exc, match=case.pattern(row)):
        case.call(mods, kw)


@pytest.mark.parametrize("case", cases.CASES, ids=[f"{c.fn}-{i}" for i, c in enumerate(cases.CASES)])
def test_a_valid_call_on_host_tensors_is_refused_last_for_the_device(mods, case):
    with pytest.raises(ValueError, match=rf"^{case.wrapper}: all tensors must be device tensors on one cuda device"):
        case.call(mods, case.valid())


def test_the_four_demonstrations(mods):
    """The calls of the issue: a 4 x 16 result through a pointer to 4 elements, host tensors, a float64 out, and a shared
    bank that does not hold nshot images."""
    ops = mods["ops"]
    x, w = cases.bf(4, 8), cases.bf(16, 8)
    with pytest.raises(ValueError, match=r"linear: out must be .*, shape \(4, 16\); got torch.float32 \(2, 2\)"):
        ops.linear(x, w, out=torch.zeros(2, 2))
    with pytest.raises(ValueError, match=r"linear: all tensors must be device tensors on one cuda device.*x lies on cpu"):
        ops.linear(x, w)
    with pytest.raises(ValueError, match=r"linear: out must be a unit-last-stride torch.bfloat16 or torch.float32 tensor.*; got torch.float64"):
        ops.linear(x, w, out=torch.zeros(4, 16, dtype=torch.float64))
    q = cases.bf(3, 128, 128)
    with pytest.raises(ValueError, match=r"fsa_attention: k_bank must hold 1 images \(nshot, one shared set\), got 3"):
        ops.fsa_attention(q, q, q, 2, q, q, nshot=1, bank_shared=True)
    with pytest.raises(ValueError, match=r"fsa_attention: k_bank must hold 3 images \(the sum of shots\), got 4"):
        ops.fsa_attention_ragged(cases.bf(4, 128, 128), q[:1].expand(4, -1, -1), q[:1].expand(4, -1, -1), 2, cases.bf(4, 128, 128),
                                 cases.bf(4, 128, 128), shots=(1, 2), group=2)


def test_the_checker_allocates_nothing_and_spans_strided_views(mods):
    ops = mods["ops"]
    tree = ast.parse(open(PATHS["ops"]).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "_Args")
    assert not [n for n in ast.walk(cls) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "torch"
                and n.attr in ("empty", "zeros", "empty_like", "zeros_like", "full", "empty_strided", "tensor")]
    arg = ops._Args("f")
    wide = torch.zeros(4, 12)
    view = wide[:, 4:8]                               # rows 12 apart: 3 * 12 + 4 elements from its first one
    assert ops._span(view) == 40 and ops._span(wide) == 48 and ops._span(torch.zeros(0, 3)) == 0
    assert arg("v", view, torch.float32, (4, 4), dense=False, extent=40) == view.data_ptr()
    with pytest.raises(ValueError, match="f: v must be a unit-last-stride torch.float32 tensor, extent 41; got"):
        arg("v", view, torch.float32, dense=False, extent=41)
    with pytest.raises(ValueError, match="f: v must be a contiguous"):
        arg("v", view, torch.float32)
    with pytest.raises(ValueError, match="f: n is odd"):
        arg.need(False, "n is odd")
    with pytest.raises(ValueError, match="f: all tensors must be device tensors"):
        arg.device()
