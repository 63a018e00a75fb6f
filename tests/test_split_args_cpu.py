"""The gate between a torch tensor and a raw pointer in diffews_amd/ops_split.py, held to what tests/test_op_args_cpu.py
asks of ops.py: no `assert`, no allocation, every tensor through ops._Args; every tensor parameter of every address-taking
function has a row in tests/split_args_cases.py and is refused by name for one defect; a valid call on host tensors is
refused last, for the device -- as imported and compiled as `python -O` compiles it.  The library and the stream are
replaced by a stand-in whose every use fails the test."""
import ast
import os
import sys
import types

import pytest

import split_args_cases as cases
import test_op_args_cpu as base

PATH = os.path.join(base.ROOT, "diffews_amd", "ops_split.py")


def _stripped():
    """ops_split compiled with optimize=1 on top of an ops module compiled the same way."""
    ops = base._stripped()["ops"]
    saved = sys.modules.get("diffews_amd.ops")
    try:
        sys.modules["diffews_amd.ops"] = ops
        m = types.ModuleType("diffews_amd.ops_split")
        m.__package__, m.__file__ = "diffews_amd", PATH
        exec(compile(open(PATH).read(), PATH, "exec", optimize=1), m.__dict__)
    finally:
        sys.modules["diffews_amd.ops"] = saved
    assert m._Args is ops._Args and ops._Args is not saved._Args
    return {"ops_split": m}


@pytest.fixture(scope="module", params=["imported", "optimize=1"])
def mods(request):
    from diffews_amd import _lib as L, ops_split
    m = {"ops_split": ops_split} if request.param == "imported" else _stripped()
    saved = [(L, "lib", L.lib), (m["ops_split"], "_stream", m["ops_split"]._stream)]
    for obj, name, _ in saved:
        setattr(obj, name, base._reached)
    yield m
    for obj, name, was in saved:
        setattr(obj, name, was)


def _address_takers():
    tree = ast.parse(open(PATH).read())
    found = {}
    for fn in (n for n in tree.body if isinstance(n, ast.FunctionDef)):
        for call in (n for n in ast.walk(fn) if isinstance(n, ast.Call)):
            f = call.func
            if (isinstance(f, ast.Attribute) and f.attr == "data_ptr") or (isinstance(f, ast.Name) and f.id in ("_p", "_Args")):
                found["ops_split." + fn.name] = fn
    return found, tree


def test_no_assert_no_allocation_and_one_checker():
    found, tree = _address_takers()
    assert set(found) == {"ops_split.seg_nearest", "ops_split.seg_components_keyed"}
    assert not [n for n in ast.walk(tree) if isinstance(n, ast.Assert)]
    assert not [n for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "torch"
                and n.attr in ("empty", "zeros", "empty_like", "zeros_like", "full", "empty_strided", "tensor", "cat", "where")]
    assert not [n for n in ast.walk(tree) if isinstance(n, ast.ClassDef)]   # the checker is ops._Args, imported
    from diffews_amd import ops, ops_split
    assert ops_split._Args is ops._Args


def test_every_tensor_parameter_has_a_row():
    found, _ = _address_takers()
    have = {c.fn: {r.param for r in c.rows if r.param in [a.arg for a in found[c.fn].args.args]} for c in cases.CASES}
    assert set(have) == set(found)
    for name, fn in found.items():
        params = [p.arg for p in fn.args.posonlyargs + fn.args.args + fn.args.kwonlyargs]
        bare = [p for p in params if p not in have[name] and p not in cases.SCALARS]
        assert not bare, f"{name}: parameter(s) {bare} have neither a row nor a place in SCALARS"
        assert not have[name] & cases.SCALARS


ROWS = [(c, r) for c in cases.CASES for r in c.rows]


@pytest.mark.parametrize("case,row", ROWS, ids=[f"{c.fn}-{r.name}-{r.defect if isinstance(r.defect, str) else 'edit'}-{i}"
                                                for i, (c, r) in enumerate(ROWS)])
def test_one_defect_is_refused_by_name(mods, case, row):
    kw = case.valid()
    row.spoil(kw)
    with pytest.raises(row.exc, match=case.pattern(row)):
        case.call(mods, kw)


@pytest.mark.parametrize("case", cases.CASES, ids=[c.fn for c in cases.CASES])
def test_a_valid_call_on_host_tensors_is_refused_last_for_the_device(mods, case):
    with pytest.raises(ValueError, match=rf"^{case.wrapper}: all tensors must be device tensors on one cuda device"):
        case.call(mods, case.valid())
    kw = case.valid()                                                      # optional tensors absent: still the device
    for k in ("filtered", "stats", "gt", "counts", "nlabels"):
        if k in kw:
            kw[k] = None
    with pytest.raises(ValueError, match=rf"^{case.wrapper}: all tensors must be device tensors on one cuda device"):
        case.call(mods, kw)
