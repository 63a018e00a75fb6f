"""The launch-guard harness (tests/launch_guard.py) catches what it claims to, on CPU tensors: small fake ops written in
torch that allocate through the proxy, each with one planted fault -- and a scan of ops.py / ops_bwd.py proving that every
allocation there goes through the module global the proxy replaces and is named by a GPU case of
tests/test_launch_guard_gpu.py (or by an existing 0xA5-guarded test)."""
import ast
import os
import types

import pytest
import torch

import launch_guard as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAKE_SRC = '''
import torch

CALLS = [0]


def _raw(t):
    st = t.untyped_storage()
    return torch.empty(0, dtype=torch.uint8).set_(st, 0, (st.nbytes(),), (1,))


def _poke(t, at, value):
    """One byte of t's storage, where the storage has it (a real allocation ends at the tensor; a kernel's stray store
    would land in the allocator's slack)."""
    raw = _raw(t)
    if 0 <= at < raw.numel():
        raw[at] = value


def _scratch(n):
    return torch.empty(n, dtype=torch.float32)


def good(x):
    """y = 2 x + rowsum(x) through a scratch buffer, everything written before it is read."""
    y = torch.empty_like(x)
    ws = _scratch(x.shape[0])
    ws.copy_(x.sum(1))
    y.copy_(2 * x + ws[:, None])
    return y


def store_past(x):
    y = good(x)
    _poke(y, (y.storage_offset() + y.numel()) * y.element_size(), 1)
    return y


def store_before(x):
    y = good(x)
    _poke(y, y.storage_offset() * y.element_size() - 1, 1)
    return y


def unwritten(x):
    y = torch.empty(x.shape, dtype=x.dtype)
    y.view(-1)[:-1].copy_((2 * x).view(-1)[:-1])
    return y


def stale_scratch(x):
    y = torch.empty_like(x)
    ws = _scratch(x.shape[0] + 1)
    ws[:x.shape[0]].copy_(x.sum(1))
    y.copy_(2 * x + ws[1:, None])          # the last row reads a slot nobody wrote
    return y


def read_past(x):
    n, have = x.numel(), x.untyped_storage().nbytes() // x.element_size()
    y = torch.empty(n, dtype=x.dtype)
    if x.storage_offset() + n + 1 <= have:                                 # one element past the end, where memory is mapped
        y.copy_(x.as_strided((n,), (1,), x.storage_offset() + 1))
    else:
        y[:-1].copy_(x.reshape(-1)[1:])
        y[-1] = 0.0
    return y


def clobber(x):
    y = good(x)
    x[0, 0] = 5.0
    return y


def drifting(x):
    CALLS[0] += 1
    y = good(x)
    y[1, 1] += float(CALLS[0])
    return y


def zero_filled(x):
    acc = torch.zeros(x.shape, dtype=x.dtype)
    acc += x
    return acc + torch.full((x.shape[1],), 3.0)


def zero_store_past(x):
    acc = torch.zeros(x.shape, dtype=x.dtype)
    _poke(acc, (acc.storage_offset() + acc.numel()) * acc.element_size(), 0)        # a zero is not the pattern either
    return acc
'''


@pytest.fixture()
def fake():
    m = types.ModuleType("fake_ops")
    exec(compile(FAKE_SRC, "fake_ops.py", "exec"), m.__dict__)
    return m


def _x():
    return torch.arange(12, dtype=torch.float32).view(3, 4) / 7 + 0.5


def _launch(fake, op, x=None, **kw):
    x = _x() if x is None else x
    return lg.check_launches([fake], lambda run: getattr(fake, op)(run.place(x)), **kw)


def test_a_correct_op_passes_and_its_allocations_are_named(fake):
    names = _launch(fake, "good", declared=("good", "_scratch"))
    assert {"good", "_scratch"} <= names
    _launch(fake, "zero_filled", declared=("zero_filled",))
    with pytest.raises(lg.GuardError, match="no allocation was recorded for .'linear'."):
        _launch(fake, "good", declared=("linear",))
    assert fake.torch is torch                       # the proxy is gone


@pytest.mark.parametrize("op,message,owner", [
    ("store_past", r"store past the end \(first damaged guard byte \+0\)", "good"),
    ("store_before", r"store in front \(last damaged guard byte -1\)", "good"),
    ("unwritten", r"differs from the plain launch in \d+ byte\(s\), first at element 11, last at element 11", "unwritten"),
    ("stale_scratch", r"differs from the plain launch .* first at element 8, last at element 11", "stale_scratch"),
    ("read_past", r"differs from the plain launch .* first at element 11, last at element 11", "read_past"),
    ("clobber", r"input modified at byte \d+", "call"),
    ("drifting", r"differs from the plain launch .* first at element 5, last at element 5", "good"),
    ("zero_store_past", r"store past the end \(first damaged guard byte \+0\)", "zero_store_past"),
])
def test_each_planted_fault_is_reported_with_its_wrapper(fake, op, message, owner):
    def call(run):
        return getattr(fake, op)(run.place(_x()))

    with pytest.raises(lg.GuardError, match=message) as err:
        lg.check_launches([fake], call)
    assert f"by {owner}" in str(err.value), str(err.value)
    assert fake.torch is torch


def test_patterns_read_as_documented():
    """0xFF: NaN in bf16 / fp16 / fp32, -1 in integers; 0x7B: large and finite in the three float types, a large positive
    integer."""
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert bool(torch.isnan(lg.Guard(0xFF).empty(5, dtype=dt)).all())
        v = lg.Guard(0x7B).empty(5, dtype=dt).double()
        assert bool(torch.isfinite(v).all()) and float(v.min()) > 6e4
    for dt in (torch.int32, torch.int64):
        assert bool((lg.Guard(0xFF).empty(5, dtype=dt) == -1).all())
        assert int(lg.Guard(0x7B).empty(5, dtype=dt).min()) > 2 ** 30


def test_views_keep_shape_stride_offset_and_alignment():
    g = lg.Guard(0xFF)
    fused = torch.randn(2, 5, 3 * 8 + 4)
    q, k = g.place(fused[..., :8]), g.place(fused[..., 8:16])
    assert q.stride() == fused[..., :8].stride() and k.storage_offset() - q.storage_offset() == 8
    assert q.untyped_storage().data_ptr() == k.untyped_storage().data_ptr()            # one copy per storage
    assert torch.equal(q, fused[..., :8]) and torch.equal(k, fused[..., 8:16])
    assert q.data_ptr() == g.bufs[0].raw.data_ptr() + lg.GUARD and lg.GUARD % 512 == 0     # the allocator's alignment kept
    t = g.torch.empty_strided((3, 4), (8, 1), dtype=torch.float32)
    assert t.stride() == (8, 1) and t.data_ptr() % 512 == g.bufs[-1].raw.data_ptr() % 512
    z = g.torch.zeros(3, 4)
    assert z.dtype == torch.float32 and float(z.abs().sum()) == 0.0
    assert g.torch.float32 is torch.float32 and g.torch.cuda is torch.cuda
    assert g.torch.empty(4, pin_memory=False).shape == (4,)          # other keywords: the real call
    g.verify()
    out = g.inout(fused[0])
    out += 1
    g.verify()                                                       # an in/out tensor may change
    assert g.owner_of(out).kind == "placed (in/out)"


# ------------------------------------------------------------------------------------------------ the wrappers' source

# Functions of ops.py that allocate and run under byte guards of their own already (the uint8 kernels, out of this
# harness' scope): name -> the test that fills every buffer they write with 0xA5 and checks the bytes around each region.
GUARDED_ELSEWHERE = {
    "_u8_buf": "tests/test_native_gpu.py (native resize: tmp and both packed outputs pre-filled with 0xA5)",
    "seg_native": "tests/test_native_gpu.py (native resize, 0xA5 around every packed region)",
    "seg_labels_native": "tests/test_nway_native_gpu.py (0xA5 around every (class, image) region)",
    "seg_labels_cand_native": "tests/test_candidates_native_gpu.py (0xA5 guards inside and around tmp / out_u8 / labels)",
    "tiles_cut": "tests/test_tiled_gpu.py (SENT = 0xA5 around the cut windows)",
    "tiles_merge": "tests/test_tiled_gpu.py (SENT = 0xA5 around the merged image)",
    "tiles_labels_cand": "tests/test_tiled_candidates_gpu.py (SENT = 0xA5 around labels / counts / mx / area)",
}
ALLOCATORS = {"empty", "empty_like", "empty_strided", "zeros", "zeros_like", "full"}


def _allocating_functions(path):
    """{top-level function or method name: [line numbers of torch.<allocator>(...) calls]} of a wrapper module, after
    asserting that nothing there allocates behind the proxy's back."""
    tree = ast.parse(open(path).read())
    found = {}

    def walk(node, owner):
        for child in ast.iter_child_nodes(node):
            name = owner
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) and owner is None:
                name = child.name
            if isinstance(child, ast.ImportFrom):
                assert (child.module or "").split(".")[0] != "torch", f"{path}:{child.lineno}: `from torch import` escapes the proxy"
            if isinstance(child, ast.Import):
                for a in child.names:
                    assert a.name != "torch" or a.asname is None, f"{path}:{child.lineno}: torch imported under another name"
            if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute):
                f = child.func
                assert not f.attr.startswith("new_"), f"{path}:{child.lineno}: .{f.attr}() allocates behind the proxy"
                if f.attr in ALLOCATORS and isinstance(f.value, ast.Name) and f.value.id == "torch":
                    assert name is not None, f"{path}:{child.lineno}: allocation at module level"
                    found.setdefault(name, []).append(child.lineno)
            walk(child, name)

    for top in tree.body:
        if isinstance(top, ast.ClassDef):
            walk(top, None)
        elif isinstance(top, (ast.FunctionDef, ast.AsyncFunctionDef)):
            walk(top, top.name)
        else:
            walk(ast.Module(body=[top], type_ignores=[]), None)
    return found


def test_every_allocation_of_the_wrappers_is_reachable_and_declared():
    import test_launch_guard_gpu as gpu_cases
    declared = set(gpu_cases.ALL_DECLARED)
    seen = {}
    for mod in ("ops.py", "ops_bwd.py"):
        seen.update(_allocating_functions(os.path.join(ROOT, "diffews_amd", mod)))
    assert len(seen) > 40 and {"linear", "_gemm_launch", "_ws", "flush", "mse_loss", "zeros"} <= set(seen), sorted(seen)
    for name, why in GUARDED_ELSEWHERE.items():
        assert name in seen and name not in declared, name
        path = why.split()[0].split("::")[0]
        assert os.path.isfile(os.path.join(ROOT, path)) and "0xA5" in open(os.path.join(ROOT, path)).read(), why
    missing = sorted(set(seen) - declared - set(GUARDED_ELSEWHERE))
    assert not missing, f"functions that allocate and that no guarded GPU case declares: {missing}"
    assert declared <= set(seen), f"declared but not allocating: {sorted(declared - set(seen))}"
