"""The LDS poisoner (tests/lds_poison.py) without a GPU: its HIP source compiles for gfx950; the launching entry points are
parsed from include/diffews_hip.h, are the entries of `_lib.SYMBOLS` the proxy poisons, and each of them is declared -- by a
case of tests/test_lds_poison_gpu.py or, in REACHED_BY, by wrapper functions of ops.py / ops_bwd.py that reach it and that the
launch-guard cases call (an AST scan, as in tests/test_launch_guard_cpu.py), so an entry point added later without a poisoned
case fails here; and the proxy on a fake handle: fill then call, arguments and return codes passed through, the rest of the
handle untouched, nothing issued while capturing, `_lib.lib` restored after an exception."""
import ast
import os
import re

import pytest

import lds_poison as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# launching entry point -> wrapper functions that reach it and that a case of tests/test_launch_guard_gpu.py (or a plan-test
# helper it runs) calls; check_launches poisons LDS in front of every one of them
REACHED_BY = {
    "dfw_gemm": ("linear", "bmm_nt", "conv3x3"),
    "dfw_gemm_tn": ("gemm_tn",),
    "dfw_conv_up2x": ("conv3x3_up2x",),
    "dfw_conv_small": ("conv_small",),
    "dfw_fsa_attention": ("fsa_attention",),
    "dfw_fsa_attention_sets": ("fsa_attention_sets",),
    "dfw_fsa_attention_ragged": ("fsa_attention_ragged",),
    "dfw_fsa_attention_routed": ("fsa_attention_routed",),
    "dfw_cross_attention": ("cross_attention",),
    "dfw_vae_attention": ("vae_attention",),
    "dfw_fsa_attention_bwd": ("fsa_attention_bwd",),
    "dfw_attention_bwd": ("attention_bwd",),
    "dfw_cross_attention_bwd": ("cross_attention_bwd",),
    "dfw_groupnorm": ("groupnorm",),
    "dfw_groupnorm_bwd": ("groupnorm_bwd",),
    "dfw_layernorm": ("layernorm",),
    "dfw_layernorm_bwd": ("layernorm_bwd",),
    "dfw_softmax_rows": ("softmax_rows",),
    "dfw_softmax_groups": ("softmax_groups",),
    "dfw_transpose": ("transpose",),
    "dfw_concat_channels": ("concat_channels",),
    "dfw_convert_f32": ("to_storage",),
    "dfw_split_f32": ("split_storage",),
    "dfw_zero": ("zeros",),
    "dfw_timestep_embedding": ("timestep_embedding",),
    "dfw_seg_postprocess_ex": ("seg_postprocess",),
    "dfw_seg_labels": ("seg_labels",),
    "dfw_seg_labels_cand": ("seg_labels_cand",),
    "dfw_colsum": ("colsum",),
    "dfw_table_write": ("flush",),
    "dfw_colsum_batch": ("flush",),
    "dfw_geglu": ("geglu_fwd", "geglu_bwd"),
    "dfw_elementwise": ("add", "pool2x2_sum", "slice_channels", "zero_stuff2x"),
    "dfw_silu": ("silu",),
    "dfw_nchw_to_nhwc": ("nchw_to_nhwc",),
    "dfw_mse_loss": ("mse_loss",),
    "dfw_loss_grad": ("loss_grad",),
    "dfw_sumsq": ("sumsq",),
    "dfw_adamw": ("adamw",),
    "dfw_weight_relayout": ("linear_wt", "conv3x3_wd"),
    "dfw_weight_relayout_batch": ("weight_relayout_batch",),
}
NOT_LAUNCHING = ("_workspace_bytes", "_kernel_name", "_rounds", "_block", "_tile", "_gn_chunks", "_plan", "_ksize", "_coeffs", "_ksize_ex", "_coeffs_ex")


def test_the_poisoner_compiles_for_gfx950(tmp_path):
    so = lp.build(str(tmp_path))
    assert os.path.getsize(so) > 0 and lp.build(str(tmp_path)) == so
    assert any(f == "--offload-arch=gfx950" for f in lp._flags())


# ------------------------------------------------------------------------------------------------ which entry points launch

def test_launching_entry_points_come_from_the_header():
    from diffews_amd import _lib
    names = lp.launching_from_header()
    assert len(names) == len(set(names)) > 50
    assert set(names) <= set(_lib.SYMBOLS), sorted(set(names) - set(_lib.SYMBOLS))
    proxy = lp.LibProxy(object(), 0)
    assert {n for n in _lib.SYMBOLS if n in proxy._names} == set(names)
    for n in names:
        assert _lib.SYMBOLS[n][0] is _lib._i32 and _lib.SYMBOLS[n][1][-1] is _lib._vp, n        # rc = f(..., stream)
        assert not n.endswith(NOT_LAUNCHING), n
    for n in set(_lib.SYMBOLS) - set(names):
        assert n.endswith(NOT_LAUNCHING) or n in ("dfw_configure", "dfw_get_config", "dfw_version", "dfw_error_string",
                                                  "dfw_graph_memset_nodes"), n
    assert {"dfw_gemm", "dfw_fsa_attention_routed", "dfw_tiles_labels_cand", "dfw_seg_contours", "dfw_mask_to_tensor"} <= set(names)


def _wrappers(path):
    """{function or method name: (dfw_ names it names, names it calls)} of a wrapper module."""
    tree = ast.parse(open(path).read())
    out = {}
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef)]
    funcs += [m for c in tree.body if isinstance(c, ast.ClassDef) for m in c.body if isinstance(m, ast.FunctionDef)]
    for fn in funcs:
        direct, calls = out.setdefault(fn.name, (set(), set()))
        for n in ast.walk(fn):
            if isinstance(n, ast.Attribute) and n.attr.startswith("dfw_"):
                direct.add(n.attr)
            if isinstance(n, ast.Call):
                calls.add(n.func.id if isinstance(n.func, ast.Name) else n.func.attr if isinstance(n.func, ast.Attribute) else "")
    return out


def _reach(table, name, seen):
    if name in seen or name not in table:
        return set()
    seen.add(name)
    direct, calls = table[name]
    return set(direct).union(*(_reach(table, c, seen) for c in calls))


def test_every_launching_entry_point_has_a_poisoned_case():
    import test_launch_guard_gpu as guard_cases
    import test_lds_poison_gpu as stage_cases
    launching = set(lp.launching_from_header())
    declared = set(stage_cases.CASES_DECLARED)
    assert declared <= launching, sorted(declared - launching)
    assert not declared & set(REACHED_BY), sorted(declared & set(REACHED_BY))
    assert set(REACHED_BY) <= launching, sorted(set(REACHED_BY) - launching)
    missing = sorted(launching - declared - set(REACHED_BY))
    assert not missing, f"launching entry points without a poisoned case: {missing}"
    table = {}
    for mod in ("ops.py", "ops_bwd.py"):
        table.update(_wrappers(os.path.join(ROOT, "diffews_amd", mod)))
    # where the launch-guard cases call wrappers: their own module and the plan-test modules whose run helpers they use
    src = open(guard_cases.__file__).read()
    for m in re.findall(r"^import (test_\w+) as", src, flags=re.M):
        src += open(os.path.join(ROOT, "tests", m + ".py")).read()
    for entry, wrappers in REACHED_BY.items():
        for w in wrappers:
            assert entry in _reach(table, w, set()), f"{w} does not reach {entry}"
            assert w in guard_cases.ALL_DECLARED or re.search(rf"\.{w}\(", src), f"no launch-guard case calls {w} (for {entry})"


# ------------------------------------------------------------------------------------------------ the proxy on a fake handle

class _Fake:
    def __init__(self, log):
        self.log = log
        self.constant = 7

    def dfw_gemm(self, a, stream):
        self.log.append(("dfw_gemm", a, stream))
        return 0

    def dfw_layernorm(self, a, stream):
        self.log.append(("dfw_layernorm", a, stream))
        return 3

    def dfw_gemm_workspace_bytes(self, a):
        self.log.append(("dfw_gemm_workspace_bytes", a))
        return 4096

    def dfw_configure(self, cfg):
        self.log.append(("dfw_configure", cfg))
        return 0


def _proxy(capturing=lambda: False):
    log = []
    fake = _Fake(log)
    return fake, log, lp.LibProxy(fake, 0x7B7B7B7B, fill=lambda w: log.append(("fill", w)), capturing=capturing)


def test_proxy_fills_then_calls_and_passes_everything_through():
    fake, log, proxy = _proxy()
    args = object()
    assert proxy.dfw_gemm(args, 11) == 0 and proxy.dfw_layernorm(args, 12) == 3
    assert log == [("fill", 0x7B7B7B7B), ("dfw_gemm", args, 11), ("fill", 0x7B7B7B7B), ("dfw_layernorm", args, 12)]
    assert log[1][1] is args and proxy.poisoned == {"dfw_gemm", "dfw_layernorm"}
    del log[:]
    assert proxy.dfw_gemm_workspace_bytes(args) == 4096 and proxy.dfw_configure(None) == 0 and proxy.constant == 7
    assert log == [("dfw_gemm_workspace_bytes", args), ("dfw_configure", None)]                 # no fill
    assert proxy.dfw_gemm_workspace_bytes.__self__ is fake                                      # the handle's own function
    with pytest.raises(AttributeError):
        proxy.dfw_missing
    with pytest.raises(AttributeError):
        proxy.constant = 8


def test_proxy_issues_nothing_while_capturing():
    state = [True]
    _, log, proxy = _proxy(capturing=lambda: state[0])
    assert proxy.dfw_gemm(None, 5) == 0
    assert log == [("dfw_gemm", None, 5)] and not proxy.poisoned
    state[0] = False
    proxy.dfw_gemm(None, 5)
    assert log[1:] == [("fill", 0x7B7B7B7B), ("dfw_gemm", None, 5)] and proxy.poisoned == {"dfw_gemm"}


def test_installed_swaps_lib_and_restores_it_after_an_exception():
    from diffews_amd import _lib
    real = _lib.lib
    log = []
    fake = _Fake(log)
    with pytest.raises(ZeroDivisionError):
        with lp.installed(0xFF, real=fake, fill=lambda w: log.append(("fill", w)), capturing=lambda: False) as proxy:
            assert _lib.lib() is proxy and _lib.lib is not real
            _lib.lib().dfw_gemm(1, 2)
            1 / 0
    assert _lib.lib is real
    assert log == [("fill", 0xFFFFFFFF), ("dfw_gemm", 1, 2)]
    assert lp.word_of(0x7B) == 0x7B7B7B7B and lp.word_of(0) == 0


def test_check_launches_has_the_switch_and_skips_lds_without_a_device():
    """On a machine without a device lds=True poisons nothing (there is no LDS); a callable is installed as given, once per
    pattern launch, and on a difference once more with zero to tell LDS from memory."""
    import contextlib
    import types

    import torch

    import launch_guard as lg
    seen = []

    @contextlib.contextmanager
    def fake_lds(pattern):
        seen.append(pattern)
        yield types.SimpleNamespace(poisoned={"dfw_fake"})

    x = torch.arange(6, dtype=torch.float32)
    lg.check_launches([], lambda run: run.place(x) * 2, lds=fake_lds)
    assert seen == [0xFF, 0x7B]
    del seen[:]
    state = types.SimpleNamespace(lds=0)

    @contextlib.contextmanager
    def leaky_lds(pattern):                                   # an op whose result depends on what "LDS" holds
        seen.append(pattern)
        state.lds = pattern
        try:
            yield types.SimpleNamespace(poisoned={"dfw_fake"})
        finally:
            state.lds = 0

    with pytest.raises(lg.GuardError, match=r"LDS pattern 0xFF \(word 0xFFFFFFFF in every CU's LDS in front of dfw_fake\): result 0 .* reads LDS it has not written"):
        lg.check_launches([], lambda run: run.place(x) + state.lds, lds=leaky_lds)
    assert seen == [0xFF, 0x00]
    if not torch.cuda.is_available():
        assert lg._lds_installer(True) is None
    assert lg._lds_installer(False) is None
