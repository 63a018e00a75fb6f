"""Rows of the refusal table (tests/op_args_cases.py) on device tensors, at least one per kernel family: a caller-supplied
output that is too small or of the wrong dtype, or one host tensor among device tensors.  Each call is refused with the
wrapper's ValueError before anything is launched, and every buffer of the call, pre-filled with 0xA5, is byte-identical
afterwards.  Valid calls are the rest of the GPU suite's business."""
import types

import pytest
import torch

import op_args_cases as cases

pytestmark = pytest.mark.gpu

HOST_MIRRORS = ("tab_host", "table_host", "planes_host")

# (function, index among its cases, argument, defect or "host", family)
PICKS = [
    ("ops.linear", 0, "out", "shape", "GEMM: a result of 4 x 16 through a pointer to 4 x 15"),
    ("ops.linear", 0, "out", "dtype", "GEMM"),
    ("ops_bwd.gemm_tn", 0, "out", "shape", "GEMM, weight gradient"),
    ("ops.conv_small", 0, "out", "dtype", "conv"),
    ("ops.conv3x3", 0, "residual", "host", "conv"),
    ("ops.fsa_attention", 0, "out", "shape", "attention forward"),
    ("ops_bwd.attention_bwd", 0, "dk_out", "dtype", "attention backward"),
    ("ops.groupnorm", 0, "gamma", "host", "norm forward"),
    ("ops_bwd.groupnorm_bwd", 0, "dgamma", "shape", "norm backward"),
    ("ops_bwd.to_f32", 0, "out", "shape", "pointwise"),
    ("ops_bwd.adamw", 0, "exp_avg", "host", "pointwise, optimizer"),
    ("ops.seg_native", 0, "pred_out", "shape", "native seg wrapper"),
    ("ops.tiles_cut", 0, "out", "dtype", "tiled"),
    ("ops.seg_components", 0, "ids", "shape", "object stage"),
    ("ops.seg_boundary", 0, "dist", "host", "object stage"),
]


def _walk(v, f, name=None):
    """v with f applied to every tensor in it (dicts by key, lists, tuples and the targets stand-in included)."""
    if isinstance(v, torch.Tensor):
        return f(name, v)
    if isinstance(v, dict):
        return {k: _walk(x, f, k) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_walk(x, f, name) for x in v)
    if isinstance(v, types.SimpleNamespace):
        return types.SimpleNamespace(**_walk(vars(v), f))
    return v


def _to_device(name, t):
    return t if name in HOST_MIRRORS else t.cuda()


def _fill(name, t):
    if t.is_cuda and t.is_contiguous() and t.numel():
        t.view(torch.uint8).fill_(0xA5)
    return t


@pytest.mark.parametrize("fn,index,name,defect,family", PICKS, ids=[f"{p[0]}-{p[2]}-{p[3]}" for p in PICKS])
def test_a_bad_buffer_is_refused_on_the_device_and_nothing_is_written(hip_lib, fn, index, name, defect, family):
    from diffews_amd import ops, ops_bwd
    case = [c for c in cases.CASES if c.fn == fn][index]
    kw = _walk(case.valid(), _to_device)
    if defect == "host":
        kw[name] = kw[name].cpu()
        want = rf"^{case.wrapper}: all tensors must be device tensors on one cuda device.*{name} lies on cpu"
    else:
        kw[name] = cases.DEFECTS[defect](kw[name])
        want = case.pattern(cases.Row(name, defect))
    kw = _walk(kw, _fill)
    seen = []
    _walk(kw, lambda n, t: seen.append((n, t, t.cpu().clone())))
    assert len(seen) >= 2 and any(n == name for n, _, _ in seen)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match=want):
        case.call({"ops": ops, "ops_bwd": ops_bwd}, kw)
    torch.cuda.synchronize()
    for n, t, before in seen:
        now = t.cpu()
        assert now.dtype == before.dtype and now.shape == before.shape, n
        same = now.contiguous().view(torch.uint8) if now.numel() else now
        assert torch.equal(same, before.contiguous().view(torch.uint8) if before.numel() else before), f"{fn}: the refused call wrote to {n}"


def test_the_picks_cover_every_family():
    families = " ".join(p[4] for p in PICKS)
    for f in ("GEMM", "conv", "attention forward", "attention backward", "norm forward", "norm backward", "pointwise",
              "native seg wrapper", "tiled", "object stage"):
        assert f in families, f
    assert len(PICKS) >= 12
