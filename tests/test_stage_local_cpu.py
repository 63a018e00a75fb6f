"""Proves the bar of the stage-local parity tests (tests/stage_local.py) with the oracle alone, no GPU.

For the tiny UNet and the tiny VAE with loud weights, every tensor of the state dict is given every applicable
single-tensor fault (what a wiring or packing mistake in unet.py / vae.py / train.py / packing.py amounts to); the one
oracle stage that owns the tensor is re-run on its recorded input, and the change of its output is expressed as a
multiple f of the stage's own yardstick e_low (the oracle stage run by torch in the storage dtype vs its fp32 run).
The GPU test allows the engine k * e_low per stage and image, so f >= 2 k + 1 means: a faulty engine sits at least
(f - k) e_low >= (k + 1) e_low from the oracle and fails.

fp16: no exception.  bf16: at most 1 % of the faults may fall below the bar, each listed by name below (bf16 and fp16
share every line of the Python wiring, so the fp16 guarantee is the decisive one).
"""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import stage_local as sl  # noqa: E402

from diffews_amd import config, weights  # noqa: E402
from oracle.unet import OracleUNet  # noqa: E402
from oracle.vae import OracleVAE  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]

# bf16 faults allowed below 2 k + 1 (at most 1 % of the model's faults): "<fault class> <tensor>".  All sit around the
# 2-token attn2 of a transformer block: its LayerNorm (norm2) and the exchange of the two attention output biases, whose
# difference is small against the block's bf16 rounding noise (e_low 2 - 6e-3).  In fp16 the same faults are at f >= 11.
_T = "transformer_blocks.0."
BF16_EXCEPTIONS = {
    "unet": {f"exchange:{p}{_T}attn2.to_out.0.bias {p}{_T}attn1.to_out.0.bias"
             for p in ("up_blocks.3.attentions.2.", "down_blocks.0.attentions.0.", "up_blocks.2.attentions.0.")}
    | {f"ablation {p}{_T}norm2.bias" for p in ("up_blocks.2.attentions.0.", "up_blocks.3.attentions.2.", "up_blocks.2.attentions.1.")}
    | {f"ablation {p}{_T}norm2.weight" for p in ("down_blocks.1.attentions.1.", "down_blocks.0.attentions.1.")},
    "vae": set(),
}


def _unet(dt, loud=True, hw=16, s=2):
    ucfg = config.get("tiny_unet")
    shapes = weights.unet_param_shapes(ucfg)
    sd = sl.loud_state_dict(shapes, 1234, round_to=dt) if loud else weights.synthetic_unet_state_dict(ucfg, round_to=dt)
    ou = OracleUNet(**sl.kw(ucfg))
    ou.load_state_dict(sd)
    ou.eval()
    te = weights.synthetic_text_embed(ucfg).to(dt).float()
    g = torch.Generator().manual_seed(1)
    zr = torch.randn(s, 8, hw, hw, generator=g) * 0.5
    zq = torch.randn(1, 4, hw, hw, generator=g) * 0.5
    return ou, sd, shapes, zr, zq, te


def _vae(dt):
    vcfg = sl.vae_config()
    shapes = weights.vae_param_shapes(vcfg)
    sd = sl.loud_state_dict(shapes, 4321, round_to=dt)
    ov = OracleVAE(**sl.kw(vcfg))
    ov.load_state_dict(sd)
    ov.eval()
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(4)) * 2 - 1
    return ov, sd, shapes, x


def _check_partition(rec, shapes):
    owner = rec.owner()
    assert set(owner) == set(shapes), sorted(set(shapes) ^ set(owner))[:5]
    twice = {k: v for k, v in owner.items() if len(v) != 1}
    assert not twice, twice
    for st in rec.stages.values():      # every stage ran, and owns something
        assert st.rec and st.owned, st.name
    return {k: v[0] for k, v in owner.items()}


def _sweep(what, rec, sd, shapes, dt, extra=None):
    """Every fault of every tensor -> rows (f, class, tensor, stage); asserts the bar."""
    owner = _check_partition(rec, shapes)
    elow = rec.e_low(dt)
    rows, unseen = [], []
    for name in shapes:
        st = rec.stages[owner[name]]
        faults = sl.faults_of(name, sd, st.owned)
        faults += [("temb_slice", f) for f in (extra or {}).get(name, [])]
        bar = 2 * sl.k_of(dt, st.kind) + 1
        for cls, fault in faults:
            f = sl.fault_effect(rec, st.name, fault, elow, enough=bar)
            if sl.unobservable(cls, name):      # mathematically without effect: assert that, instead of the bar
                assert f < 0.1, (cls, name, f)
                unseen.append(cls + " " + name)
                continue
            rows.append((f, cls, name, st.name))
    lows = [l for v in elow.values() for l in v]
    mins = collections.defaultdict(lambda: (float("inf"), ""))
    for f, cls, name, stage in rows:
        c = cls.split(":")[0]
        mins[c] = min(mins[c], (f, cls + " " + name))
    print(f"\n{what} {dt}: {len(shapes)} tensors, each owned by exactly one of {len(rec.stages)} stages; {len(rows)} faults; "
          f"e_low {min(lows):.2e} .. {max(lows):.2e}")
    for c, (f, n) in sorted(mins.items()):
        print(f"  min f  {c:13s} {f:9.2f}   {n}")
    for n in unseen:
        print(f"  without effect on the stage's function (softmax shift invariance), not counted: {n}")
    # the bar of a fault is set by the allowance of the stage kind that owns the tensor
    below = sorted((f, cls + " " + name) for f, cls, name, stage in rows
                   if not f >= 2 * sl.k_of(dt, rec.stages[stage].kind) + 1)
    for f, n in below:
        print(f"  below 2k+1: {f:6.2f}  {n}")
    if dt == torch.float16:
        assert not below, below
    else:
        names = {n for _, n in below}
        assert len(below) <= len(rows) // 100, (len(below), len(rows))
        assert names <= BF16_EXCEPTIONS[what], sorted(names - BF16_EXCEPTIONS[what])
    return rows


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_unet_every_tensor_fault_moves_its_stage(dt):
    ou, sd, shapes, zr, zq, te = _unet(dt)
    rec = sl.record_unet(ou, shapes, zr, zq, te.repeat(zr.shape[0], 1, 1), te)
    assert rec.order["support"][0] == "conv_in_ref" and rec.order["query"][0] == "conv_in"
    assert rec.order["support"][1:] == rec.order["query"][1:] and rec.order["query"][-1] == "head"
    _sweep("unet", rec, sd, shapes, dt, extra=sl.temb_slice_faults(sd))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_vae_every_tensor_fault_moves_its_stage(dt):
    ov, sd, shapes, x = _vae(dt)
    rec = sl.record_vae(ov, shapes, x)
    assert rec.order["encode"][0] == "encoder.conv_in" and rec.order["encode"][-2:] == ["encoder.head", "quant_conv"]
    assert rec.order["decode"][:2] == ["post_quant_conv", "decoder.conv_in"] and rec.order["decode"][-1] == "decoder.head"
    _sweep("vae", rec, sd, shapes, dt)


# ---------------------------------------------------------------------------------------------- backward

# Backward faults no check can see, "<class> <what>": at most 2 % of the (tensor, class) pairs.  The head of the support
# pass gets no gradient at all (its output is multiplied by zero), so the term it deposits on the last transformer's output
# is exactly zero and leaving it out changes nothing.
BWD_UNOBSERVABLE = {"arrived-drop up_blocks.3.attentions.2<-head support"}

_GREC = {}


def _grad_rec(dt, b, s, h, w):
    """The oracle's training graph with gradients, as the GPU test records it (same draws)."""
    if (dt, b, s, h, w) not in _GREC:
        ucfg = config.get("tiny_unet")
        shapes = weights.unet_param_shapes(ucfg)
        sd = sl.loud_state_dict(shapes, 1234, round_to=dt)
        ou = OracleUNet(**sl.kw(ucfg)); ou.load_state_dict(sd); ou.eval()
        te = weights.synthetic_text_embed(ucfg, tokens=77).to(dt).float()
        g = torch.Generator().manual_seed(1000 + 100 * b + 10 * s + w)
        zr = torch.randn(b * s, 8, h, w, generator=g) * 0.5
        zq = torch.randn(b, 4, h, w, generator=g) * 0.5
        target = torch.randn(b, 4, h, w, generator=g) * 0.5
        rec = sl.record_unet_grads(ou, shapes, zr, zq, te.repeat(b * s, 1, 1), te.repeat(b, 1, 1), target)
        _GREC[(dt, b, s, h, w)] = (rec, sd, shapes)
    return _GREC[(dt, b, s, h, w)]


def _dx_effect(rec, st, elow, fault=None, **kw):
    """Change of the stage's dx (against the recording) as a multiple of e_low_bwd: the largest over passes and images."""
    with sl.faulted(rec.model, fault or {}):
        dx, _ = st.grad_run(rec.model, **kw)
    return max(e / l for p, v in dx.items() for e, l in zip(sl.rel_images(v, st.grad[p]["dx"]), elow[(st.name, p)]) if l is not None)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_backward_faults_move_the_recorded_gradients(dt):
    """With the oracle alone: every fault class of the hand-written backward moves the quantity the GPU test records by at
    least (2 k_bwd + 1) * e_low_bwd (dx, parameter gradients), or beyond the sum of both rounding bounds (arrived).
    The inputs are the GPU test's 1 x 2-shot cases at 16x16 and 16x24 (a fault counts as seen when either input shows it:
    the engine runs both) and its 2 x 2-shot case for the episode-to-bank mapping."""
    scale = sl.LOSS_SCALE[dt]
    recs = [_grad_rec(dt, 1, 2, 16, 16)[0], _grad_rec(dt, 1, 2, 16, 24)[0]]
    sd = _grad_rec(dt, 1, 2, 16, 16)[1]
    lows = [r.e_low_bwd(dt, scale) for r in recs]
    rec = recs[0]
    # the recording itself: what the consumers of a stage output send back adds up to the total gradient there
    for (n, p), cons in rec.consumers.items():
        total = sum(rec.stages[c].grad[p]["dx"][:, lo:hi] for c, lo, hi in cons)
        dy = rec.stages[n].grad[p]["dy"]
        assert float((total - dy).abs().max()) <= 1e-5 * float(dy.abs().max()) + 1e-30, (n, p)
    wiring = ("transpose", "mirror", "kykx", "geglu_halves", "exchange")
    pairs, below, mins = 0, [], collections.defaultdict(lambda: (float("inf"), ""))

    def note(cls, what, f, bar):
        nonlocal pairs
        pairs += 1
        mins[cls] = min(mins[cls], (f, what))
        if not f >= bar:
            below.append((f, cls + " " + what))

    # (1) dx recomputed with one owned weight faulted (a wrong derived copy: W^T of a Linear, the mirrored conv weight)
    for n, st in rec.stages.items():
        if st.kind in ("stem", "time"):
            continue
        bar = 2 * sl.k_bwd(dt, st.kind + ".dx") + 1
        for name in st.owned:
            if sd[name].dim() < 2:
                continue
            for cls, fault in sl.faults_of(name, sd, [q for q in st.owned if sd[q].dim() >= 2]):
                if cls.split(":")[0] not in wiring:
                    continue
                f = 0.0
                for r, (ex, _) in zip(recs, lows):
                    f = max(f, _dx_effect(r, r.stages[n], ex, fault))
                    if f >= bar:
                        break
                note("dx-" + cls.split(":")[0], cls + " " + name, f, bar)
    # (2) a parameter gradient with the same permutations applied to the gradient itself
    owner = {k: v[0] for k, v in rec.owner().items()}
    for name in sd:
        st = rec.stages[owner[name]]
        bar = 2 * sl.k_bwd(dt, sl.grad_class(st.kind, name)) + 1
        per_input = [dict(sl.faults_of(name, r.pgrad, st.owned)) for r in recs]
        for cls in per_input[0]:
            if cls.split(":")[0] not in wiring:
                continue
            f = max(sl.rel_images(v[None], r.pgrad[k][None])[0] / ep[k]
                    for r, (_, ep), faults in zip(recs, lows, per_input) for k, v in faults[cls].items())
            note("grad-" + cls.split(":")[0], cls + " " + name, f, bar)
    # (3) arrived: one consumer's term missing; the two halves of a concat handed out crosswise
    seen = collections.OrderedDict()
    for r in recs:
        for (n, p), cons in r.consumers.items():
            ref, bound = sl.arrived_ref(r, n, p, dt, scale)
            for c, lo, hi in cons:
                kinds = [("arrived-drop", dict(drop=c))]
                if hi - lo < r.stages[c].rec[p][0][0].shape[1]:
                    kinds.append(("arrived-halves", dict(exchange=(c,))))
                for cls, kw_ in kinds:
                    bad, bbound = sl.arrived_ref(r, n, p, dt, scale, **kw_)
                    key = (cls, f"{n}<-{c} {p}")
                    seen[key] = seen.get(key, False) or bool(((bad - ref).abs() > bound + bbound).any())
    for (cls, what), ok in seen.items():
        note(cls, what, float("inf") if ok else 0.0, 1.0)
    # (4) the support rows' dx of a transformer without the bank term, or with the bank term of the other episode
    rec22 = _grad_rec(dt, 2, 2, 16, 16)[0]
    ex22 = rec22.e_low_bwd(dt, scale)[0]
    for n, st in rec22.stages.items():
        if st.kind == "transformer":
            bar = 2 * sl.k_bwd(dt, "transformer.dx") + 1
            note("bank-missing", n, _dx_effect(rec22, st, {k: v for k, v in ex22.items() if k[1] == "support"}, bank=False), bar)
            note("bank-other-episode", n, _dx_effect(rec22, st, ex22, flip_query=True), bar)
    print(f"\nbackward faults {dt}: {pairs} (tensor, class) pairs")
    for c, (f, what) in sorted(mins.items()):
        print(f"  min f  {c:20s} {f:9.2f}   {what}")
    for f, what in sorted(below):
        print(f"  below the bar: {f:6.2f}  {what}")
    names = {w for _, w in below}
    assert names <= BWD_UNOBSERVABLE, sorted(names - BWD_UNOBSERVABLE)
    assert len(BWD_UNOBSERVABLE) <= pairs // 50


def test_loud_draw_keeps_layout_and_surgery():
    ucfg = config.get("tiny_unet")
    shapes = weights.unet_param_shapes(ucfg)
    stock, loud = weights.synthetic_unet_state_dict(ucfg), sl.loud_state_dict(shapes, 1234)
    assert list(stock) == list(loud)
    for k in shapes:
        if sl.is_norm(k) or k.endswith("bias"):
            sig = 0.3 if sl.is_norm(k) else 0.5
            t = loud[k] - 1.0 if (sl.is_norm(k) and k.endswith("weight")) else loud[k]
            if t.numel() >= 64:
                assert 0.6 * sig < float(t.std()) < 1.4 * sig, k
        else:
            assert torch.equal(stock[k], loud[k]), k      # weight draws unchanged
    assert torch.equal(loud["conv_in_ref.weight"], loud["conv_in.weight"].repeat(1, 2, 1, 1) / 2)
    assert torch.equal(loud["conv_in_ref.bias"], loud["conv_in.bias"])


def test_whole_output_check_is_blind_to_most_tensors():
    """Why this file exists: with the stock synthetic weights, ablating ONE tensor moves the query-pass output of the
    whole UNet by less than the bf16 model tolerance (TOL_Z0 of test_model_gpu.py) for at least 300 of the 688 tensors
    (365 measured at 16x16 latents, 2-shot; run here at 8x8, 1-shot for time)."""
    tol = 2e-2
    dt = torch.bfloat16
    ou, sd, shapes, zr, zq, te = _unet(dt, loud=False, hw=8, s=1)

    def run():
        with torch.no_grad():
            ou.clear_attn_bank()
            ou(zr, 1, te, is_target=False)
            y = ou(zq, 1, te)
            ou.clear_attn_bank()
        return y
    base = run()
    quiet = 0
    for name in shapes:
        cls, fault = sl.faults_of(name, sd, [])[0]
        assert cls == "ablation"
        with sl.faulted(ou, fault):
            quiet += sl.rel_images(run(), base)[0] < tol
    print(f"\nablations invisible to the whole-output check at {tol}: {quiet} of {len(shapes)}")
    assert len(shapes) == 688 and quiet >= 300
