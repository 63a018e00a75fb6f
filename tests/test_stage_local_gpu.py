"""The engine, stage by stage (tests/stage_local.py): MyUNet2DConditionModel, AutoencoderKL and UNetTrainer._forward run
teacher-forced on the oracle's recorded stage inputs, loud weights, tiny configs, fp16 and bf16; every stage output is
compared per image with the oracle's fp32 output and must stay within k * e_low, e_low being the same oracle stage run by
torch in the storage dtype.  tests/test_stage_local_cpu.py proves that every single-tensor fault moves its stage by at
least (2 k + 1) * e_low, so these assertions pin every parameter of the three hand-written copies of the wiring.

The trainer's hand-written backward is pinned the same way (test_trainer_backward_stage_by_stage): the oracle's two-pass
training graph is recorded with its gradients, the engine's tape walks teacher-forced -- every stage receives the oracle's
dy at its output and its dx is judged alone against k_bwd * e_low_bwd -- and the wiring between the stages is judged by the
gradient that ARRIVED at each stage output before it was replaced, which must be the sum of what the consumers deposited
to within one rounding per add.  Every key of grad_dict() is judged per tensor.  Known limit: a stage's forced input is a
fresh tensor, so `tape.take` ACROSS a stage boundary (the dx_add fusion of a stage's first norm with the gradient its input
already has from another consumer) is not exercised here and stays with the whole-step tests of test_backward_gpu.py;
`take` inside a stage (a resnet's norm1 receiving conv2's residual term) is.

A failure names the stage prefix, the pass, the image and the ratio.  Each test prints the worst ratio per stage class;
the module prints the aggregate per dtype when it finishes (the table of DESIGN.md section 4).
"""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import stage_local as sl  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_Z0 = {torch.float16: 2e-3, torch.bfloat16: 2e-2}   # the whole-output tolerance of test_model_gpu.py
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for dt, tab in _WORST.items():
        print(f"\nworst rel / e_low per stage class, {dt}:")
        for kind, (r, name, p, i) in sorted(tab.items()):
            print(f"  {kind:12s} {r:5.2f}   (k = {k_of_any(dt, kind):.2f})   {name}, {p} pass, image {i}")


def k_of_any(dt, kind):
    """The allowance a row class is judged by: forward stage kinds, backward classes, `arrived` (error / its own bound)."""
    return 1.0 if kind == "arrived" else sl.k_bwd(dt, kind) if "." in kind else sl.k_of(dt, kind)


def _finish(rec, tf, dt, label):
    tf.check_order()
    rows, bad = sl.compare(rec, tf, dt, label)
    sl.worst_by_kind(rows, _WORST.setdefault(dt, {}))
    print(f"\n{label} [{dt}]: " + ", ".join(f"{k} {v[0]:.2f}" for k, v in sorted(sl.worst_by_kind(rows).items())))
    return rows, bad


_CTX = {}


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def ctx(request, hip_lib):
    return _make_ctx(request.param)


def _make_ctx(dt):
    if dt not in _CTX:
        _CTX[dt] = _build_ctx(dt)
    return _CTX[dt]


def _build_ctx(dt):
    from diffews_amd import config, weights
    from oracle.unet import OracleUNet
    from oracle.vae import OracleVAE
    ucfg, vcfg = config.get("tiny_unet"), sl.vae_config()
    ushapes, vshapes = weights.unet_param_shapes(ucfg), weights.vae_param_shapes(vcfg)
    usd = sl.loud_state_dict(ushapes, 1234, round_to=dt)
    vsd = sl.loud_state_dict(vshapes, 4321, round_to=dt)
    ou = OracleUNet(**sl.kw(ucfg)); ou.load_state_dict(usd); ou.eval()
    ov = OracleVAE(**sl.kw(vcfg)); ov.load_state_dict(vsd); ov.eval()
    te = {L: weights.synthetic_text_embed(ucfg, tokens=L).to(dt).float() for L in (2, 77)}
    recs = {}

    def unet_rec(b, s, L, hw=16):
        """The oracle's two passes on b episodes of s support images, recorded once per shape."""
        key = (b, s, L, hw)
        if key not in recs:
            g = torch.Generator().manual_seed(100 + 10 * b + s)
            zr = torch.randn(b * s, 8, hw, hw, generator=g) * 0.5
            zq = torch.randn(b, 4, hw, hw, generator=g) * 0.5
            rec = sl.record_unet(ou, ushapes, zr, zq, te[L].repeat(b * s, 1, 1), te[L].repeat(b, 1, 1))
            rec.e_low(dt)
            recs[key] = (rec, zr, zq)
        return recs[key]
    grecs = {}

    def grad_rec(b, s, h, w, scale):
        """The oracle's two-pass training graph with its gradients (77-token prompt, seeded target), once per shape."""
        key = (b, s, h, w)
        if key not in grecs:
            g = torch.Generator().manual_seed(1000 + 100 * b + 10 * s + w)
            zr = torch.randn(b * s, 8, h, w, generator=g) * 0.5
            zq = torch.randn(b, 4, h, w, generator=g) * 0.5
            target = torch.randn(b, 4, h, w, generator=g) * 0.5
            rec = sl.record_unet_grads(ou, ushapes, zr, zq, te[77].repeat(b * s, 1, 1), te[77].repeat(b, 1, 1), target)
            rec.e_low_bwd(dt, scale)
            grecs[key] = (rec, zr, zq)
        return grecs[key]
    return dict(dt=dt, ucfg=ucfg, vcfg=vcfg, usd=usd, vsd=vsd, ou=ou, ov=ov, te=te, unet_rec=unet_rec, grad_rec=grad_rec,
                ushapes=ushapes, vshapes=vshapes)


@pytest.fixture(scope="module")
def unet(ctx):
    from diffews_amd.unet import MyUNet2DConditionModel
    return MyUNet2DConditionModel(ctx["ucfg"], ctx["usd"], torch_dtype=ctx["dt"])


def _run_unet(unet, rec, zr, zq, te, form, folded):
    """One teacher-forced run of the engine in the given form -> the TeacherForce with the recorded stage outputs."""
    b, n_ref = zq.shape[0], zr.shape[0]
    ehs_r, ehs_q = (None, None) if folded else (te.repeat(n_ref, 1, 1).cuda(), te.repeat(b, 1, 1).cuda())
    unet.unfold_conditioning()
    unet.clear_attn_bank()
    try:
        with sl.TeacherForce(rec, unet) as tf:
            if form == "pair":
                tf.at("support", "query")
                if folded:
                    unet.fold_conditioning(1, te)
                unet.forward_pair(zr.cuda(), zq.cuda(), 1, ehs_r, ehs_q)
            else:
                tf.at("support")
                if folded:
                    unet.fold_conditioning(1, te)
                unet(zr.cuda(), 1, ehs_r, is_target=False)
                tf.at("query")
                unet(zq.cuda(), 1, ehs_q)
            torch.cuda.synchronize()
    finally:
        unet.clear_attn_bank()
    return tf


UNET_CASES = [
    # id, form, episodes, shots, prompt tokens, folded conditioning, fold_attn2
    ("two_pass-1shot", "two_pass", 1, 1, 2, False, True),
    ("two_pass-2shot", "two_pass", 1, 2, 2, False, True),
    ("two_pass-2x2shot", "two_pass", 2, 2, 2, False, True),
    ("pair-1shot", "pair", 1, 1, 2, False, True),
    ("pair-2x2shot", "pair", 2, 2, 2, False, True),
    ("two_pass-2shot-folded", "two_pass", 1, 2, 2, True, True),
    ("pair-2shot-folded", "pair", 1, 2, 2, True, True),
    ("pair-2shot-folded-attn2-unfolded", "pair", 1, 2, 2, True, False),
    ("two_pass-1shot-77tok", "two_pass", 1, 1, 77, False, True),
    ("pair-2shot-77tok-fold-refused", "pair", 1, 2, 77, True, True),
]


@pytest.mark.parametrize("case", UNET_CASES, ids=[c[0] for c in UNET_CASES])
def test_unet_stage_by_stage(ctx, unet, case):
    label, form, b, s, L, folded, fold_attn2 = case
    rec, zr, zq = ctx["unet_rec"](b, s, L)
    unet.fold_attn2 = fold_attn2
    try:
        tf = _run_unet(unet, rec, zr, zq, ctx["te"][L], form, folded)
        if folded:      # the fold is taken when it applies and refused for the 77-token prompt (heads * L > 64)
            want = fold_attn2 and L == 2
            assert all((t.fold2 is not None) == want for t in unet._transformers())
    finally:
        unet.fold_attn2 = True
        unet.unfold_conditioning()
    # every oracle stage ran in the engine, in both passes (folded: the time projection is made once, at fold time)
    want = {(n, p) for n, st in rec.stages.items() for p in st.rec}
    once = {("time", "query")} if folded else set()
    assert set(tf.out) - once == want - once, sorted(want ^ set(tf.out))
    rows, bad = _finish(rec, tf, ctx["dt"], "unet " + label)
    assert not bad, "\n".join(bad)


def test_unet_fp32_residual_stream(hip_lib):
    """residual_dtype=torch.float32 (the parity mode of fp16 storage): same stages, same yardstick."""
    from diffews_amd.unet import MyUNet2DConditionModel
    ctx = _make_ctx(torch.float16)
    un = MyUNet2DConditionModel(ctx["ucfg"], ctx["usd"], torch_dtype=torch.float16, residual_dtype=torch.float32)
    for form, b, s in (("two_pass", 1, 2), ("pair", 2, 2)):
        rec, zr, zq = ctx["unet_rec"](b, s, 2)
        tf = _run_unet(un, rec, zr, zq, ctx["te"][2], form, False)
        rows, bad = _finish(rec, tf, ctx["dt"], f"unet fp32-stream {form}")
        assert len(tf.out) == sum(len(st.rec) for st in rec.stages.values())
        assert not bad, "\n".join(bad)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("flash", [False, True, "auto"], ids=["materialised", "flash", "auto"])
def test_vae_stage_by_stage(ctx, flash, batch):
    from diffews_amd.vae import AutoencoderKL
    dt = ctx["dt"]
    if "vae" not in ctx:
        ctx["vae"] = AutoencoderKL(ctx["vcfg"], ctx["vsd"], torch_dtype=dt)
    vae = ctx["vae"]
    from diffews_amd import ops
    # "auto" takes the flash kernel for a token count off the 64 grid: 72 x 72 pixels -> 9 x 9 = 81 mid-block tokens
    # (which the materialised path cannot run); 64 x 64 -> 64 tokens for the two forced settings
    hw = 72 if flash == "auto" else 64
    if ("vrec", batch, hw) not in ctx:
        x = torch.rand(batch, 3, hw, hw, generator=torch.Generator().manual_seed(4 + batch)) * 2 - 1
        ctx[("vrec", batch, hw)] = (sl.record_vae(ctx["ov"], ctx["vshapes"], x), x)
    rec, x = ctx[("vrec", batch, hw)]
    z = rec.stages["post_quant_conv"].rec["decode"][0][0]
    vae.encoder.mid.att.flash = vae.decoder.mid.att.flash = flash
    flash_calls, orig = [], ops.vae_attention
    ops.vae_attention = lambda *a, **k: flash_calls.append(1) or orig(*a, **k)
    try:
        with sl.TeacherForce(rec, vae) as tf:
            tf.at("encode")
            vae.quant_conv(vae.encoder(x.cuda()))
            tf.at("decode")
            vae.decoder(vae.post_quant_conv(z.cuda()))
            torch.cuda.synchronize()
    finally:
        ops.vae_attention = orig
        vae.encoder.mid.att.flash = vae.decoder.mid.att.flash = "auto"
    assert len(flash_calls) == (0 if flash is False else 2)      # encoder + decoder mid attention on the path asked for
    assert len(tf.out) == len(rec.stages) == sum(len(st.rec) for st in rec.stages.values())
    rows, bad = _finish(rec, tf, dt, f"vae flash={flash} batch={batch}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shots", [1, 2])
def test_trainer_forward_stage_by_stage(ctx, shots):
    """UNetTrainer._forward (lock-step, 77-token prompt): parameters come from the flat master / shadow, so this covers
    ParamStore's offsets and the fused tp_w / kv_w_all tables."""
    from diffews_amd.train import UNetTrainer
    dt = ctx["dt"]
    if "trainer" not in ctx:
        ctx["trainer"] = UNetTrainer(ctx["ucfg"], ctx["usd"], torch_dtype=dt)
    tr = ctx["trainer"]
    rec, zr, zq = ctx["unet_rec"](1, shots, 77)
    te = ctx["te"][77]
    with sl.TeacherForce(rec, tr) as tf:
        tf.at("support", "query")
        tr._forward(zr.cuda(), zq.cuda(), 1, te.cuda(), ehs_ref=te.repeat(shots, 1, 1).cuda())
        torch.cuda.synchronize()
    assert len(tf.out) == sum(len(st.rec) for st in rec.stages.values())
    rows, bad = _finish(rec, tf, dt, f"trainer {shots}-shot")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- trainer backward

LOSS_SCALE = sl.LOSS_SCALE      # fp16 runs scaled by 1024: grad_scale / gs are under test
BWD_CASES = [
    # id, episodes, shots, latent h, w
    ("1x1-16x16", 1, 1, 16, 16),
    ("1x2-16x16", 1, 2, 16, 16),
    ("2x2-16x16", 2, 2, 16, 16),      # the episode-to-bank mapping and segs = B in the dtproj column sums
    ("1x2-16x24", 1, 2, 16, 24),      # levels 16x24, 8x12, 4x6, 2x3: non-square at every stride-2 and upsample conv
]


def _bwd_trainer(ctx):
    from diffews_amd.train import UNetTrainer
    if "trainer_bwd" not in ctx:
        ctx["trainer_bwd"] = UNetTrainer(ctx["ucfg"], ctx["usd"], torch_dtype=ctx["dt"], loss_scale=LOSS_SCALE[ctx["dt"]],
                                         dynamic_loss_scale=False)
    return ctx["trainer_bwd"]


def _run_trainer_bwd(tr, rec, zr, zq, te, zero_grad=True, fault=None):
    """One teacher-forced forward + backward of the trainer -> (TeacherForce, grad_dict() on the host)."""
    n_ref, b = zr.shape[0], zq.shape[0]
    with sl.TeacherForce(rec, tr) as tf, (fault(tf) if fault else contextlib.nullcontext()):
        tf.at("support", "query")
        c = tr._forward(zr.cuda(), zq.cuda(), 1, te.repeat(b, 1, 1).cuda(), zero_grad=zero_grad, ehs_ref=te.repeat(n_ref, 1, 1).cuda())
        tf.seed_head(c)
        tr._backward(c)
        torch.cuda.synchronize()
    return tf, {k: v.float().cpu() for k, v in tr.grad_dict().items()}


def _finish_bwd(rec, tf, grads, dt, label):
    rows, bad, failing = sl.compare_bwd(rec, tf, grads, dt, label)
    sl.worst_by_kind(rows, _WORST.setdefault(dt, {}))
    print(f"\n{label} [{dt}]: " + ", ".join(f"{k} {v[0]:.2f}" for k, v in sorted(sl.worst_by_kind(rows).items())))
    return rows, bad, failing


@pytest.mark.parametrize("case", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_trainer_backward_stage_by_stage(ctx, case):
    """UNetTrainer's tape, teacher-forced on the oracle's recorded gradients: every stage's dx per image, every tensor of
    grad_dict() and the gradient that arrived at every stage output (see the module docstring)."""
    label, b, s, h, w = case
    dt, tr = ctx["dt"], _bwd_trainer(ctx)
    rec, zr, zq = ctx["grad_rec"](b, s, h, w, tr.loss_scale)
    tf, grads = _run_trainer_bwd(tr, rec, zr, zq, ctx["te"][77])
    tf.check_order()
    # stage coverage: every stage of every pass sent a dx (the stems and the time MLP have no input gradient) and
    # received a gradient at its output (the head's is the seed); tensor coverage is asserted inside compare_bwd
    stages = {(n, p): st.kind for n, st in rec.stages.items() for p in st.rec}
    assert set(tf.dx) == {k for k, kind in stages.items() if kind not in ("stem", "time")}, sorted(set(stages) ^ set(tf.dx))
    assert set(tf.arrived) == set(rec.consumers) == {k for k, kind in stages.items() if kind not in ("head", "time")}
    assert set(grads) == set(ctx["usd"])
    rows, bad, failing = _finish_bwd(rec, tf, grads, dt, "trainer backward " + label)
    assert sum(r[0].endswith(".grad") for r in rows) == sum(v is not None for v in rec.e_low_bwd(dt, tr.loss_scale)[1].values())
    assert not bad, "\n".join(bad)
    if label == "1x2-16x16":
        # zero_grad=False adds the same gradients once more (P.acc routes every writer to accumulate): twice the first,
        # to the rounding of fp32 sums taken in another order (1e-5, as test_training_step_gradients_vs_oracle_autograd)
        tf2, grads2 = _run_trainer_bwd(tr, rec, zr, zq, ctx["te"][77], zero_grad=False)
        for k, g in grads.items():
            assert sl.rel_images(grads2[k][None], 2 * g[None])[0] < 1e-5, k


@contextlib.contextmanager
def _drop_residual(tf, stage):
    """The tape loses the first gradient sent to the stage's input: conv2's `tape.accum(residual, dy)` of a resnet
    without a shortcut conv."""
    from diffews_amd import train as T
    orig, seen = T._Tape.accum, []

    def accum(self, t, g):
        xf = tf.forced_in.get(stage)
        if xf is not None and not seen and self._key(t) == self._key(xf):
            seen.append(1)
            return None
        return orig(self, t, g)
    T._Tape.accum = accum
    try:
        yield
    finally:
        T._Tape.accum = orig
    assert seen


@contextlib.contextmanager
def _swap_cat_offsets(tf):
    """cat_bwd of the first concat the tape walks (up_blocks.3.resnets.2 reads [up_blocks.3.attentions.1 ; stem], 64 + 64
    channels) hands the two halves out crosswise."""
    from diffews_amd import ops_bwd
    orig, calls = ops_bwd.slice_channels, []

    def slice_channels(a, c0, Cc):
        calls.append(c0)
        if len(calls) <= 2:
            assert a.shape[-1] == 2 * Cc and c0 in (0, Cc)
            c0 = Cc - c0
        return orig(a, c0, Cc)
    ops_bwd.slice_channels = slice_channels
    try:
        yield
    finally:
        ops_bwd.slice_channels = orig
    assert len(calls) >= 2


@contextlib.contextmanager
def _wrong_derived_copy(tr, name, other):
    """_d("D", name) answers with the tap-mirrored copy of another conv of the same shape: the forward is untouched."""
    orig = tr._d
    tr._d = lambda kind, n: orig(kind, other if (kind, n) == ("D", name) else n)
    try:
        yield
    finally:
        del tr._d


def test_injected_backward_faults_are_caught_and_named(ctx):
    """Three wiring faults patched into the engine's backward: the stage-local check fails at the stage that owns the
    faulty gradient and nowhere else (teacher forcing confines a fault to its stage)."""
    dt, tr = ctx["dt"], _bwd_trainer(ctx)
    rec, zr, zq = ctx["grad_rec"](1, 2, 16, 16, tr.loss_scale)
    m0, m1 = "mid_block.resnets.0", "mid_block.resnets.1"
    faults = [
        ("dropped residual accum", {m0}, lambda tf: _drop_residual(tf, m0)),
        ("cat_bwd offsets swapped", {"up_blocks.3.attentions.1", "conv_in", "conv_in_ref"}, _swap_cat_offsets),
        ("wrong derived D copy", {m1}, lambda tf: _wrong_derived_copy(tr, m1 + ".conv1.weight", m1 + ".conv2.weight")),
    ]
    for what, owners, fault in faults:
        tf, grads = _run_trainer_bwd(tr, rec, zr, zq, ctx["te"][77], fault=fault)
        rows, bad, failing = sl.compare_bwd(rec, tf, grads, dt, what)
        print(f"\ninjected {what:24s} [{dt}]: failing stages {sorted(failing)}; {bad[0] if bad else ''}")
        assert failing == owners, (what, sorted(failing), bad[:3])
        assert all(any(f"stage {o} " in m for m in bad) for o in owners)
    tf, grads = _run_trainer_bwd(tr, rec, zr, zq, ctx["te"][77])      # the patches are gone: clean again
    assert not sl.compare_bwd(rec, tf, grads, dt)[1]


def test_fullsize_unet_stage_by_stage(hip_lib):
    """One full-size pass: SD-2.1 UNet, fp16, 1-shot, 512x512 (64x64 latents), stock synthetic weights; the oracle and
    its fp16 copy run on the device (plain torch there, the checker only).  The real shapes' kernel plans are checked per
    stage and a regression is named by stage; tensor coverage comes from the tiny runs above."""
    from diffews_amd import config, weights
    from diffews_amd.unet import MyUNet2DConditionModel
    from oracle.unet import OracleUNet
    from test_fullsize_gpu import _sd      # the module-wide cache of the full-size synthetic weights
    dt = torch.float16
    ucfg = config.get("sd21_unet")
    usd = _sd("unet", dt)
    te = weights.synthetic_text_embed(ucfg).to(dt).float().cuda()
    prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        ou = OracleUNet(**sl.kw(ucfg)); ou.load_state_dict(usd); ou = ou.eval().cuda()
        g = torch.Generator().manual_seed(7)
        zr = (torch.randn(1, 8, 64, 64, generator=g) * 0.5).cuda()
        zq = (torch.randn(1, 4, 64, 64, generator=g) * 0.5).cuda()
        rec = sl.record_unet(ou, weights.unet_param_shapes(ucfg), zr, zq, te, te)
        rec.e_low(dt)
        rec.model = None
        del ou
        un = MyUNet2DConditionModel(ucfg, usd, torch_dtype=dt)
        tf = _run_unet(un, rec, zr, zq, te, "two_pass", False)
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev
    assert len(tf.out) == sum(len(st.rec) for st in rec.stages.values())
    tf.check_order()
    rows, bad = sl.compare(rec, tf, dt, "full-size unet")
    print(f"\nfull-size unet [{dt}]: " + ", ".join(f"{k} {v[0]:.2f} ({v[1]}, {v[2]})" for k, v in sorted(sl.worst_by_kind(rows).items())))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- injected faults

def _mid_faults(sd):
    """One fault of each class in the middle block -> [(class, owning stage, {key: tensor})]."""
    a = "mid_block.attentions.0.transformer_blocks.0."
    pick = lambda key, cls, sib=(): next(f for c, f in sl.faults_of(key, sd, sib) if c.split(":")[0] == cls)
    return [
        ("ablation", "mid_block.resnets.1", pick("mid_block.resnets.1.conv2.bias", "ablation")),
        ("exchange", "mid_block.attentions.0", pick(a + "attn1.to_out.0.bias", "exchange", [a + "attn2.to_out.0.bias"])),
        ("transpose", "mid_block.attentions.0", pick(a + "attn1.to_q.weight", "transpose")),
        ("geglu_halves", "mid_block.attentions.0", pick(a + "ff.net.0.proj.bias", "geglu_halves")),
        ("mirror", "mid_block.resnets.0", pick("mid_block.resnets.0.conv2.weight", "mirror")),
        ("kykx", "mid_block.resnets.0", pick("mid_block.resnets.0.conv1.weight", "kykx")),
        ("temb_slice", "mid_block.resnets.1", sl.temb_slice_faults(sd)["mid_block.resnets.1.time_emb_proj.weight"][0]),
    ]


def test_injected_faults_are_caught_and_named(ctx):
    """An engine built from a state dict with ONE fault in the middle block: the stage-local assertion fails, and fails
    at the stage that owns the tensor and nowhere else (teacher forcing confines a fault to its stage)."""
    from diffews_amd.unet import MyUNet2DConditionModel
    dt = ctx["dt"]
    rec, zr, zq = ctx["unet_rec"](1, 2, 2)
    for cls, stage, fault in _mid_faults(ctx["usd"]):
        un = MyUNet2DConditionModel(ctx["ucfg"], dict(ctx["usd"], **fault), torch_dtype=dt)
        tf = _run_unet(un, rec, zr, zq, ctx["te"][2], "two_pass", False)
        rows, bad = sl.compare(rec, tf, dt, cls)
        worst = max(r[6] for r in rows if r[1] == stage)
        print(f"\ninjected {cls:13s} [{dt}]: {stage} at {worst:8.1f} x e_low; stages beyond k: {sorted({r[1] for r in rows if not r[6] <= sl.k_of(dt, r[0])})}")
        # the engine exposes the time MLP only through the fused projection, which holds every time_emb_proj too
        also = {"time"} if cls == "temb_slice" else set()
        failing = {r[1] for r in rows if not r[6] <= sl.k_of(dt, r[0])}
        assert stage in failing and failing <= {stage} | also, (cls, bad[:3])
        assert any(f"stage {stage} " in m for m in bad)


def test_whole_output_assertion_accepts_quiet_faults(ctx):
    """The same faults on the stock synthetic weights, judged as test_model_gpu.py judges (whole-output relative L2 of
    both passes within TOL_Z0): the quiet ones pass -- the gap the stage-local tests close."""
    from diffews_amd import weights
    from diffews_amd.unet import MyUNet2DConditionModel
    from oracle.unet import OracleUNet
    dt = ctx["dt"]
    ucfg = ctx["ucfg"]
    usd = weights.synthetic_unet_state_dict(ucfg, round_to=dt)
    ou = OracleUNet(**sl.kw(ucfg)); ou.load_state_dict(usd); ou.eval()
    te = ctx["te"][2]
    g = torch.Generator().manual_seed(1)
    zr = torch.randn(2, 8, 16, 16, generator=g) * 0.5
    zq = torch.randn(1, 4, 16, 16, generator=g) * 0.5
    with torch.no_grad():
        ou.clear_attn_bank()
        ref_r = ou(zr, 1, te.repeat(2, 1, 1), is_target=False)
        ref_q = ou(zq, 1, te)
        ou.clear_attn_bank()
    accepted = []
    for cls, stage, fault in _mid_faults(usd):
        un = MyUNet2DConditionModel(ucfg, dict(usd, **fault), torch_dtype=dt)
        un.clear_attn_bank()
        out_r = un(zr.cuda(), 1, te.repeat(2, 1, 1).cuda(), is_target=False).sample
        out_q = un(zq.cuda(), 1, te.cuda()).sample
        un.clear_attn_bank()
        e = max(sl.rel_images(out_r.flatten()[None], ref_r.flatten()[None])[0], sl.rel_images(out_q.flatten()[None], ref_q.flatten()[None])[0])
        print(f"\nwhole-output, faulty engine, {cls:13s} [{dt}]: {e:.3e} (tolerance {TOL_Z0[dt]:.0e})")
        if e < TOL_Z0[dt]:
            accepted.append(cls)
    assert "ablation" in accepted, accepted     # mid_block.resnets.1.conv2.bias never added: invisible to the old check
