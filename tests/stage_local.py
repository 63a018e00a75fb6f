"""Stage-local parity: helper shared by test_stage_local_cpu.py and test_stage_local_gpu.py (no tests here).

A whole-output relative L2 on quiet synthetic weights cannot see most single-parameter wiring mistakes (a bias never added,
norm1 read where norm2 belongs): the residual stream dilutes them below the model tolerance.  Here every STAGE of the oracle
(ResnetBlock2D, Transformer2DModel, Downsample2D, Upsample2D, the VAE's mid attention, the stem convs, the time embedding,
conv_norm_out + conv_out, quant_conv / post_quant_conv) is compared on its own:

  * the oracle runs once with forward hooks that keep each stage's input and output, per pass;
  * the engine runs TEACHER-FORCED: each stage callable receives the oracle's recorded input for that stage instead of the
    engine's own upstream value, and its output is recorded;
  * the yardstick of a stage is e_low: the same oracle stage cast to the storage dtype and run by torch on the same recorded
    input, against the recorded fp32 output -- what the reference's own arithmetic loses at that precision;
  * everything is compared by relative L2 per stage AND per image of the batch.

The engine must stay within K * e_low; the CPU test shows that every single-tensor fault moves its stage by at least
(2 K + 1) * e_low, so a faulty engine is at least (K + 1) * e_low from the oracle and fails.

The trainer's backward is pinned the same way.  record_unet_grads keeps, per stage and pass of the oracle's two-pass
training graph, dy (the total gradient at the stage's output), dx (what this stage alone sends to its input) and every
parameter's gradient; TeacherForce on a UNetTrainer then registers extra tape entries around each stage: the gradient
that ARRIVED at a stage output is kept and replaced by the oracle's dy, the engine's dx of the stage is kept and the
oracle's dx of this consumer is deposited upstream.  So each stage's backward is judged alone (dx and parameter
gradients against K_BWD * e_low_bwd, the oracle stage under torch autograd in the storage dtype) and the wiring
between stages is judged by `arrived`, which must be the sum of the deposited terms to one rounding per add.
Known limit: the forced input is a fresh tensor, so `tape.take` across a stage boundary (the dx_add fusion of a
stage's first norm with a gradient its input already holds) is not exercised; `take` inside a stage is.
"""
import contextlib
import copy
from collections import OrderedDict

import torch
import torch.nn.functional as F

from diffews_amd import weights
from oracle import blocks as ob

# Engine allowance per stage kind: rel(engine, oracle_fp32) <= K * e_low(stage, image).  1.25 is the project's margin
# against the reference's own low-precision run (test_not_worse_than_reference_precision).  A kind listed here needed more
# because the engine rounds at other places than torch does; the value is 1.25 x the worst ratio measured on MI355X
# (table in DESIGN.md section 4).
K_DEFAULT = 1.25
K = {torch.float16: {}, torch.bfloat16: {}}


def k_of(dtype, kind):
    return K[dtype].get(kind, K_DEFAULT)


# The same for the backward: rel(engine, oracle_fp32) <= K_BWD * e_low_bwd, per class "<stage kind>.dx" (a stage's data
# gradient, per image) and "<stage kind>.grad" (a parameter gradient of a tensor the stage owns, per tensor).
# attn1's to_q / to_k weight gradients are a class of their own, "attn1_qk.grad": the engine's q leaves its GEMM
# pre-scaled for the exp2 softmax and rounded there, and dS is rounded once more for the dQ / dK MFMAs, where torch's
# low-precision attention backward rounds elsewhere.  Worst measured ratio 1.423 (both dtypes) -> 1.25 x 1.423.
K_BWD = {torch.float16: {"attn1_qk.grad": 1.78}, torch.bfloat16: {"attn1_qk.grad": 1.78}}
# unit roundoff of the storage dtypes: one round-to-nearest per add of the tape's gradient accumulation
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


# fp16 gradients run under a loss scale (1024, a power of two: scaling and rounding commute); bf16 needs none
LOSS_SCALE = {torch.float16: 1024.0, torch.bfloat16: 1.0}


def k_bwd(dtype, cls):
    return K_BWD[dtype].get(cls, K_DEFAULT)


def grad_class(kind, key):
    """The allowance class of a parameter gradient: the owning stage's kind, but see K_BWD."""
    return "attn1_qk.grad" if key.endswith(("attn1.to_q.weight", "attn1.to_k.weight")) else kind + ".grad"


def vae_config():
    """tiny_vae with a 512-channel last level: the SD VAE's mid-block width, the one the flash attention kernel serves."""
    from diffews_amd import config
    return dict(config.get("tiny_vae"), block_out_channels=[64, 128, 256, 512])


def kw(cfg):
    return {k: v for k, v in cfg.items() if not k.startswith("_")}


def rel_images(a, b):
    """Relative L2 per image (row of the batch) -> list of floats."""
    a, b = a.detach().float().cpu().flatten(1), b.detach().float().cpu().flatten(1)
    return ((a - b).norm(dim=1) / (b.norm(dim=1) + 1e-30)).tolist()


def is_norm(name):
    return ".norm" in name or name.startswith("norm") or "group_norm" in name or "conv_norm_out" in name


def loud_state_dict(shapes, seed, bias_sigma=0.5, norm_sigma=0.3, round_to=None):
    """weights._synthetic's layout and draws, with biases at N(0, bias_sigma^2) and norm parameters at 1 +- norm_sigma /
    +- norm_sigma instead of 0.02 and 0.1: the same normal deviates (the generator is consumed identically), rescaled.
    conv_in_ref keeps the surgery relation of synthetic_unet_state_dict."""
    base = weights._synthetic(shapes, seed, None)
    sd = OrderedDict()
    for name, t in base.items():
        leaf = name.rsplit(".", 1)[-1]
        if is_norm(name):
            t = (t - 1.0) * (norm_sigma / 0.1) + 1.0 if leaf == "weight" else t * (norm_sigma / 0.1)
        elif leaf == "bias":
            t = t * (bias_sigma / 0.02)
        sd[name] = t
    if "conv_in_ref.weight" in sd and sd["conv_in_ref.weight"].shape[1] == 2 * sd["conv_in.weight"].shape[1]:
        sd["conv_in_ref.weight"] = sd["conv_in.weight"].repeat(1, 2, 1, 1) / 2
        sd["conv_in_ref.bias"] = sd["conv_in.bias"].clone()
    if round_to is not None:
        sd = OrderedDict((k, v.to(round_to).float()) for k, v in sd.items())
    return sd


# ---------------------------------------------------------------------------------------------- oracle side

def _cast(t, dtype):
    return t.to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t


class _ConvFp16(torch.autograd.Function):
    """conv2d whose backward is computed by torch's fp32 kernels on the fp16 operands and rounded to fp16 once per
    element: fp16 storage with fp32 accumulation, the arithmetic an fp16 conv backward has anyway.  torch's own fp16
    conv backward on the CPU takes a slow path (0.2 s per layer at these shapes, 60 x the bf16 one); the forward is
    torch's fp16 kernel as before."""

    @staticmethod
    def forward(ctx, conv, x, w, b, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.geom, ctx.bias = (stride, padding), b is not None
        return conv(x, w, b, stride, padding)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        stride, padding = ctx.geom
        g32 = g.float()
        gx = torch.nn.grad.conv2d_input(x.shape, w.float(), g32, stride, padding).to(x.dtype) if ctx.needs_input_grad[1] else None
        gw = torch.nn.grad.conv2d_weight(x.float(), w.shape, g32, stride, padding).to(w.dtype) if ctx.needs_input_grad[2] else None
        gb = g32.sum((0, 2, 3)).to(g.dtype) if ctx.bias and ctx.needs_input_grad[3] else None
        return None, gx, gw, gb, None, None


@contextlib.contextmanager
def _fp16_conv_backward(dtype):
    if dtype != torch.float16:
        yield
        return
    conv = F.conv2d

    def conv2d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        if x.dtype != torch.float16 or x.is_cuda or not torch.is_grad_enabled():
            return conv(x, w, b, stride, padding, dilation, groups)
        assert groups == 1 and dilation in (1, (1, 1))
        return _ConvFp16.apply(conv, x, w, b, stride, padding)
    F.conv2d = conv2d
    try:
        yield
    finally:
        F.conv2d = conv


class Stage:
    """One oracle stage: `name` (module path, or a composite's prefix + tag), `kind` (the stage class), the state-dict
    keys it owns, and per pass the recorded (args, kwargs, output)."""

    def __init__(self, name, kind, owned, prefix=""):
        self.name, self.kind, self.owned, self.prefix = name, kind, owned, prefix
        self.rec = {}
        self.grad = {}      # pass -> {"dy": ..., "dx": ...} (gradient recordings only)

    def _call(self, model, args, kwargs):
        if self.kind == "head":
            sub = model.get_submodule(self.prefix[:-1]) if self.prefix else model
            return sub.conv_out(F.silu(sub.conv_norm_out(*args)))
        if self.kind == "time":
            (t,) = args
            cfg = model.cfg
            dt = next(model.parameters()).dtype
            e = ob.timestep_embedding(t, cfg["block_out_channels"][0], cfg["flip_sin_to_cos"], cfg["freq_shift"])
            emb = model.time_embedding(e.to(dt))
            self._emb = emb
            res = [m for m in model.modules() if isinstance(m, ob.ResnetBlock2D)]
            return torch.cat([r.time_emb_proj(F.silu(emb)) for r in res], 1)
        return model.get_submodule(self.name)(*args, **kwargs)

    def run(self, model, pas, dtype=torch.float32):
        """Re-run the stage of `model` on the recorded input of pass `pas`, cast to `dtype`.  A transformer stage of the
        query pass reads a bank: it is filled by the same module's own call on the recorded support-pass input."""
        c = lambda rec: ([_cast(t, dtype) for t in rec[0]], {k: _cast(v, dtype) for k, v in rec[1].items()})
        with torch.no_grad():
            if self.kind != "transformer":
                a, k = c(self.rec[pas])
                return self._call(model, a, k)
            m = model.get_submodule(self.name)
            banked = [b.attn1 for b in m.transformer_blocks]
            for at in banked:
                at.clear_bank()
            if pas == "query":
                a, k = c(self.rec["support"])
                m(*a, **k)
            a, k = c(self.rec[pas])
            out = m(*a, **k)
            for at in banked:
                at.clear_bank()
            return out


    def grad_run(self, model, dtype=torch.float32, scale=1.0, bank=True, flip_query=False):
        """The stage of `model` under torch autograd on the recorded input and the recorded dy (times `scale`), both
        cast to `dtype` -> ({pass: dx}, {owned key: gradient}), fp32 and divided by `scale` again; parameter gradients
        are summed over the passes, as one training step sums them.  A transformer runs its support call and its query
        call on one graph, so the support rows' dx holds what the query pass sends back through the bank.
        bank=False: the support call alone (the support rows' dx without the bank term); flip_query: the query rows
        (inputs and dy) in reverse order, so every bank is read by another episode's query."""
        c = lambda rec: ([_cast(t, dtype) for t in rec[0]], {k: _cast(v, dtype) for k, v in rec[1].items()})
        named = dict(model.named_parameters())
        ps = [named[k] for k in self.owned]
        flip = lambda t, p: t.flip(0) if (flip_query and p == "query" and torch.is_tensor(t)) else t
        dys = lambda p: flip((self.grad[p]["dy"] * scale).to(dtype), p)
        has_dx = self.kind not in ("stem", "time")
        dx, pg = {}, {k: 0.0 for k in self.owned}

        def back(outs, xs, gs, passes):
            g = torch.autograd.grad(outs, xs + ps, gs, allow_unused=True)
            for p, v in zip(passes, g[:len(xs)]):
                dx[p] = flip(v.detach().float() / scale, p)
            for k, prm, v in zip(self.owned, ps, g[len(xs):]):
                pg[k] = pg[k] + (torch.zeros_like(prm, dtype=torch.float32) if v is None else v.detach().float() / scale)

        def call(p):
            a, k = c(self.rec[p])
            a = [flip(t, p) for t in a]
            if has_dx:
                a[0] = a[0].detach().requires_grad_()
            return a, k

        with torch.enable_grad(), _fp16_conv_backward(dtype):
            if self.kind == "time":
                a, k = call(next(iter(self.rec)))
                total = sum((self.grad[p]["dy"] for p in self.rec))
                back([self._call(model, a, k)], [], [(total * scale).to(dtype)], [])
            elif self.kind == "transformer":
                m = model.get_submodule(self.name)
                banked = [b.attn1 for b in m.transformer_blocks]
                for at in banked:
                    at.clear_bank()
                outs, xs, gs, passes = [], [], [], []
                for p in [q for q in ("support", "query") if q in self.rec]:
                    a, k = call(p)
                    outs.append(m(*a, **k)); xs.append(a[0]); gs.append(dys(p)); passes.append(p)
                    if not bank:
                        break
                back(outs, xs, gs, passes)
                for at in banked:
                    at.clear_bank()
            else:
                for p in self.rec:
                    a, k = call(p)
                    back([self._call(model, a, k)], [a[0]] if has_dx else [], [dys(p)], [p] if has_dx else [])
        return dx, pg


_KINDS = ((ob.ResnetBlock2D, "resnet"), (ob.Transformer2DModel, "transformer"), (ob.Downsample2D, "down"),
          (ob.Upsample2D, "up"))
_STEMS = ("conv_in", "conv_in_ref", "encoder.conv_in", "decoder.conv_in", "quant_conv", "post_quant_conv")


class Recording:
    """The oracle's stages (in definition order), the call order per pass, and e_low per (stage, pass)."""

    def __init__(self, model, keys, grads=False):
        self.model, self.stages, self.order, self._pass, self._low = model, OrderedDict(), {}, None, {}
        self.grads, self.pgrad, self._tp, self._low_bwd = grads, None, {}, {}
        keys = list(keys)
        own = lambda p: [k for k in keys if k.startswith(p)]
        mods = dict(model.named_modules())
        for n, m in mods.items():
            kind = next((k for c, k in _KINDS if isinstance(m, c)), None)
            if kind is None and isinstance(m, ob.Attention) and ".mid_block.attentions." in n and n.split(".")[0] in ("encoder", "decoder"):
                kind = "vae_attn"
            if kind is None and n in _STEMS:
                kind = "stem"
            if kind is not None:
                self.stages[n] = Stage(n, kind, own(n + "."))
        for pre in ("", "encoder.", "decoder."):
            if pre + "conv_norm_out" in mods:
                self.stages[pre + "head"] = Stage(pre + "head", "head", own(pre + "conv_norm_out.") + own(pre + "conv_out."), pre)
        if "time_embedding" in mods:
            self.stages["time"] = Stage("time", "time", own("time_embedding."))
        self._hooks = []
        if grads:       # registered before the forward hooks: the recorded input is the view whose gradient is the stage's dx
            for n, st in self.stages.items():
                if st.kind != "time":
                    m = mods[st.prefix + "conv_norm_out"] if st.kind == "head" else mods[n]
                    self._hooks.append(m.register_forward_pre_hook(lambda mod, a, k, st=st: self._pre(st, a, k), with_kwargs=True))
            for i, r in enumerate(m for m in model.modules() if isinstance(m, ob.ResnetBlock2D)):
                self._hooks.append(r.time_emb_proj.register_forward_hook(lambda mod, a, o, i=i: self._tproj(i, o)))
        for n, st in self.stages.items():
            if st.kind == "head":
                self._hooks.append(mods[st.prefix + "conv_norm_out"].register_forward_hook(
                    lambda mod, a, k, o, st=st: self._enter(st, a, k), with_kwargs=True))
                self._hooks.append(mods[st.prefix + "conv_out"].register_forward_hook(
                    lambda mod, a, k, o, st=st: self._leave(st, o), with_kwargs=True))
            elif st.kind != "time":
                self._hooks.append(mods[n].register_forward_hook(
                    lambda mod, a, k, o, st=st: self._enter(st, a, k) or self._leave(st, o), with_kwargs=True))

    def _enter(self, st, a, k):
        st.rec[self._pass] = [tuple(t.detach().clone() if torch.is_tensor(t) else t for t in a),
                              {kk: v.detach().clone() if torch.is_tensor(v) else v for kk, v in k.items()}, None]
        self.order[self._pass].append(st.name)

    def _leave(self, st, o):
        st.rec[self._pass][2] = o.detach().clone()
        if self.grads and o.requires_grad:
            o.register_hook(lambda g, d=st.grad.setdefault(self._pass, {}): d.__setitem__("dy", g.detach().clone()))

    def _pre(self, st, a, k):
        """The stage receives a fresh view of its input: the gradient of that view is what this stage alone sends to its
        input, whoever else reads the same tensor."""
        x = a[0]
        if self._pass is None or not (torch.is_tensor(x) and x.requires_grad):
            return None
        v = x.view_as(x)
        v.register_hook(lambda g, d=st.grad.setdefault(self._pass, {}): d.__setitem__("dx", g.detach().clone()))
        return (v,) + tuple(a[1:]), k

    def _tproj(self, i, o):
        if self._pass is not None and o.requires_grad:
            o.register_hook(lambda g, key=(self._pass, i): self._tp.__setitem__(key, g.detach().sum(0, keepdim=True)))

    def finish_grads(self):
        """After loss.backward(): parameter gradients, exact zeros where autograd gave none (support-pass stages the loss
        reaches only through the banks, or not at all), the time stage's dy, and who consumes whose output."""
        self.pgrad = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone())
                      for k, p in self.model.named_parameters()}
        widths = [m.time_emb_proj.out_features for m in self.model.modules() if isinstance(m, ob.ResnetBlock2D)]
        for st in self.stages.values():
            for p, r in st.rec.items():
                d = st.grad.setdefault(p, {})
                if st.kind == "time":       # dy of the fused projection: every resnet's slice, summed over the pass' rows
                    d["dy"] = torch.cat([self._tp.get((p, i), torch.zeros(1, c)) for i, c in enumerate(widths)], 1)
                    continue
                d.setdefault("dy", torch.zeros_like(r[2]))
                if st.kind != "stem":
                    d.setdefault("dx", torch.zeros_like(r[0][0]))
        self.consumers = {}
        for p, order in self.order.items():
            for cn in order:
                cs = self.stages[cn]
                if cs.kind == "stem":
                    continue
                X, lo = cs.rec[p][0][0], 0
                while lo < X.shape[1]:
                    hit = [n for n in order if n != cn and self.stages[n].rec[p][2].shape[2:] == X.shape[2:]
                           and lo + self.stages[n].rec[p][2].shape[1] <= X.shape[1]
                           and torch.equal(self.stages[n].rec[p][2], X[:, lo:lo + self.stages[n].rec[p][2].shape[1]])]
                    assert len(hit) == 1, (cn, p, lo, hit)
                    hi = lo + self.stages[hit[0]].rec[p][2].shape[1]
                    self.consumers.setdefault((hit[0], p), []).append((cn, lo, hi))
                    lo = hi

    @contextlib.contextmanager
    def recording(self, pas, timestep=None):
        """Everything the oracle runs inside is recorded as pass `pas`.  Module hooks fire when a module RETURNS, so the
        recorded order is the order of completion -- which equals the call order for stages that do not nest."""
        self._pass = pas
        self.order[pas] = []
        try:
            yield self
        finally:
            self._pass = None
        if timestep is not None and "time" in self.stages:
            st = self.stages["time"]
            t = torch.tensor([float(timestep)], device=next(self.model.parameters()).device)
            st.rec[pas] = [(t,), {}, None]
            st.rec[pas][2] = st.run(self.model, pas)
            st.emb = st._emb.detach().clone()

    def close(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []

    def owner(self):
        """state-dict key -> list of owning stage names (the CPU test asserts each list has exactly one entry)."""
        out = {}
        for st in self.stages.values():
            for k in st.owned:
                out.setdefault(k, []).append(st.name)
        return out

    def e_low_bwd(self, dtype, scale=1.0):
        """({(stage, pass): [rel of dx per image, None where the fp32 dx of the image is exactly zero]}, {key: rel of the
        parameter gradient}) of the oracle cast to `dtype` under torch autograd on the recorded input and dy, against the
        fp32 recording.  scale: the loss scale the engine runs with (a power of two): dy is scaled before it is rounded
        and the gradients are unscaled in fp32, which is what a GradScaler does -- without it fp16 would lose the small
        dy to subnormals and the yardstick would be wider than the reference's own run."""
        if (dtype, scale) not in self._low_bwd:
            low = copy.deepcopy(self.model).to(dtype)
            ex, ep = {}, {}
            for n, st in self.stages.items():
                dx, pg = st.grad_run(low, dtype, scale)
                for p, v in dx.items():
                    ref = st.grad[p]["dx"]
                    ex[(n, p)] = [None if float(ref[i].abs().max()) == 0.0 else e for i, e in enumerate(rel_images(v, ref))]
                for k, v in pg.items():
                    ep[k] = None if float(self.pgrad[k].abs().max()) == 0.0 else rel_images(v[None], self.pgrad[k][None])[0]
            self._low_bwd[(dtype, scale)] = (ex, ep)
        return self._low_bwd[(dtype, scale)]

    def e_low(self, dtype):
        """{(stage, pass): [rel per image]} of the oracle cast to `dtype` against the recorded fp32 outputs."""
        if dtype not in self._low:
            low = copy.deepcopy(self.model).to(dtype)
            self._low[dtype] = {(n, p): rel_images(st.run(low, p, dtype), st.rec[p][2])
                                for n, st in self.stages.items() for p in st.rec}
        return self._low[dtype]


def record_unet(ou, sd_keys, zr, zq, ehs_r, ehs_q, timestep=1):
    rec = Recording(ou, sd_keys)
    with torch.no_grad():
        ou.clear_attn_bank()
        with rec.recording("support", timestep):
            ou(zr, timestep, ehs_r, is_target=False)
        with rec.recording("query", timestep):
            ou(zq, timestep, ehs_q)
        ou.clear_attn_bank()
    rec.close()
    return rec


def record_unet_grads(ou, sd_keys, zr, zq, ehs_r, ehs_q, target, timestep=1):
    """record_unet plus the gradients of the oracle's two-pass training graph: the support pass keeps its graph and
    fills the banks, the query pass reads them, loss = MSE(pred, target), fp32 autograd.  Every stage of every pass gets
    grad[pass] = {dy: total gradient at its output, dx: what this stage alone sends to its input}; rec.pgrad holds
    every parameter's gradient and rec.consumers who reads each stage's output (and which channels of its input)."""
    rec = Recording(ou, sd_keys, grads=True)
    ou.zero_grad()
    ou.clear_attn_bank()
    with torch.enable_grad():
        with rec.recording("support", timestep):
            ou(zr, timestep, ehs_r, is_target=False)
        with rec.recording("query", timestep):
            pred = ou(zq, timestep, ehs_q)
        rec.loss = F.mse_loss(pred.float(), target.float())
        rec.loss.backward()
    ou.clear_attn_bank()
    rec.finish_grads()
    rec.close()
    ou.zero_grad()
    rec.loss = float(rec.loss.detach())
    return rec


def record_vae(ov, sd_keys, x, z=None):
    """encode pass: quant_conv(encoder(x)); decode pass: decoder(post_quant_conv(z)), z = the latent mean by default."""
    rec = Recording(ov, sd_keys)
    with torch.no_grad():
        with rec.recording("encode"):
            mom = ov.quant_conv(ov.encoder(x))
        with rec.recording("decode"):
            ov.decode(mom[:, :ov.cfg["latent_channels"]] if z is None else z)
    rec.close()
    return rec


# ---------------------------------------------------------------------------------------------- single-tensor faults

# Exchanges that leave the stage's function unchanged, so no test can (or needs to) see them: both biases of a pair are
# added to the same sum.  ResnetBlock2D: h = conv1(.) + conv1.bias + time_emb_proj(.) + time_emb_proj.bias, and
# out = conv_shortcut(x) + conv_shortcut.bias + conv2(.) + conv2.bias.
NO_OP_EXCHANGES = (("conv1.bias", "time_emb_proj.bias"), ("conv2.bias", "conv_shortcut.bias"))


# Ablations no test can see: a bias on the keys of a softmax attention adds q . b to every score of a query's row, and
# softmax is invariant under a shift of the row (the VAE's mid attention is the only one with biased q/k/v).
def unobservable(cls, name):
    return cls == "ablation" and name.endswith(".mid_block.attentions.0.to_k.bias")


def _no_op(a, b):
    pa, la = a.rsplit(".", 2)[0], ".".join(a.rsplit(".", 2)[1:])
    pb, lb = b.rsplit(".", 2)[0], ".".join(b.rsplit(".", 2)[1:])
    return pa == pb and tuple(sorted((la, lb))) in NO_OP_EXCHANGES


def faults_of(name, sd, siblings):
    """[(fault class, {key: faulty tensor})] for one tensor.  siblings: the other keys of the owning stage."""
    t = sd[name]
    leaf = name.rsplit(".", 1)[-1]
    out = []
    if leaf == "weight" and is_norm(name):
        out.append(("ablation", {name: torch.ones_like(t)}))
    else:
        out.append(("ablation", {name: torch.zeros_like(t)}))
    if (t.dim() == 2 or (t.dim() == 4 and t.shape[-1] == 1)) and t.shape[0] == t.shape[1]:
        out.append(("transpose", {name: t.transpose(0, 1).contiguous()}))
    if t.dim() == 4 and t.shape[-1] == 3:
        out.append(("mirror", {name: t.flip(-1, -2).contiguous()}))
        out.append(("kykx", {name: t.transpose(-1, -2).contiguous()}))
    if ".ff.net.0.proj." in name:
        h = t.shape[0] // 2
        out.append(("geglu_halves", {name: torch.cat([t[h:], t[:h]], 0)}))
    for q in siblings:
        if q > name and sd[q].shape == t.shape and not _no_op(name, q):
            out.append(("exchange:" + q, {name: sd[q].clone(), q: t.clone()}))
    return out


def temb_slice_faults(sd):
    """What a wrong `temb_slice` into the fused time projection does: a resnet reads the rows one slot further or one slot
    back in the concatenation of all time_emb_proj layers (weight and bias together).  -> {weight key: [fault dict]}"""
    names = [k[:-len("weight")] for k in sd if k.endswith("time_emb_proj.weight")]
    W = torch.cat([sd[p + "weight"] for p in names], 0)
    B = torch.cat([sd[p + "bias"] for p in names], 0)
    out, off = {}, 0
    for p in names:
        c = sd[p + "weight"].shape[0]
        out[p + "weight"] = [{p + "weight": W[o:o + c].clone(), p + "bias": B[o:o + c].clone()}
                             for o in (off - c, off + c) if o >= 0 and o + c <= W.shape[0]]
        off += c
    return out


@contextlib.contextmanager
def faulted(model, fault):
    """Apply {key: tensor} to the module's parameters in place, restore on exit."""
    params = dict(model.named_parameters())
    old = {k: params[k].data.clone() for k in fault}
    try:
        for k, v in fault.items():
            params[k].data.copy_(v)
        yield
    finally:
        for k, v in old.items():
            params[k].data.copy_(v)


def fault_effect(rec, stage, fault, elow, enough=float("inf")):
    """f: the change of the stage's output under the fault, as a multiple of e_low -- the largest over the stage's passes
    and images (a faulty engine fails as soon as one image of one pass is out of bounds).  Later passes are evaluated only
    while f < enough, so the result is a lower bound of that maximum."""
    st = rec.stages[stage]
    f = 0.0
    with faulted(rec.model, fault):
        for p in st.rec:
            eff = rel_images(st.run(rec.model, p), st.rec[p][2])
            f = max(f, max(e / l for e, l in zip(eff, elow[(stage, p)])))
            if f >= enough:
                break
    return f


# ---------------------------------------------------------------------------------------------- engine side

def _nhwc(t, like):
    return t.permute(0, 2, 3, 1).contiguous().to(device=like.device, dtype=like.dtype)


def _nchw(t):
    return t.detach().float().permute(0, 3, 1, 2).contiguous().cpu()


class TeacherForce:
    """Context manager: while active, every stage of the engine (MyUNet2DConditionModel, AutoencoderKL or UNetTrainer)
    receives the oracle's recorded input for that stage and has its output recorded.

    passes: the oracle passes the engine's batch maps to, in batch order -- ("support",) then ("query",) for the two-pass
    form (set with `at`), ("support", "query") for forward_pair / the trainer's lock-step batch, ("encode",) / ("decode",).
    Stage identity comes from the engine's own tables (_resnets_with_prefix, _transformers, the trainer's prefixes) or from
    the weight a stage-less call was given, never from the position of the call."""

    def __init__(self, rec, engine):
        self.rec, self.engine = rec, engine
        self.out, self.order, self.passes = {}, [], ()
        self._ids, self._ptr, self._patches = {}, {}, []
        # backward (UNetTrainer on a gradient recording): the engine's dx per stage, the gradient that arrived at each stage
        # output before it was replaced, both NCHW fp32 with the loss scale divided out, per (stage, pass)
        self.bwd = bool(getattr(rec, "grads", False)) and hasattr(engine, "P") and not hasattr(engine, "_resnets_with_prefix")
        self.scale = float(getattr(engine, "loss_scale", 1.0))
        self.dx, self.arrived, self.forced_in = {}, {}, {}

    def at(self, *passes):
        self.passes = passes
        return self

    # ---- bookkeeping
    def _passes(self, st):
        ps = [p for p in self.passes if p in st.rec]
        assert ps, f"engine ran stage {st.name} in pass {self.passes}, where the oracle never ran it"
        return ps

    def _forced(self, name, like, nhwc=True):
        st = self.rec.stages[name]
        x = torch.cat([st.rec[p][0][0] for p in self._passes(st)], 0)
        if nhwc:      # the oracle's NCHW fp32 -> the engine's NHWC storage dtype (fp32 in the fp32-stream mode)
            x = x.permute(0, 2, 3, 1)
        assert tuple(x.shape) == tuple(like.shape), (name, self.passes, tuple(x.shape), tuple(like.shape))
        return x.contiguous().to(device=like.device, dtype=like.dtype)

    def _record(self, name, y, nhwc=True):
        st = self.rec.stages[name]
        y = _nchw(y) if nhwc else y.detach().float().cpu()
        row = 0
        for p in self._passes(st):
            n = st.rec[p][2].shape[0]
            assert (name, p) not in self.out, f"stage {name} ran twice in pass {p}"
            self.out[(name, p)] = y[row:row + n]
            row += n
        assert row == y.shape[0], (name, self.passes, row, y.shape)
        if st.kind != "time":
            self.order.append((name, tuple(self._passes(st))))

    def check_order(self):
        """The engine's stage sequence equals the oracle's, pass by pass: no stage skipped, doubled or mismatched."""
        for p, want in self.rec.order.items():
            got = [n for n, ps in self.order if p in ps]
            if got:
                assert got == want, f"pass {p}: engine stage order differs from the oracle's at " \
                    f"{next((i, a, b) for i, (a, b) in enumerate(zip(got + [None], want + [None])) if a != b)}"

    # ---- patching
    def _patch(self, obj, attr, make):
        orig = getattr(obj, attr)
        had = attr in vars(obj)
        setattr(obj, attr, make(orig))
        self._patches.append((obj, attr, orig, had))

    def __enter__(self):
        from diffews_amd import ops, unet as U, vae as V
        e, tf = self.engine, self
        block = lambda orig: (lambda s, x, *a, **k: tf._block(orig, s, x, a, k))
        if hasattr(e, "_resnets_with_prefix"):                     # MyUNet2DConditionModel
            for r, p in e._resnets_with_prefix():
                self._ids[id(r)] = p[:-1]
            tp = [f"down_blocks.{i}.attentions.{j}" for i, b in enumerate(e.down) for j, _ in enumerate(b["attn"] or [])]
            tp += [f"up_blocks.{i}.attentions.{j}" for i, b in enumerate(e.up) for j, _ in enumerate(b["attn"] or [])]
            for t, p in zip(e._transformers(), tp + ["mid_block.attentions.0"]):
                self._ids[id(t)] = p
            self._patch(U._Resnet, "__call__", block)
            self._patch(U._Transformer, "__call__", block)
            for i, b in enumerate(e.down):
                if b["down"] is not None:
                    self._ptr[b["down"].w.data_ptr()] = f"down_blocks.{i}.downsamplers.0"
            for i, b in enumerate(e.up):
                if b["up"] is not None:
                    self._ptr[b["up"].w.data_ptr()] = f"up_blocks.{i}.upsamplers.0"
            self._ptr.update({e.w_in.data_ptr(): "conv_in", e.w_in_ref.data_ptr(): "conv_in_ref",
                              e.gn_out[0].data_ptr(): "head", e.conv_out.w.data_ptr(): "head", e.tp_w.data_ptr(): "time"})
        elif hasattr(e, "encoder"):                                # AutoencoderKL
            for side, pre in ((e.encoder, "encoder."), (e.decoder, "decoder.")):
                lvl = "down_blocks" if pre == "encoder." else "up_blocks"
                smp = "downsamplers" if pre == "encoder." else "upsamplers"
                for i, (res, s) in enumerate(side.blocks):
                    for j, r in enumerate(res):
                        self._ids[id(r)] = f"{pre}{lvl}.{i}.resnets.{j}"
                    if s is not None:
                        self._ptr[s.w.data_ptr()] = f"{pre}{lvl}.{i}.{smp}.0"
                self._ids[id(side.mid.r0)] = pre + "mid_block.resnets.0"
                self._ids[id(side.mid.att)] = pre + "mid_block.attentions.0"
                self._ids[id(side.mid.r1)] = pre + "mid_block.resnets.1"
                self._ptr.update({side.w_in.data_ptr(): pre + "conv_in", side.gn_out[0].data_ptr(): pre + "head",
                                  side.conv_out.w.data_ptr(): pre + "head"})
            self._ptr.update({e.quant_conv.w.data_ptr(): "quant_conv", e.post_quant_conv.w.data_ptr(): "post_quant_conv"})
            self._patch(V._VaeResnet, "__call__", block)
            self._patch(V._VaeAttention, "__call__", block)
        else:                                                      # UNetTrainer: stages are methods keyed by prefix
            P = e.P
            self._patch(e, "_resnet", lambda orig: (lambda tape, p, x, *a, **k: tf._named(orig, p[:-1], (tape, p), x, a, k)))
            self._patch(e, "_transformer", lambda orig: (lambda tape, p, x, *a, **k: tf._named(orig, p[:-1], (tape, p), x, a, k)))
            self._patch(e, "_gn", lambda orig: (lambda tape, x, gname, *a, **k: tf._head_gn(orig, tape, x, gname, a, k)))
            smp = {n + "weight": n[:-len(".conv.")] for n in e.samplers}
            self._patch(e, "_conv", lambda orig: (lambda tape, x, wname, *a, **k: tf._named(orig, smp[wname], (tape,), x, (wname,) + a, k)
                                                  if wname in smp else orig(tape, x, wname, *a, **k)))
            self._ptr.update({P.p("conv_in.weight").data_ptr(): "conv_in", P.p("conv_in_ref.weight").data_ptr(): "conv_in_ref",
                              P.p("conv_norm_out.weight").data_ptr(): "head", P.w("conv_out.weight").data_ptr(): "head",
                              P.w("tp_w").data_ptr(): "time"})
        self._patch(ops, "conv3x3_stream", lambda orig: (lambda x, w, *a, **k: tf._sampler(orig, x, w, a, k)))
        self._patch(ops, "conv_small", lambda orig: (lambda x, w, *a, **k: tf._stem(orig, x, w, a, k)))
        self._patch(ops, "groupnorm", lambda orig: (lambda x, gamma, *a, **k: tf._head_in(orig, x, gamma, a, k)))
        self._patch(ops, "conv3x3", lambda orig: (lambda x, w, *a, **k: tf._head_out(orig, x, w, a, k)))
        self._patch(ops, "linear", lambda orig: (lambda x, w, *a, **k: tf._time(orig, x, w, a, k)))
        return self

    def __exit__(self, *exc):
        for obj, attr, orig, had in reversed(self._patches):
            if had or isinstance(obj, type) or not hasattr(type(obj), attr):
                setattr(obj, attr, orig)
            else:
                delattr(obj, attr)      # an instance attribute that shadowed a method
        self._patches = []
        return False

    # ---- the wrapped stages
    def _block(self, orig, s, x, a, k):
        name = self._ids.get(id(s))
        if name is None:
            return orig(s, x, *a, **k)
        y = orig(s, self._forced(name, x), *a, **k)
        self._record(name, y)
        return y

    def _named(self, orig, name, head, x, a, k):
        xf = self._forced(name, x)
        if self.bwd:
            tape = head[0]
            if name == self.rec.order["query"][1]:      # the first trunk stage reads the stem's output
                self._arrive(tape, [("conv_in_ref", "support"), ("conv_in", "query")], x)
            self._leave_dx(tape, name, xf, x)
        y = orig(*head, xf, *a, **k)
        self._record(name, y)
        if self.bwd:
            self._arrive(tape, [(name, p) for p in self._passes(self.rec.stages[name])], y)
        return y

    # ---- teacher-forced backward: extra tape entries around each stage (the tape walks its entries in reverse)
    def _grad(self, parts, what, like):
        """The oracle's recorded gradient of the (stage, pass) parts, rows concatenated, NHWC, times the loss scale, rounded
        to the storage dtype."""
        g = torch.cat([self.rec.stages[n].grad[p][what] for n, p in parts if p in self.passes], 0).permute(0, 2, 3, 1)
        assert tuple(g.shape) == tuple(like.shape), (parts, what, tuple(g.shape), tuple(like.shape))
        return (g * self.scale).contiguous().to(device=like.device, dtype=like.dtype)

    def _keep(self, store, parts, g):
        y, row = _nchw(g) / self.scale, 0
        for n, p in parts:
            if p in self.passes:
                rows = self.rec.stages[n].rec[p][2].shape[0]
                assert (n, p) not in store, f"stage {n}: a second gradient in pass {p}"
                store[(n, p)] = y[row:row + rows]
                row += rows
        assert row == y.shape[0], (parts, row, y.shape)

    def _arrive(self, tape, parts, y):
        """Registered AFTER the op that made y, so it runs before it: keeps the gradient that arrived at the stage's
        output (the wiring between stages) and hands the stage the oracle's dy instead."""
        def hook(g):
            self._keep(self.arrived, parts, g)
            tape.accum(y, self._grad(parts, "dy", y))
        tape.add(y, hook)

    def _leave_dx(self, tape, name, xf, x):
        """Registered BEFORE the stage's ops, on the forced input (a leaf no op produced), so it runs after all of them:
        keeps the engine's dx of this stage and deposits the oracle's dx of this consumer on the engine's own upstream
        tensor."""
        parts = [(name, p) for p in self._passes(self.rec.stages[name])]
        self.forced_in[name] = xf

        def hook(g):
            self._keep(self.dx, parts, g)
            tape.accum(x, self._grad(parts, "dx", x))
        tape.add(xf, hook)

    def _head_gn(self, orig, tape, x, gname, a, k):
        if not self.bwd or gname != "conv_norm_out.weight":
            return orig(tape, x, gname, *a, **k)
        xf = self._forced("head", x)
        self._leave_dx(tape, "head", xf, x)
        return orig(tape, xf, gname, *a, **k)

    def seed_head(self, c):
        """The oracle's dL/dpred (zero on the support rows) through ob.loss_grad into the seeds of _backward: conv_out's
        weight gradient and data gradient are computed by the engine from the same dy the oracle's head had."""
        from diffews_amd import ops_bwd
        st = self.rec.stages["head"]
        g = torch.cat([st.grad[p]["dy"] for p in self.passes], 0).float().contiguous().to(c["dpn"].device)
        ops_bwd.loss_grad(g, self.engine.dtype, scale=self.scale, dpred_out=c["dpred"], dpred_nchw_out=c["dpn"])

    def _sampler(self, orig, x, w, a, k):
        name = self._ptr.get(w.data_ptr())
        if name is None or self.rec.stages[name].kind not in ("down", "up"):
            return orig(x, w, *a, **k)
        y = orig(self._forced(name, x), w, *a, **k)
        self._record(name, y)
        return y

    def _stem(self, orig, x, w, a, k):
        name = self._ptr.get(w.data_ptr())
        if name is None or self.rec.stages[name].kind != "stem":
            return orig(x, w, *a, **k)
        if torch.is_tensor(x):      # NCHW fp32 on both sides
            x = self._forced(name, x, nhwc=False)
        y = orig(x, w, *a, **k)
        self._record(name, y, nhwc=not k.get("nchw_f32_out", False))
        return y

    def _head_in(self, orig, x, gamma, a, k):
        name = self._ptr.get(gamma.data_ptr())
        if name is None or self.rec.stages[name].kind != "head":
            return orig(x, gamma, *a, **k)
        return orig(self._forced(name, x), gamma, *a, **k)

    def _head_out(self, orig, x, w, a, k):
        name = self._ptr.get(w.data_ptr())
        y = orig(x, w, *a, **k)
        if name is not None and self.rec.stages[name].kind == "head":
            assert k.get("out_nchw_f32")
            self._record(name, y / float(k.get("out_scale", 1.0)), nhwc=False)
        return y

    def _time(self, orig, x, w, a, k):
        if self._ptr.get(w.data_ptr()) != "time":
            return orig(x, w, *a, **k)
        # the engine's own time MLP + fused projection is the "time" stage's output; the resnets then read the projection
        # of the ORACLE's embedding, made by the same GEMM on the engine's fused weight (so temb_slice stays under test)
        st = self.rec.stages["time"]
        y = orig(x, w, *a, **k)
        for p in self._passes(st):
            self.out.setdefault(("time", p), y.detach().float().cpu()[:1])
        semb = F.silu(st.emb[:1]).expand(x.shape[0], -1).contiguous().to(device=x.device, dtype=x.dtype)
        return orig(semb, w, *a, **k)


def compare(rec, tf, dtype, label=""):
    """-> (rows, failures).  rows: (kind, stage, pass, image, rel, e_low, ratio); failures: messages naming the stage
    prefix, pass, image and ratio for every (stage, image) beyond k * e_low."""
    elow = rec.e_low(dtype)
    rows, bad = [], []
    for (name, p), y in sorted(tf.out.items()):
        st = rec.stages[name]
        ref = st.rec[p][2]
        if name == "time":
            ref = ref[:1]
        for i, (e, l) in enumerate(zip(rel_images(y, ref), elow[(name, p)])):
            r = e / l
            rows.append((st.kind, name, p, i, e, l, r))
            if not r <= k_of(dtype, st.kind):
                bad.append(f"{label} stage {name} ({st.kind}), {p} pass, image {i}: rel {e:.3e} = {r:.2f} x e_low {l:.3e}"
                           f" > {k_of(dtype, st.kind):.2f}")
    return rows, bad


def arrived_ref(rec, name, p, dtype, scale=1.0, drop=None, exchange=()):
    """What the tape must have accumulated at the output of stage `name` in pass p when every consumer deposits the
    oracle's dx (times the loss scale, rounded to the storage dtype): -> (the fp64 sum of the n terms, the per-element
    bound (n - 1) * u * max |partial sum| -- one round-to-nearest per add, nothing more; the partial sums are taken in
    the tape's order, last consumer first, and in the forward order, whichever is larger).
    drop: leave out that consumer's term; exchange: consumers whose two concat halves are handed out crosswise (the
    first producer gets the last channels of dx, the second the first ones) -- the faults of the CPU proof."""
    terms = []
    for cn, lo, hi in rec.consumers[(name, p)]:
        if cn == drop:
            continue
        d = rec.stages[cn].grad[p]["dx"]
        if cn in exchange and hi - lo < d.shape[1]:
            lo, hi = (d.shape[1] - hi, d.shape[1]) if lo == 0 else (0, hi - lo)
        terms.append((d[:, lo:hi] * scale).to(dtype).double() / scale)
    zero = torch.zeros_like(rec.stages[name].rec[p][2], dtype=torch.float64)
    peak = zero.clone()
    for order in (terms[::-1], terms):
        part = zero.clone()
        for t in order:
            part = part + t
            peak = torch.maximum(peak, part.abs())
    return sum(terms, zero), max(len(terms) - 1, 0) * U[dtype] * peak


def compare_bwd(rec, tf, grads, dtype, label=""):
    """The teacher-forced backward against the gradient recording -> (rows, failures, failing stages).
    rows: (class, stage or tensor, pass, image, rel, e_low_bwd, ratio); a row of class "arrived" holds the largest
    error and the bound at that element.  Every stage's dx, every stage output's arrived gradient and every key of
    `grads` (tr.grad_dict(), loss scale already divided out by the engine) is judged exactly once; what is missing
    is a failure."""
    ex, ep = rec.e_low_bwd(dtype, tf.scale)
    owner = {k: v[0] for k, v in rec.owner().items()}
    rows, bad, failing = [], [], set()

    def fail(stage, msg):
        failing.add(stage)
        bad.append(f"{label} stage {stage} {msg}")

    def judge(cls, stage, what, p, i, got, ref, low):
        if low is None:      # the oracle's gradient is exactly zero: so is the engine's
            if float(got.abs().max()) != 0.0:
                fail(stage, f"{what}, {p} pass, image {i}: exactly zero in the oracle, max |engine| {float(got.abs().max()):.3e}")
            return
        e = rel_images(got[None], ref[None])[0]
        r = e / low
        rows.append((cls, what, p, i, e, low, r))
        if not r <= k_bwd(dtype, cls):
            fail(stage, f"{what}, {p} pass, image {i}: rel {e:.3e} = {r:.2f} x e_low_bwd {low:.3e} > {k_bwd(dtype, cls):.2f}")

    for n, st in rec.stages.items():
        for p in st.rec:
            if st.kind in ("stem", "time"):
                continue
            got = tf.dx.get((n, p))
            if got is None:
                fail(n, f"dx, {p} pass: no gradient reached the stage's input")
                continue
            for i, low in enumerate(ex[(n, p)]):
                judge(st.kind + ".dx", n, f"{n} dx", p, i, got[i], st.grad[p]["dx"][i], low)
    assert set(grads) == set(rec.pgrad), sorted(set(grads) ^ set(rec.pgrad))[:5]
    for key, ref in rec.pgrad.items():
        judge(grad_class(rec.stages[owner[key]].kind, key), owner[key], key, "both", 0, grads[key].detach().float().cpu(), ref, ep[key])
    for (n, p), cons in rec.consumers.items():
        got = tf.arrived.get((n, p))
        if got is None:
            fail(n, f"arrived, {p} pass: no gradient reached the stage's output")
            continue
        ref, bound = arrived_ref(rec, n, p, dtype, tf.scale)
        err = (got.double() - ref).abs()
        j = int((err - bound).argmax())
        e, b = float(err.flatten()[j]), float(bound.flatten()[j])
        rows.append(("arrived", n, p, len(cons), e, b, e / b if b > 0 else (0.0 if e == 0 else float("inf"))))
        if not bool((err <= bound).all()):
            fail(n, f"arrived, {p} pass: {len(cons)} consumers {[c for c, _, _ in cons]}, |arrived - sum| {e:.3e} > "
                    f"(n - 1) u max|partial| = {b:.3e}")
    return rows, bad, failing


def worst_by_kind(rows, into=None):
    into = {} if into is None else into
    for kind, name, p, i, e, l, r in rows:
        if r > into.get(kind, (0.0,))[0]:
            into[kind] = (r, name, p, i)
    return into
