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


class Stage:
    """One oracle stage: `name` (module path, or a composite's prefix + tag), `kind` (the stage class), the state-dict
    keys it owns, and per pass the recorded (args, kwargs, output)."""

    def __init__(self, name, kind, owned, prefix=""):
        self.name, self.kind, self.owned, self.prefix = name, kind, owned, prefix
        self.rec = {}

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


_KINDS = ((ob.ResnetBlock2D, "resnet"), (ob.Transformer2DModel, "transformer"), (ob.Downsample2D, "down"),
          (ob.Upsample2D, "up"))
_STEMS = ("conv_in", "conv_in_ref", "encoder.conv_in", "decoder.conv_in", "quant_conv", "post_quant_conv")


class Recording:
    """The oracle's stages (in definition order), the call order per pass, and e_low per (stage, pass)."""

    def __init__(self, model, keys):
        self.model, self.stages, self.order, self._pass, self._low = model, OrderedDict(), {}, None, {}
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
        y = orig(*head, self._forced(name, x), *a, **k)
        self._record(name, y)
        return y

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


def worst_by_kind(rows, into=None):
    into = {} if into is None else into
    for kind, name, p, i, e, l, r in rows:
        if r > into.get(kind, (0.0,))[0]:
            into[kind] = (r, name, p, i)
    return into
