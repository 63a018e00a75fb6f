"""Few-shot segmentation pipeline with the reference's interface, running on the MI355X engine.

Drop-in for `MarigoldPipelineRGBLatentNoise`
(/root/reference/diffews/marigold_pipeline_rgb_latent_noise.py:99): same constructor / `__call__`
signature (P:126-138, P:223-238), `test_timestep` attribute (evaluation_util/main_oss.py:373),
`enable_xformers_memory_efficient_attention()` (E:376, no-op), `single_infer` (P:617),
`encode_rgb` (P:839), `decode_seg` (P:887).

Differences that are deliberate:
  * the CLIP text tower on "" (P:585-601) is constant per checkpoint: pass `text_embeds`
    ([1, L, cross_attention_dim]); a `text_encoder`+`tokenizer` pair is used once if given;
  * `rgb_paths` is ignored (the reference opens each path and throws the result away, P:312-316);
  * inner batching uses the explicit `batch_size`, not the VRAM lookup table (P:397-407);
  * `run_episodes()` is the fused fast path the launcher/bench use: z0 = -v is folded into the
    UNet's conv_out epilogue and the threshold + intersection/union counts stay on device; with
    `use_graph` / `captured=True` the whole step is one HIP-graph replay owned by the pipeline.
Only the segmentation task is implemented; the reference treats every mode except 'depth' as
'seg' (`mode == 'seg' or 'semseg'` is always truthy, P:280).
"""
from dataclasses import dataclass
from typing import List, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .scheduler import DDIMSchedulerCustomized


@dataclass
class MarigoldSegOutput:
    seg_colored: Union["PIL.Image.Image", List["PIL.Image.Image"]]
    uncertainty: Union[None, np.ndarray]


def chw2hwc(chw):
    """marigold/util/image_util.py:55."""
    assert chw.ndim == 3
    return np.moveaxis(chw, 0, -1) if isinstance(chw, np.ndarray) else chw.permute(1, 2, 0)


def load_empty_text_embed(checkpoint, tokenizer=None):
    """CLIP("") of a diffusers checkpoint directory -> [1, L, cross_attention_dim] fp32 (P:585-601):
    `tokenizer("", padding="do_not_pad", max_length=model_max_length, truncation=True)` => [BOS, EOS], then
    `text_encoder(ids)[0]`.  Uses `transformers` on the host (the CLIP tower is a constant input of the
    hot path); `tokenizer` may be the launcher's own CLIPTokenizer (E:351-353)."""
    import os
    from transformers import CLIPTextModel, CLIPTokenizer
    if checkpoint is None:
        raise ValueError("need text_embeds, a text_encoder, or a checkpoint directory holding text_encoder/ and tokenizer/")
    enc_dir = os.path.join(checkpoint, "text_encoder")
    if not os.path.isdir(enc_dir):
        raise FileNotFoundError(f"{enc_dir} not found: pass text_embeds=[1, L, D] or text_encoder=")
    if tokenizer is None:
        tokenizer = CLIPTokenizer.from_pretrained(os.path.join(checkpoint, "tokenizer"))
    enc = CLIPTextModel.from_pretrained(enc_dir).float().eval()
    ids = tokenizer("", padding="do_not_pad", max_length=tokenizer.model_max_length, truncation=True,
                    return_tensors="pt").input_ids
    with torch.no_grad():
        return enc(ids)[0].float()


def _assert_no_memset_nodes(graph):
    """Invariant of the captured step: no memset node.  On ROCm 7.2 a small memset node replayed
    next to plain launches on the same stream received the following launch's kernel arguments (all-zero predictions in
    the bench metric); the library therefore zeroes its scratch words with kernels.  A torch.zeros / .zero_() / fill_ that
    slips into the step later would re-introduce such a node silently, so every capture is inspected once
    (dfw_graph_memset_nodes walks the hipGraph_t's nodes).  Returns the node count."""
    import ctypes as C
    from . import _lib as L
    n = C.c_int32(0)
    rc = L.lib().dfw_graph_memset_nodes(C.c_void_p(graph.raw_cuda_graph()), C.byref(n))
    if rc < 0:
        L.check(rc, "dfw_graph_memset_nodes")
    if rc > 0:
        raise RuntimeError(f"the captured step contains {rc} memset node(s) (torch.zeros / zero_ / fill_ inside the step?): "
                           "zero scratch with a library kernel instead, see DESIGN.md section 2")
    return n.value


class MarigoldPipelineRGBLatentNoise:
    rgb_latent_scale_factor = 0.18215   # P:120-124
    seg_latent_scale_factor = 0.18215

    def __init__(self, unet, vae, scheduler, tokenizer=None, text_embeds=None, text_encoder=None,
                 image_encoder=None, image_projector=None, controlnet=None, customized_head=None):
        if image_encoder is not None or image_projector is not None or controlnet is not None or customized_head is not None:
            raise NotImplementedError("image_encoder / image_projector / controlnet / customized_head are always "
                                      "None on the DiffewS path (evaluation_util/main_oss.py:355-364)")
        if text_embeds is None and text_encoder is None:
            raise ValueError("need text_embeds ([1, L, cross_attention_dim]) or a text_encoder + tokenizer")  # P:160-161
        self.unet, self.vae, self.scheduler = unet, vae, scheduler
        self.tokenizer, self.text_encoder = tokenizer, text_encoder
        self.empty_text_embed = text_embeds
        self.test_timestep = 1
        self.fold_conditioning = True   # run_episodes: precompute the constant conditioning once
        self.use_graph = False          # run_episodes: replay the step as one HIP graph (see run_episodes)
        self.device = unet.device
        self.dtype = unet.dtype
        self._graphs = {}

    # ------------------------------------------------------------------ reference surface
    @classmethod
    def from_pretrained(cls, checkpoint=None, unet=None, vae=None, scheduler=None, tokenizer=None, text_embeds=None,
                        text_encoder=None, controlnet=None, image_projector=None, customized_head=None,
                        image_encoder=None, torch_dtype=None, residual_dtype=None, **kw):
        from .unet import MyUNet2DConditionModel
        from .vae import AutoencoderKL
        requested = torch_dtype
        if torch_dtype == torch.float32:
            # The launcher's DEFAULT (evaluation_util/main_oss.py:332-336: `dtype = torch.float32` unless
            # --half_precision) reaches this call as torch_dtype=torch.float32 beside prebuilt unet= / vae=
            # (E:355-369).  The engine has no fp32-operand kernels; what it offers for an
            # fp32 request is its most precise mode, fp16 storage + fp32 residual stream: z0 within north_star's
            # 1e-3 of the fp32 path (7.4-7.7e-4).  Selected here, loudly, instead of
            # silently staying in whatever 16-bit dtype the engines were built with.
            import warnings
            warnings.warn("torch_dtype=torch.float32: the MI355X engine computes with 16-bit MFMA operands; running its "
                          "parity mode (fp16 storage + fp32 residual stream, z0 within 1e-3 of fp32) instead", stacklevel=2)
            torch_dtype = torch.float16
            if residual_dtype is None:
                residual_dtype = torch.float32
        dt = torch_dtype or torch.bfloat16
        if text_embeds is None and text_encoder is None:
            # evaluation_util/main_oss.py:355-369 passes text_embeds=None and no text_encoder: diffusers then
            # loads CLIPTextModel from <checkpoint>/text_encoder and P:585-601 runs it on "" in every call.
            # The prompt is a per-checkpoint constant: evaluate it ONCE here (host, fp32) and keep the result.
            text_embeds = load_empty_text_embed(checkpoint, tokenizer)
        if unet is None:
            unet = MyUNet2DConditionModel.from_pretrained(checkpoint, subfolder="unet", torch_dtype=dt, residual_dtype=residual_dtype)
        if vae is None:
            vae = AutoencoderKL.from_pretrained(checkpoint, subfolder="vae", torch_dtype=dt, residual_dtype=residual_dtype)
        if scheduler is None:
            scheduler = DDIMSchedulerCustomized.from_pretrained(checkpoint, subfolder="scheduler")
        # prebuilt engines (the launcher's call form, E:338-349) follow an EXPLICIT torch_dtype / residual_dtype: they
        # are repacked from their host state dict once (`to`), the residual-stream mode is a flag
        if requested is not None:
            unet.to(dtype=dt)
            vae.to(dtype=dt)
        pipe = cls(unet, vae, scheduler, tokenizer=tokenizer, text_embeds=text_embeds, text_encoder=text_encoder,
                   image_encoder=image_encoder, image_projector=image_projector, controlnet=controlnet,
                   customized_head=customized_head)
        if residual_dtype is not None and (unet.residual_dtype != residual_dtype or vae.residual_dtype != residual_dtype):
            pipe.set_residual_dtype(residual_dtype)
        pipe.requested_dtype = requested
        return pipe

    def to(self, device=None, dtype=None):
        self.unet.to(device, dtype)
        self.vae.to(device, dtype)
        self.device, self.dtype = self.unet.device, self.unet.dtype
        self._graphs = {}
        return self

    def enable_xformers_memory_efficient_attention(self, *a, **k):
        """E:374-376.  The UNet's KV-fusion attention is always the memory-efficient (flash) kernel; for the VAE's mid-block
        attention this call selects the flash kernel too (csrc/vae_attention.hip: no N x N score tensor), as xformers does in
        the reference.  Without the call the VAE picks per shape (vae._VaeAttention.flash = "auto")."""
        for half in (self.vae.encoder, self.vae.decoder):
            half.mid.att.flash = True
        self._graphs = {}
        return None

    @property
    def residual_dtype(self):
        return self.unet.residual_dtype

    def set_residual_dtype(self, residual_dtype=None, vae_residual_dtype="same"):
        """Storage of the residual stream of the UNet and the VAE: None = the engines' storage dtype (fastest),
        torch.float32 = fp32 stream with 16-bit MFMA operands (north_star's 1e-3 in fp16).  The
        weights are shared by both modes (only epilogue flags differ), so this is a switch, not a rebuild; captured
        graphs are dropped."""
        rd = residual_dtype or self.unet.dtype
        vd = rd if vae_residual_dtype == "same" else (vae_residual_dtype or self.vae.dtype)
        if rd not in (self.unet.dtype, torch.float32) or vd not in (self.vae.dtype, torch.float32):
            raise ValueError("residual_dtype must be None (= storage dtype) or torch.float32")
        self.unet.residual_dtype, self.unet._f32s = rd, rd == torch.float32
        self.vae.residual_dtype = vd
        self.vae.encoder.f32s = vd == torch.float32
        self.vae.decoder.f32s = vd == torch.float32 and self.vae.decoder_f32_stream    # downstream of z0: 16-bit stream by default
        self._graphs = {}
        return self

    def encode_clip_feature(self, clip_rgb_in=None):
        """P:585-601; evaluated once, the prompt is the constant ""."""
        if self.empty_text_embed is None:
            ids = self.tokenizer("", padding="do_not_pad", max_length=self.tokenizer.model_max_length,
                                 truncation=True, return_tensors="pt").input_ids
            with torch.no_grad():
                self.empty_text_embed = self.text_encoder(ids.to(self.text_encoder.device))[0]
        return self.empty_text_embed

    def encode_rgb(self, rgb_in):
        """P:839-862: mean of quant_conv(encoder(x)) times the latent scale (no sampling)."""
        h = self.vae.encoder(rgb_in.to(self.device))
        lc = self.vae.config["latent_channels"]
        return self.vae.quant_conv(h, out_scale=self.rgb_latent_scale_factor, channels=lc)

    def decode_seg(self, seg_latent):
        """P:887-905; the clip to [-1, 1] (P:903) happens in the decoder's last conv epilogue."""
        z = self.vae.post_quant_conv(seg_latent.to(self.device), in_scale=1.0 / self.seg_latent_scale_factor)
        return self.vae.decoder(z, clamp=True)

    @torch.no_grad()
    def single_infer(self, rgb_in_ref, rgb_in_tag, gt_in_ref, clip_rgb_in=None, num_inference_steps=1,
                     show_pbar=False, mode="seg", seed=None, return_latents=False):
        """P:617-802, generic scheduler path (any number of denoising steps)."""
        self.scheduler.set_timesteps(num_inference_steps, device=self.device)
        z_ref, z_tag, z_gt = self.encode_rgb(rgb_in_ref), self.encode_rgb(rgb_in_tag), self.encode_rgb(gt_in_ref)
        cond_ref = torch.cat([z_ref, z_gt], dim=1)   # P:674
        z = z_tag.clone()                            # P:675
        b = z_tag.shape[0]
        embed = self.encode_clip_feature(clip_rgb_in).to(self.device)
        ehs = embed.repeat((b, 1, 1))                # P:690
        ehs_ref = ehs.repeat((z_ref.shape[0] // b, 1, 1))  # P:692
        step_out = None
        for t in self.scheduler.timesteps:
            self.unet.clear_attn_bank()              # P:715
            self.unet(cond_ref, t * self.test_timestep, encoder_hidden_states=ehs_ref, is_target=False)  # P:719-720
            noise_pred = self.unet(z, t * self.test_timestep, encoder_hidden_states=ehs).sample          # P:721-724
            self.unet.clear_attn_bank()              # P:725
            step_out = self.scheduler.step(noise_pred, t, z)   # P:764
            z = step_out.prev_sample
        z0 = step_out.pred_original_sample           # P:769
        seg = self.decode_seg(z0)
        seg = (torch.clip(seg, -1.0, 1.0) * 0.5 + 0.5) * 255  # P:790-795
        if return_latents:
            return seg, dict(z_ref=z_ref, z_tag=z_tag, z_gt=z_gt, z0=z0)
        return seg

    def _fold_conditioning(self, tt):
        """the "" prompt embedding and the one timestep are per-checkpoint constants;
        fold them into the UNet once (time projections + all attn2 K/V) -- True when forwards can run
        with encoder_hidden_states=None.  Re-folds if test_timestep or the embedding object changed."""
        if not self.fold_conditioning or not hasattr(self.unet, "fold_conditioning"):
            return False
        if torch.is_tensor(tt) and (tt.device.type != "cpu" or tt.numel() != 1):
            return False
        embed = self.encode_clip_feature()
        key = (float(tt), id(embed), embed._version)
        if getattr(self, "_fold_key", None) != key:
            self.unet.fold_conditioning(float(tt), embed)
            self._fold_key = key
        return True

    # ------------------------------------------------------------------ fused fast path
    @torch.no_grad()
    def run_episodes(self, support_imgs, query_img, support_masks, query_gt=None, r_threshold=0.25, threshold=0.0,
                     batch_max=False, captured=None, native=None):
        """One denoising step for a batch of episodes, everything on device.

        support_imgs / support_masks [b*s, 3, H, W], query_img [b, 3, H, W] in [-1, 1];
        query_gt optional uint8 [b, H, W] (0/1, 255 = ignore).
        Returns dict(z0 [b,4,h,w] fp32, dec [b,3,H,W] fp32 in [-1,1], seg_u8 [b,3,H,W] uint8,
        counts [b,4] int64 = inter0, inter1, union0, union1 or None).
        Equivalent to single_infer(num_inference_steps=1) when the scheduler is the reference's
        degenerate DDIM (z0 = -v); falls back to it otherwise.
        r_threshold / threshold / batch_max: the launcher's thresholding flags (main_oss.py:128-135; see
        ops.seg_postprocess).

        native (input_pipeline.NativeTargets for these b queries): the dict gains `native` = ops.seg_native on seg_u8 with
        the same flags -- masks and counts at every query's own size (the launcher's --use_original_imgsize).  Launched
        on the same stream after the step; sizes vary per batch, so after a captured replay it runs eagerly and is
        neither part of the graph nor of its key.  Every other entry is what the call without `native` returns.

        captured (default: self.use_graph): replay the whole step (~750 kernel launches) as ONE HIP graph,
        captured on first use per (b, s, H, W, flags) into static buffers.  The inputs are copied into the
        graph's input buffers and the returned tensors are the graph's output buffers: they are
        overwritten by the next captured call with the same key (consume or clone them first).
        """
        sched = self.scheduler
        sched.set_timesteps(1, device=self.device)
        t = sched.timesteps[0]
        if not sched.z0_is_neg_v(t):
            seg, lat = self.single_infer(support_imgs, query_img, support_masks, return_latents=True)
            dec = (seg / 255.0 * 2.0 - 1.0).contiguous()
            seg_u8, counts = ops.seg_postprocess(dec, query_gt, r_threshold, threshold, batch_max)
            return self._with_native(dict(z0=lat["z0"], dec=dec, seg_u8=seg_u8, counts=counts), native, ops.seg_native,
                                     r_threshold, threshold, batch_max)
        tt = t * self.test_timestep
        folded = self._fold_conditioning(tt)      # host + load-time work: never inside a capture
        dev = self.device
        ins = dict(support_imgs=support_imgs.to(dev, torch.float32).contiguous(),
                   query_img=query_img.to(dev, torch.float32).contiguous(),
                   support_masks=support_masks.to(dev, torch.float32).contiguous(),
                   query_gt=None if query_gt is None else query_gt.to(dev).contiguous())
        flags = (float(r_threshold), float(threshold), bool(batch_max))

        def step(support_imgs, query_img, support_masks, query_gt=None):
            return self._episodes_step(support_imgs, query_img, support_masks, query_gt, tt, folded, flags)
        if captured is None:
            captured = self.use_graph
        if not captured:
            return self._with_native(step(**ins), native, ops.seg_native, *flags)
        key = self._graph_key((tuple(ins["support_imgs"].shape), tuple(ins["query_img"].shape), query_gt is not None, flags),
                              tt, folded)
        return self._with_native(self._replay(key, step, ins), native, ops.seg_native, *flags)

    @staticmethod
    def _with_native(r, native, op, *args, **kw):
        """r plus r["native"] = op(r["seg_u8"], native, *args, **kw) -- ops.seg_native or ops.seg_labels_native with the call's
        flags --, eagerly on the current stream (r itself may be a captured step's cached output dict: it is copied, not
        written)."""
        if native is None:
            return r
        r = dict(r)
        r["native"] = op(r["seg_u8"], native, *args, **kw)
        return r

    def _graph_key(self, head, tt, folded):
        """The key of a captured step: `head` (the route, its support's uid, shapes and flags) plus what every step depends
        on -- the timestep, the fold and both residual-stream modes."""
        return head + (float(tt), folded, getattr(self, "_fold_key", None), self.unet.residual_dtype, self.vae.residual_dtype)

    def _episodes_step(self, support_imgs, query_img, support_masks, query_gt, tt, folded, flags):
        """The kernels of one step; every buffer it touches is written by a library kernel (no torch.cat /
        slice-assign / clip passes): conv_in reads the three image groups in place, quant_conv writes the
        latent means straight into cat([rgb, mask]) (P:674) and z_tag, conv_out folds z0 = -v, the decoder's
        last conv clips to [-1, 1] (P:903)."""
        b, n_sup = query_img.shape[0], support_imgs.shape[0]
        lc = self.vae.config["latent_channels"]
        # one VAE-encoder launch train for all 2s+1 image groups (weights read once)
        mom = self.vae.encoder([support_imgs, support_masks, query_img])       # [2 n_sup + b, 2 lc, h, w] fp32
        h, w = mom.shape[-2:]
        cond_ref = torch.empty(n_sup, 2 * lc, h, w, dtype=torch.float32, device=mom.device)
        z_tag = torch.empty(b, lc, h, w, dtype=torch.float32, device=mom.device)
        qc, sf = self.vae.quant_conv, self.rgb_latent_scale_factor
        qc(mom[:n_sup], out_scale=sf, out=cond_ref[:, :lc], channels=lc)               # z_ref      (P:649)
        qc(mom[n_sup:2 * n_sup], out_scale=sf, out=cond_ref[:, lc:], channels=lc)      # z_mask_ref (P:651)
        qc(mom[2 * n_sup:], out_scale=sf, out=z_tag, channels=lc)                      # z_tag      (P:650)
        # support + query passes in layer lock-step (one trunk pass over [support ; query], weights
        # read once); z0 = -v folded into conv_out.  Same per-image arithmetic as P:715-725.
        if folded:
            z0 = self.unet.forward_pair(cond_ref, z_tag, tt, out_scale=-1.0)
        else:
            embed = self.encode_clip_feature().to(self.device)
            ehs = embed.repeat((b, 1, 1))
            ehs_ref = ehs.repeat((n_sup // b, 1, 1))
            z0 = self.unet.forward_pair(cond_ref, z_tag, tt, ehs_ref, ehs, out_scale=-1.0)
        dec = self.decode_seg(z0)
        seg_u8, counts = ops.seg_postprocess(dec, query_gt, *flags)
        return dict(z0=z0, dec=dec, seg_u8=seg_u8, counts=counts)

    # ------------------------------------------------------------------ shared support bank
    # prepare_support / prepare_support_classes turn support images into a SupportBank / SupportBankSet (diffews_amd.unet);
    # segment_queries, segment_classes, segment_routed and segment_candidates(_native) run query images against one.  The
    # five routes are one scaffold around a `step` closure -- _query_context (every check, on the host, before anything is
    # launched or replayed), the step (_query_latents, a unet.forward_query* pass with z0 = -v folded into conv_out,
    # decode_seg, the ops.seg_* post-processing) and _run_query_step -- and share these rules, stated here once:
    #   scheduler  the reference's degenerate one-step scheduler (z0 = -v) is required; any other raises
    #              NotImplementedError (run_episodes, which falls back to single_infer, takes any).
    #   stale      a support prepared under another test_timestep, prompt, residual-stream mode, resolution or set of
    #              weights raises ValueError (SupportBank.check names the first mismatch).
    #   captured   (default: self.use_graph) as in run_episodes: the step is ONE HIP graph per key -- the route, the
    #              support's uid (its tensors are read in place, so two supports of equal shape never share a graph), the
    #              query shape, whether a ground truth was given, the flags and _graph_key's tail.  Tables of a route
    #              (routed, candidates) are pinned host tensors among the step's static inputs: one H2D copy each per call
    #              into the graph's buffer, read by the kernels when they run, so they are NOT part of the key.  At most
    #              MAX_QUERY_GRAPHS captured query steps are kept per pipeline, over all routes: capturing one more drops
    #              the least recently used (its buffers with it; outputs returned from it must have been consumed).
    #   native     (input_pipeline.NativeTargets for the b queries) the dict gains `native`, the route's ops.seg_*_native on
    #              the step's seg_u8 with the call's flags: launched on the same stream after the step, eagerly even after
    #              a replay (sizes vary per batch), neither part of the graph nor of its key; every other entry is what
    #              the call without `native` returns.
    MAX_QUERY_GRAPHS = 4    # captured query steps kept per pipeline (least recently used goes first)

    @property
    def _vae_factor(self):
        """Image pixels per latent pixel: the encoder halves (floor) once per level but the last."""
        return 2 ** (len(self.vae.config["block_out_channels"]) - 1)

    def _single_step_timestep(self):
        sched = self.scheduler
        sched.set_timesteps(1, device=self.device)
        t = sched.timesteps[0]
        return t, t * self.test_timestep

    def _support_latents(self, sup, msk):
        """Support images and masks [n, 3, H, W] -> cond_ref [n, 2 lc, h, w] fp32: one VAE-encoder launch train over the 2n
        images, quant_conv straight into the halves of cat([z_ref, z_mask_ref]) (P:674), as _episodes_step does."""
        n, lc = sup.shape[0], self.vae.config["latent_channels"]
        mom = self.vae.encoder([sup, msk])                                        # [2n, 2 lc, h, w] fp32
        h, w = mom.shape[-2:]
        cond_ref = torch.empty(n, 2 * lc, h, w, dtype=torch.float32, device=mom.device)
        qc, sf = self.vae.quant_conv, self.rgb_latent_scale_factor
        qc(mom[:n], out_scale=sf, out=cond_ref[:, :lc], channels=lc)              # z_ref      (P:649)
        qc(mom[n:], out_scale=sf, out=cond_ref[:, lc:], channels=lc)              # z_mask_ref (P:651)
        return cond_ref

    def _query_latents(self, query_img, chunk=None):
        """Query images [b, 3, H, W] -> z_tag [b, lc, h, w] fp32 (P:650): the VAE encoder, then quant_conv.  chunk: encode in
        chunks of `chunk` queries, the last one padded by repeating the last query (the padding's latents are returned
        too): GEMM plans, and so the bits, depend on the batch, and this way the encoder runs at batch `chunk` only."""
        lc, sf = self.vae.config["latent_channels"], self.rgb_latent_scale_factor
        if chunk is None:
            return self.vae.quant_conv(self.vae.encoder(query_img), out_scale=sf, channels=lc)
        b = query_img.shape[0]
        pad = -b % chunk
        qs = query_img if not pad else torch.cat([query_img, query_img[-1:].expand(pad, -1, -1, -1)])
        zs = [self.vae.quant_conv(self.vae.encoder(qs[c0:c0 + chunk]), out_scale=sf, channels=lc)
              for c0 in range(0, b + pad, chunk)]
        return zs[0] if len(zs) == 1 else torch.cat(zs)

    def _query_context(self, name, support, wrong, query_img, gt, tables=None):
        """The checks of query route `name`, in the order callers rely on (the first two read no model): `support` is a
        SupportBankSet, else the exception class `wrong` (None: the route takes a SupportBank and leaves the type to
        unet.forward_queries); the scheduler restriction; fold and prompt; the inputs staged on the device as contiguous fp32
        / uint8; tables(b) -- the route's own argument checks, which may raise and whose result is handed back --; and
        support.check against this resolution and the engines' current state.
        Returns (tt, folded, prompt, ins = dict(query_img=, gt=), tables' result)."""
        from .unet import SupportBankSet
        if wrong is not None and not isinstance(support, SupportBankSet):
            raise wrong("bankset must be a SupportBankSet (prepare_support_classes)" if wrong is TypeError else
                        f"{name} needs a SupportBankSet (prepare_support_classes)")
        t, tt = self._single_step_timestep()
        if not self.scheduler.z0_is_neg_v(t):
            raise NotImplementedError(f"{name} needs the one-step scheduler with z0 = -v (the reference's setting); "
                                      "run_episodes() takes any scheduler (the generic single_infer path)")
        folded = self._fold_conditioning(tt)
        dev = self.device
        prompt = None if folded else self.encode_clip_feature()
        ins = dict(query_img=query_img.to(dev, torch.float32).contiguous(), gt=None if gt is None else gt.to(dev).contiguous())
        made = None if tables is None else tables(ins["query_img"].shape[0])
        H, W = ins["query_img"].shape[-2:]
        support.check(hw=(H // self._vae_factor, W // self._vae_factor), dtype=self.unet.dtype,
                      residual_dtype=self.unet.residual_dtype, fold_key=self.unet._fold_key(tt, prompt),
                      weights_id=self.unet._weights_id)
        return tt, folded, prompt, ins, made

    def _touch_query_graph(self, key):
        """Least-recently-used bookkeeping of the captured query steps (keys that start with "queries"; run_episodes' graphs
        are neither counted nor dropped): a known key moves to the end, a new one first drops the oldest until fewer than
        MAX_QUERY_GRAPHS are left."""
        if key in self._graphs:
            self._graphs[key] = self._graphs.pop(key)          # most recently used last
        else:
            mine = [k for k in self._graphs if k[0] == "queries"]
            for k in mine[:max(0, len(mine) - (self.MAX_QUERY_GRAPHS - 1))]:
                del self._graphs[k]

    def _run_query_step(self, key_head, step, ins, tt, folded, captured, finish):
        """finish(the step's dict), the step run eagerly -- pinned host inputs (a route's tables) copied to the device first
        -- or, captured, replayed from the graph keyed _graph_key(key_head, tt, folded)."""
        if captured is None:
            captured = self.use_graph
        if not captured:
            dev = self.device
            return finish(step(**{k: v if v is None or v.is_cuda else v.to(dev, non_blocking=True) for k, v in ins.items()}))
        key = self._graph_key(key_head, tt, folded)
        self._touch_query_graph(key)
        return finish(self._replay(key, step, ins))

    @torch.no_grad()
    def prepare_support(self, support_imgs, support_masks):
        """Prepare ONE support set for any number of segment_queries() calls: support_imgs / support_masks [s, 3, H, W] in
        [-1, 1] -> SupportBank (diffews_amd.unet), the K/V of the s support images in every self-attention layer:
        _support_latents, then one support pass of the UNet (unet.prepare_bank).  The bank is valid for this pipeline's
        current test_timestep, prompt, residual-stream mode and weights, and for queries of the same H x W."""
        t, tt = self._single_step_timestep()
        folded = self._fold_conditioning(tt)
        dev = self.device
        sup = support_imgs.to(dev, torch.float32).contiguous()
        msk = support_masks.to(dev, torch.float32).contiguous()
        if sup.shape != msk.shape or sup.dim() != 4:
            raise ValueError(f"support_imgs {tuple(sup.shape)} and support_masks {tuple(msk.shape)} must both be [s, 3, H, W]")
        return self.unet.prepare_bank(self._support_latents(sup, msk), tt, None if folded else self.encode_clip_feature())

    @torch.no_grad()
    def segment_queries(self, bank, query_img, query_gt=None, r_threshold=0.25, threshold=0.0, batch_max=False,
                        captured=None, native=None):
        """One denoising step for b query images against a prepared support set (prepare_support): query_img
        [b, 3, H, W] in [-1, 1], any b >= 1; query_gt optional uint8 [b, H, W].  Returns run_episodes' dict (z0, dec,
        seg_u8, counts) -- per image what run_episodes computes with the supports replicated b times, without encoding
        the supports or running them through the UNet again: only the queries are encoded, every attn1 reads the bank
        (unet.forward_queries), decode, seg_postprocess.

        Scheduler, stale banks, `captured` and `native` (ops.seg_native): the rules at the head of this section."""
        tt, folded, prompt, ins, _ = self._query_context("segment_queries", bank, None, query_img, query_gt)
        flags = (float(r_threshold), float(threshold), bool(batch_max))

        def step(query_img, gt=None):
            z0 = self.unet.forward_queries(self._query_latents(query_img), tt, bank, prompt, out_scale=-1.0)
            dec = self.decode_seg(z0)
            seg_u8, counts = ops.seg_postprocess(dec, gt, *flags)
            return dict(z0=z0, dec=dec, seg_u8=seg_u8, counts=counts)
        head = ("queries", bank.uid, tuple(ins["query_img"].shape), query_gt is not None, flags)
        return self._run_query_step(head, step, ins, tt, folded, captured,
                                    lambda r: self._with_native(r, native, ops.seg_native, *flags))

    # ------------------------------------------------------------------ N-way: a stack of class banks
    @torch.no_grad()
    def prepare_support_classes(self, support_imgs, support_masks):
        """Prepare the support sets of N classes for segment_classes(): support_imgs / support_masks [N, s, 3, H, W] in
        [-1, 1] (s annotated examples of each class) -> SupportBankSet (diffews_amd.unet).  prepare_support's launches over
        all N * s images at once: _support_latents, then one support pass of the UNet (unet.prepare_bank_sets).  Valid for
        what a SupportBank is valid for.

        Classes with different numbers of examples: give two lists of N tensors [s_c, 3, H, W] instead.  The same launches
        run over all sum(s_c) images and the result is a ragged SupportBankSet (shots == (s_0, ..., s_{N-1})), which
        segment_classes takes like any other."""
        t, tt = self._single_step_timestep()
        folded = self._fold_conditioning(tt)
        dev = self.device
        if isinstance(support_imgs, (list, tuple)):
            if not isinstance(support_masks, (list, tuple)) or len(support_masks) != len(support_imgs) or not support_imgs:
                raise ValueError("support_imgs and support_masks must be two lists of N tensors [s_c, 3, H, W]")
            sups = [t.to(dev, torch.float32) for t in support_imgs]
            msks = [t.to(dev, torch.float32) for t in support_masks]
            for c, (a, m) in enumerate(zip(sups, msks)):
                if a.shape != m.shape or a.dim() != 4 or a.shape[0] < 1 or a.shape[1:] != sups[0].shape[1:]:
                    raise ValueError(f"class {c}: support_imgs {tuple(a.shape)} and support_masks {tuple(m.shape)} must both be "
                                     f"[s_c >= 1, {', '.join(str(d) for d in sups[0].shape[1:])}]")
            shots = tuple(a.shape[0] for a in sups)
            N, sup, msk = len(shots), torch.cat(sups).contiguous(), torch.cat(msks).contiguous()
        else:
            sup = support_imgs.to(dev, torch.float32).contiguous()
            msk = support_masks.to(dev, torch.float32).contiguous()
            if sup.shape != msk.shape or sup.dim() != 5:
                raise ValueError(f"support_imgs {tuple(sup.shape)} and support_masks {tuple(msk.shape)} must both be "
                                 "[N, s, 3, H, W]")
            N, shots = sup.shape[0], None
            sup, msk = sup.flatten(0, 1), msk.flatten(0, 1)
        return self.unet.prepare_bank_sets(self._support_latents(sup, msk), N, tt,
                                           None if folded else self.encode_clip_feature(), shots=shots)

    @torch.no_grad()
    def segment_classes(self, bankset, query_img, query_labels=None, r_threshold=0.25, threshold=0.0, batch_max=False,
                        max_batch=16, captured=None, native=None, class_ids=None):
        """N-way segmentation of b query images against the N prepared classes of `bankset` (prepare_support_classes):
        query_img [b, 3, H, W] in [-1, 1]; query_labels optional uint8 [b, H, W] with 0 = background, 1 + c = class c,
        255 (or anything above N) = ignore.  The queries are encoded ONCE; the classes go through the UNet and the decoder
        in chunks of max(1, max_batch // b) sets (64 at the most), each chunk one class-major batch whose attn1 reads its sets of the stack
        in place (unet.forward_query_sets); seg_postprocess writes every chunk into its slice of one uint8 buffer and of
        the maxima, and one ops.seg_labels launch fuses the N masks into labels and counts.

        Returns dict(z0 [N, b, 4, h, w], dec [N, b, 3, H, W], seg_u8 [N, b, 3, H, W], labels uint8 [b, H, W], counts int64
        [b, 2, N+1] or None) -- z0[c] / dec[c] / seg_u8[c] are what segment_queries(bankset.bank(c), query_img) returns;
        a class is foreground where segment_queries' prediction is (batch_max: the maximum over that class' b masks) and
        the label is 0 where none is, else 1 + the foreground class of the largest mean mask value, lowest class on a
        tie; counts rows are per-label intersections and unions (metrics.nway_iou).

        TypeError for anything but a SupportBankSet.  Scheduler, stale sets, `captured` (max_batch is part of the key) and
        `native`: the rules at the head of this section; `native` is ops.seg_labels_native with this call's flags and
        `class_ids` -- labels, and per-label counts against the targets' ground truth, at every query's own h x w."""
        tt, folded, prompt, ins, _ = self._query_context("segment_classes", bankset, TypeError, query_img, query_labels)
        b, _, H, W = ins["query_img"].shape
        flags = (float(r_threshold), float(threshold), bool(batch_max))
        N, per = bankset.nsets, min(64, max(1, int(max_batch) // b))     # a ragged launch carries at most 64 sets

        def step(query_img, gt=None):
            z_tag = self._query_latents(query_img)
            seg_u8 = torch.empty(N, b, 3, H, W, dtype=torch.uint8, device=query_img.device)
            mx = torch.empty(N * b, dtype=torch.int32, device=query_img.device)
            z0s, decs = [], []
            for c0 in range(0, N, per):
                c1 = min(N, c0 + per)
                z0 = self.unet.forward_query_sets(z_tag, tt, bankset, prompt, out_scale=-1.0, sets=range(c0, c1))
                dec = self.decode_seg(z0.view(-1, *z0.shape[2:]))
                # gt-less call: zeroes this chunk's maxima, quantises, takes the per-image maxima
                ops.seg_postprocess(dec, None, *flags, u8_out=seg_u8[c0:c1].view(-1, 3, H, W), scratch=mx[c0 * b:c1 * b])
                z0s.append(z0)
                decs.append(dec.view(c1 - c0, b, *dec.shape[1:]))
            labels, counts = ops.seg_labels(seg_u8, mx, gt, *flags)
            z0 = z0s[0] if len(z0s) == 1 else torch.cat(z0s)
            dec = decs[0] if len(decs) == 1 else torch.cat(decs)
            return dict(z0=z0, dec=dec, seg_u8=seg_u8, labels=labels, counts=counts)
        head = ("queries", "classes", bankset.uid, tuple(ins["query_img"].shape), query_labels is not None, flags, int(max_batch))
        return self._run_query_step(head, step, ins, tt, folded, captured,
                                    lambda r: self._with_native(r, native, ops.seg_labels_native, *flags, class_ids=class_ids))

    # ------------------------------------------------------------------ routed queries: one class of a stack per query
    @torch.no_grad()
    def segment_routed(self, bankset, query_img, route, query_gt=None, r_threshold=0.25, threshold=0.0, batch_max=False,
                       captured=None, native=None):
        """One denoising step for b query images, EACH against one class of `bankset` (prepare_support_classes, uniform or
        ragged): query_img [b, 3, H, W] in [-1, 1], `route` b set indices (any order, repeats allowed, sets may go
        unused), query_gt optional uint8 [b, H, W].  Returns segment_queries' dict (z0, dec, seg_u8, counts): entry i is,
        per image, what segment_queries(bankset.bank(route[i]), query_img[i:i+1]) computes -- in one pass of batch b
        whose every attn1 reads the stack in place through a device table of (first image, shots) rows
        (unet.forward_query_routed, ops.fsa_attention_routed), where segment_classes would run all N classes per query.

        ValueError for anything but a SupportBankSet and for a route that is not b long or names a set outside the stack.
        Scheduler, stale sets, `captured` and `native` (ops.seg_native): the rules at the head of this section.  The
        route table is the step's one table: one graph serves every route of that shape.  A replay runs no library-side
        validation of the table; it needs none, because SupportBankSet.route_table builds every row from the set's own
        offsets."""
        def tables(b):
            table_host = bankset.route_table(route)          # ValueError: empty, or a set outside the stack
            if table_host.shape[0] != b:
                raise ValueError(f"a route of {table_host.shape[0]} entries for {b} queries")
            return table_host
        tt, folded, prompt, ins, table_host = self._query_context("segment_routed", bankset, ValueError, query_img, query_gt,
                                                                  tables)
        flags = (float(r_threshold), float(threshold), bool(batch_max))
        ins["table"] = table_host = table_host.pin_memory()

        def step(query_img, table, gt=None):
            # table_host mirrors `table` whenever this runs (eagerly, or while a graph is warmed up and captured)
            z0 = self.unet.forward_query_routed(self._query_latents(query_img), tt, bankset, table, table_host, prompt,
                                                out_scale=-1.0)
            dec = self.decode_seg(z0)
            seg_u8, counts = ops.seg_postprocess(dec, gt, *flags)
            return dict(z0=z0, dec=dec, seg_u8=seg_u8, counts=counts)
        head = ("queries", "routed", bankset.uid, tuple(ins["query_img"].shape), query_gt is not None, flags)
        return self._run_query_step(head, step, ins, tt, folded, captured,
                                    lambda r: self._with_native(r, native, ops.seg_native, *flags))

    # ------------------------------------------------------------------ candidate classes per query, one label map
    @torch.no_grad()
    def segment_candidates(self, bankset, query_img, candidates, query_labels=None, r_threshold=0.25, threshold=0.0,
                           entry_batch=8, labels="set", captured=None):
        """One label map per query over a SUBSET of `bankset`'s classes, a different subset per query: query_img
        [b, 3, H, W] in [-1, 1]; `candidates` b sequences of set indices (sorted here, so the lowest class wins a tie; a
        query may have none, the batch needs at least one); query_labels optional uint8 [b, H, W] in the labels the call
        writes (0 = background, 255 or anything above nlabels = ignore).  It sits between segment_classes (all N classes
        for every query) and segment_routed (one class per query, a binary mask): the cost is one UNet entry per
        (query, candidate) pair -- E = sum of the list lengths -- whatever N is.

        The b queries are VAE-encoded ONCE, however many candidates they have -- in chunks of entry_batch queries, the last
        chunk padded by repeating the last query, so that the encoder too runs at batch entry_batch (_query_latents): with
        every kernel of the step at ONE batch an entry is bit for bit what segment_routed computes at that batch, whatever
        b and the other candidates are.  An entry_batch that divides b pads nothing.  The E entries, query-major, are
        padded to E_pad (a multiple of entry_batch; SupportBankSet.candidate_tables) and run as E_pad / entry_batch passes
        of entry_batch entries: the pass's latents
        are gathered by index_select on a device index tensor, the pass goes through unet.forward_query_routed on its rows
        of the (first image, shots) table, decode_seg, and a gt-less ops.seg_postprocess into its slice of one seg_u8 / maxima
        buffer; one ops.seg_labels_cand launch then fuses every query's entries into its label map.  There is no batch_max
        form: a maximum over "the class' b images" has no meaning when every query has its own classes.

        labels="set": label = 1 + set index, nlabels = nsets.  labels="local": label = 1 + position in the query's sorted
        list, nlabels = the longest list (a library of more than 254 classes; query_labels is then in local labels).

        Returns dict(z0 [E, 4, h, w], dec [E, 3, H, W], seg_u8 [E, 3, H, W], labels uint8 [b, H, W], counts int64
        [b, 2, nlabels+1] or None, area int64 [E, 2] = per entry (pixels foreground on its own, pixels where it won the
        label), entries = the (query, set) pair of every entry, offsets = b + 1 ints, query i owns entries
        [offsets[i], offsets[i+1])).  Entry e is what segment_routed computes for the same pass batch; a gt label that is
        not among the query's candidates counts as a miss in that label's union.

        ValueError for anything but a SupportBankSet, for a number of lists other than b and for what candidate_tables
        rejects.  Scheduler, stale sets and `captured`: the rules at the head of this section.  The entry indices, the
        rows and the label table are the step's tables; the key also holds E_pad, entry_batch, labels and nlabels, so one
        graph serves every assignment with the same b and number of passes (with labels="local" also the same longest
        list).

        entry_batch = 8 is a choice, not a measurement.  It bounds the decoder's batch: 16 entries at 512 x 512 reach the
        VAE decoder's 2 GiB buffer-descriptor range (DFW_ERANGE).

        segment_candidates_native is this call plus labels and counts at every query's own size."""
        return self._segment_candidates(bankset, query_img, candidates, query_labels, r_threshold, threshold, entry_batch,
                                        labels, captured)

    @torch.no_grad()
    def segment_candidates_native(self, bankset, query_img, candidates, native, class_ids=None, query_labels=None,
                                  r_threshold=0.25, threshold=0.0, entry_batch=8, labels="set", captured=None):
        """segment_candidates with its result scored at every query's OWN size: the same arguments, the same step, the same
        graph and key, and the same dict with one more entry.

        native (input_pipeline.NativeTargets for these b queries): the dict gains `native` = dict(labels [uint8 [h_i, w_i]],
        counts int64 [b, 2, nlabels+1] or None, area int64 [E, 2], mx int32 [E], sizes) -- ops.seg_labels_cand_native on the
        step's seg_u8 and this call's table and flags: every entry resized to its query's own h x w, the label rule on the
        resized bytes, counts against the targets' ground truth read in place; otherwise the section's `native` rule.
        ValueError without `native`.
        class_ids: the ground-truth id of each SET, nsets ints, for targets that hold class-id maps.  With labels="set" it
        is the table from id to label 1 + set; a class outside the query's candidates is a miss in its label's union.  With
        labels="local" it is gathered per entry, and an id none of the query's candidates carries is background (local
        labels have no bin for it).  Without class_ids the targets hold label maps in the labels the call writes."""
        if native is None:
            raise ValueError("segment_candidates_native needs NativeTargets for the queries; without them call segment_candidates")
        return self._segment_candidates(bankset, query_img, candidates, query_labels, r_threshold, threshold, entry_batch,
                                        labels, captured, native, class_ids)

    def _segment_candidates(self, bankset, query_img, candidates, query_labels, r_threshold, threshold, entry_batch, labels,
                            captured, native=None, class_ids=None):
        """The body of segment_candidates / segment_candidates_native (callers hold torch.no_grad)."""
        def tables(b):
            cands = list(candidates)
            if len(cands) != b:
                raise ValueError(f"{len(cands)} candidate lists for {b} queries")
            return bankset.candidate_tables(cands, entry_batch, labels)       # ValueError: see candidate_tables
        tt, folded, prompt, ins, ct = self._query_context("segment_candidates", bankset, ValueError, query_img, query_labels,
                                                          tables)
        b, _, H, W = ins["query_img"].shape
        E, E_pad, nlabels, eb = ct["E"], ct["E_pad"], ct["nlabels"], int(entry_batch)
        flags = (float(r_threshold), float(threshold))
        rows_host, tab_host = ct["rows"].pin_memory(), ct["tab"].pin_memory()
        ins.update(entries=ct["entries"].pin_memory(), rows=rows_host, tab=tab_host)

        def step(query_img, entries, rows, tab, gt=None):
            z_tag = self._query_latents(query_img, eb)      # every kernel of the step runs at batch entry_batch
            seg_u8 = torch.empty(E_pad, 3, H, W, dtype=torch.uint8, device=query_img.device)
            mx = torch.empty(E_pad, dtype=torch.int32, device=query_img.device)
            z0s, decs = [], []
            for e0 in range(0, E_pad, eb):
                # the indices and rows are read on the device: a capture bakes in the pointers, not the candidates.
                # rows_host mirrors `rows` whenever this runs (eagerly, or while a graph is warmed up and captured)
                zp = z_tag.index_select(0, entries[e0:e0 + eb])
                z0 = self.unet.forward_query_routed(zp, tt, bankset, rows[e0:e0 + eb], rows_host[e0:e0 + eb], prompt,
                                                    out_scale=-1.0)
                dec = self.decode_seg(z0)
                # gt-less call: zeroes this pass's maxima, quantises, takes the per-entry maxima
                ops.seg_postprocess(dec, None, *flags, False, u8_out=seg_u8[e0:e0 + eb], scratch=mx[e0:e0 + eb])
                z0s.append(z0)
                decs.append(dec)
            lab, counts, area = ops.seg_labels_cand(seg_u8, mx, tab, tab_host, nlabels, gt, *flags, want_area=True)
            z0 = z0s[0] if len(z0s) == 1 else torch.cat(z0s)
            dec = decs[0] if len(decs) == 1 else torch.cat(decs)
            return dict(z0=z0, dec=dec, seg_u8=seg_u8, labels=lab, counts=counts, area=area, tab=tab)

        ids_kw = {}
        if class_ids is not None:
            ids = torch.as_tensor(class_ids, dtype=torch.int32)
            if ids.shape != (bankset.nsets,):
                raise ValueError(f"class_ids must hold one id per set ({bankset.nsets}), got {tuple(ids.shape)}")
            # "set": the table from id to label 1 + set; "local": the id of every entry's own set
            ids_kw = dict(class_ids=ids) if labels == "set" else \
                dict(entry_ids=ids[ct["entry_sets"].to(ids.device, non_blocking=True).long()])

        def trimmed(r):       # the padding entries are dropped from what the caller sees; the candidates are the call's own
            out = {k: r[k][:E] for k in ("z0", "dec", "seg_u8", "area")}
            out.update(labels=r["labels"], counts=r["counts"],
                       entries=[(i, c) for i, cs in enumerate(ct["sets"]) for c in cs],
                       offsets=ct["tab"][:b + 1].tolist())
            if native is not None:
                # eagerly after the step, on its seg_u8 (padding entries included: the table never names them) and its table
                n = ops.seg_labels_cand_native(r["seg_u8"], native, r["tab"], tab_host, nlabels, *flags, want_area=True, **ids_kw)
                out["native"] = dict(labels=n["labels"], counts=n["counts"], area=n["area"][:E], mx=n["mx"][:E],
                                     sizes=n["sizes"])
            return out
        head = ("queries", "candidates", bankset.uid, tuple(ins["query_img"].shape), E_pad, eb, labels, nlabels,
                query_labels is not None, flags)
        return self._run_query_step(head, step, ins, tt, folded, captured, trimmed)

    def segment_stream(self, support, queries, batch=4, size=None, depth=2, class_value=None, ignore_value=-1,
                       class_ids=None, r_threshold=0.25, threshold=0.0, batch_max=False, max_batch=16, captured=None,
                       route=None, candidates=None, entry_batch=8, labels="set", native=False):
        """Generator: a stream of decoded images against one prepared support -- `support` a SupportBank (prepare_support;
        routed to segment_queries) or a SupportBankSet (prepare_support_classes; routed to segment_classes, with
        `class_ids` and `max_batch`).  `queries` yields dicts with `query_img` (PIL / uint8 [H, W, 3], any size) and
        optionally `gt` ([H, W] class-id or label map); an input_pipeline.QueryLoader (`batch`, `depth`, `class_value`,
        `ignore_value`; `size` = processing size, default: the one the support was prepared at) resizes and normalises
        them on a side stream, one H2D copy and three launches per batch, while the previous batch is in the UNet.

        Yields (index, r): `index` the positions of the batch's queries in the stream, `r` the routed call's dict with
        `native` present -- masks / labels at every query's own size and, with `gt`, counts against it read in place from
        the batch's staged bytes.  With `class_value` (SupportBank only) the queries' nearest-resized 0/1 masks also feed
        r["counts"] at the processing size.  The last batch may be short.

        r is valid until the next item is drawn: its tensors belong to a captured step's outputs and to the loader's
        recycled slots, and drawing the next item lets both be overwritten.  Consume (or clone) it first, on the current
        stream; no host synchronisation is needed.

        route (a SupportBankSet only, else ValueError): a callable on the query dict, or the name of one of its keys, that
        gives the index of the ONE set the query is segmented against -- a stream whose class changes from query to
        query.  Every batch then goes through segment_routed (r is segment_queries' dict, plus `route`, the batch's set
        indices) instead of segment_classes; with `class_ids` the ground-truth id of query i is class_ids[route_i], so
        r["native"]["counts"] and the processing-size r["counts"] are binary counts for the query's own class.

        candidates (a SupportBankSet only, and not together with `route`, else ValueError): a callable on the query dict,
        or the name of one of its keys, that gives the indices of the sets the query is segmented against -- a handful
        of the library's classes, a different handful per query.  Every batch then goes through segment_candidates with
        `entry_batch` and `labels` (r is its dict, plus `candidates`, the batch's lists as given).  The ground truth of
        the processing-size r["counts"] is q["labels"] when the queries carry one: a label map ALREADY at the processing
        size, in the labels the call writes.  `class_value` and `batch_max` do not apply (ValueError when given).
        native (read with `candidates` only -- the other routes always return `native`; default False, and then r has no
        `native` and `class_ids` is a ValueError): every batch goes through segment_candidates_native with the loader's
        NativeTargets, so r["native"] holds the native-size labels, area and -- when the queries carry `gt` -- counts against it read in place from the batch's staged bytes; `class_ids` is then the
        ground-truth id of each set, as segment_candidates_native takes it."""
        from .input_pipeline import QueryLoader
        from .unet import SupportBank, SupportBankSet
        if not isinstance(support, (SupportBank, SupportBankSet)):
            raise TypeError("support must be a SupportBank (prepare_support) or a SupportBankSet (prepare_support_classes)")
        nway = isinstance(support, SupportBankSet)
        if route is not None and not nway:
            raise ValueError("route picks one set of a SupportBankSet per query; a SupportBank has only one")
        if nway and class_value is not None:
            raise ValueError("class_value belongs to a SupportBank; with a SupportBankSet give class_ids")
        if not nway and class_ids is not None:
            raise ValueError("class_ids belongs to a SupportBankSet; with a SupportBank give class_value")
        if size is None:
            size = (support.hw[0] * self._vae_factor, support.hw[1] * self._vae_factor)
        getter = lambda g: g if callable(g) else (lambda q: q[g])     # a callable on the query dict, or the name of a key
        flags = dict(r_threshold=r_threshold, threshold=threshold, captured=captured)
        # per route: the QueryLoader's own keywords and call(bt) -> r; every argument error before the first batch is drawn
        if candidates is not None:
            if not nway:
                raise ValueError("candidates name sets of a SupportBankSet; a SupportBank has only one")
            if route is not None:
                raise ValueError("give `route` (one set per query, a binary mask) or `candidates` (a label map), not both")
            if batch_max:
                raise ValueError("batch_max does not apply to candidates (there is no batch_max form)")
            if class_ids is not None and not native:
                raise ValueError("class_ids maps the ground truth of the native-size pass: give native=True with it")
            if class_ids is not None:     # staged once, not per batch
                class_ids = torch.as_tensor(class_ids, dtype=torch.int32).to(self.device)
            loader_kw = dict(candidates=getter(candidates))

            def call(bt):
                kw = dict(query_labels=bt.get("query_labels"), entry_batch=entry_batch, labels=labels, **flags)
                if native:
                    r = self.segment_candidates_native(support, bt["query_img"], bt["candidates"], bt["native"], class_ids, **kw)
                else:
                    r = self.segment_candidates(support, bt["query_img"], bt["candidates"], **kw)
                return dict(r, candidates=bt["candidates"])
        elif route is not None:
            route_of = getter(route)
            if class_ids is not None:     # the query's own class is its foreground value (QueryLoader's callable form)
                ids = [int(c) for c in class_ids]
                if len(ids) != support.nsets:
                    raise ValueError(f"{len(ids)} class_ids for a support bank set of {support.nsets}")

                def class_value(q):
                    c = int(route_of(q))
                    if not 0 <= c < len(ids):
                        raise ValueError(f"a query is routed to set {c} of a support bank set of {len(ids)}")
                    return ids[c]
            loader_kw = dict(class_value=class_value, route=route_of)

            def call(bt):
                r = self.segment_routed(support, bt["query_img"], bt["route"], bt.get("query_mask"), native=bt["native"],
                                        batch_max=batch_max, **flags)
                return dict(r, route=bt["route"])
        else:
            if class_ids is not None:     # staged once, not per batch
                class_ids = torch.as_tensor(class_ids, dtype=torch.int32).to(self.device)
            loader_kw = dict(class_value=class_value)

            def call(bt):
                if nway:
                    return self.segment_classes(support, bt["query_img"], None, max_batch=max_batch, native=bt["native"],
                                                class_ids=class_ids, batch_max=batch_max, **flags)
                return self.segment_queries(support, bt["query_img"], bt.get("query_mask"), native=bt["native"],
                                            batch_max=batch_max, **flags)
        for bt in QueryLoader(queries, size, batch, device=self.device, depth=depth, ignore_value=ignore_value, **loader_kw):
            yield bt["index"], call(bt)

    def _tile_stage(self, support, image, gt, overlap, ramp, batch):
        """segment_tiled's staging: the TilePlan of `image` for windows of the size `support` was prepared at; image and gt
        through one pinned buffer and one H2D copy; the window transform (kept on the pipeline between calls); and one fp32
        [batch, 3, th, tw] query buffer.  Returns (plan, its C record, gt on the device [1, h, w] or None, cut), where
        cut(runs) fills that buffer -- one ops.tiles_cut per (first window, count) run, in order, the rest of the batch
        padded by repeating the last window cut -- and returns it."""
        from .input_pipeline import DeviceImageTransform, TilePlan
        th, tw = support.hw[0] * self._vae_factor, support.hw[1] * self._vae_factor
        img = DeviceImageTransform.as_rgb_bytes(image)
        h, w = img.shape[:2]
        plan = TilePlan((h, w), (th, tw), min(th, tw) // 8 if overlap is None else overlap, ramp)
        if gt is not None:
            gt = np.ascontiguousarray(gt.cpu().numpy() if torch.is_tensor(gt) else gt)
            if gt.dtype != np.uint8 or gt.shape != (h, w):
                raise ValueError(f"gt must be a uint8 label map [{h}, {w}], got {gt.dtype} {gt.shape}")
        n_img = 3 * h * w
        host = torch.empty(n_img + (h * w if gt is not None else 0), dtype=torch.uint8, pin_memory=True)
        host[:n_img].view(h, w, 3).numpy()[...] = img
        if gt is not None:
            host[n_img:].view(h, w).numpy()[...] = gt
        staged = host.to(self.device, non_blocking=True)                       # the one H2D copy
        img_dev = staged[:n_img].view(h, w, 3)
        gt_dev = staged[n_img:].view(1, h, w) if gt is not None else None
        tf = getattr(self, "_tile_tf", None)
        if tf is None or (tf.out_h, tf.out_w) != (th, tw) or tf.device != torch.device(staged.device):
            tf = self._tile_tf = DeviceImageTransform((th, tw), staged.device)  # owns the ToTensor + Normalize table
        cplan = plan.c_struct()
        q = torch.empty(batch, 3, th, tw, dtype=torch.float32, device=staged.device)

        def cut(runs):
            n = 0
            for first, count in runs:
                ops.tiles_cut(cplan, img_dev, tf.lut, first, count, out=q[n:n + count])
                n += count
            if n < batch:
                q[n:] = q[n - 1]                                              # padding: the last window again
            return q
        return plan, cplan, gt_dev, cut

    @torch.no_grad()
    def segment_tiled(self, support, image, gt=None, overlap=None, ramp=None, batch=4, r_threshold=0.25, threshold=0.0,
                      max_batch=16, captured=None, candidates=None, entry_batch=8):
        """One image LARGER than the processing size, segmented at its own resolution: `image` (PIL / uint8 [h, w, 3]) is
        covered with overlapping windows of the size `support` was prepared at (input_pipeline.TilePlan: `overlap`, default
        min(tile) // 8, and `ramp`), every window is one query of segment_queries (`support` a SupportBank) or
        segment_classes (a SupportBankSet, uniform or ragged, with `max_batch`), the windows' seg_u8 are blended back into
        one image (ops.tiles_merge) and that image is thresholded ONCE by ops.seg_labels: the dynamic threshold uses the
        merged image's maximum per class, so a window without the object cannot turn its noise into foreground.

        The image (and `gt`, optional uint8 [h, w]: 0 = background, 1 + c = class c, 255 = ignored; 0 / 1 / 255 for a bank)
        goes through one pinned buffer and one H2D copy.  Windows are cut on the device (ops.tiles_cut) and run in batches
        of `batch`, the last one padded by repeating the image's last window, so ONE captured graph serves the whole image;
        each batch's seg_u8 is copied on the same stream into its slice of one uint8 [N, T, 3, th, tw] buffer (3 * th * tw
        bytes per window and class) before the next call overwrites it, the padding never.  Cut, merge and labels run
        eagerly (their sizes vary per image) and are part of no graph.

        Returns dict(seg_u8 uint8 [N, 3, h, w], labels uint8 [h, w], counts, mx int32 [N], plan); N = 1 for a bank, where
        `pred` is an alias of `labels` and counts is int64 [4] in seg_postprocess' order (inter0, inter1, union0, union1);
        for a set counts is int64 [2, N+1] (metrics.nway_iou); counts is None without gt.  There is no batch_max: the
        merged image has one maximum per class.  Scheduler, stale supports and `captured`: the rules at the head of the
        support-bank section; an image smaller than the tile in either axis is a ValueError (segment_stream resizes).

        candidates (a SupportBankSet only, else ValueError; default None: everything above, launch for launch): T lists of
        set indices, or a callable on the TilePlan that returns them (plan.candidates_from_labels, or
        propose_tile_candidates' lists) -- the classes each WINDOW is segmented against.  A (window, class) pair that is
        not listed is DECLARED to have returned an all-zero mask: the result is bit for bit the dense route's merge and
        labels on a window buffer that holds the listed pairs' seg_u8 and zeros elsewhere, so a class ramps down to 0 toward
        a neighbouring window that does not list it, and a class no window lists is never foreground.  The cost follows
        the scene: the windows with a non-empty list, in ascending order, run in groups of `batch` (the last group padded
        by repeating its last window with an EMPTY list: no entry more, the same graph key) through segment_candidates
        (`entry_batch`, labels="set"), one UNet entry per listed pair; each group's seg_u8 is copied on the same stream
        into its slice of one uint8 [E, 3, th, tw] buffer, and one ops.tiles_labels_cand call merges and labels them.  No
        buffer is sized by N * T or by N * h * w; with every list empty no UNet runs and the labels are all 0.

        With candidates the call returns dict(labels uint8 [h, w], counts int64 [2, N+1] or None, mx int32 [N], area int64
        [N, 2] = per class (pixels foreground on its own, pixels where it won), entries = the (window, set) pair of every
        entry, offsets = T + 1 ints, window t owns entries [offsets[t], offsets[t+1]), groups = the (windows, lists)
        passed to each segment_candidates call, padding included -- enough to replay the calls --, plan).  There is no
        seg_u8 key: the merged [N, 3, h, w] image is what this route exists not to build."""
        from .unet import SupportBank, SupportBankSet
        if not isinstance(support, (SupportBank, SupportBankSet)):
            raise TypeError("support must be a SupportBank (prepare_support) or a SupportBankSet (prepare_support_classes)")
        nway = isinstance(support, SupportBankSet)
        if candidates is not None and not nway:
            raise ValueError("candidates name sets of a SupportBankSet; a SupportBank has only one")
        batch = int(batch)
        if batch < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        plan, cplan, gt_dev, cut = self._tile_stage(support, image, gt, overlap, ramp, batch)
        h, w, th, tw, dev = plan.img_h, plan.img_w, plan.tile_h, plan.tile_w, self.device
        N, T = (support.nsets if nway else 1), plan.T
        if candidates is not None:
            ct = plan.candidate_table(candidates(plan) if callable(candidates) else candidates, N)   # ValueError: see there
            sets, E = ct["sets"], ct["E"]
            tab_host = ct["tab"].pin_memory()
            tab = tab_host.to(dev, non_blocking=True)
            ent = torch.empty(E, 3, th, tw, dtype=torch.uint8, device=dev) if E else None
            live = [t for t in range(T) if sets[t]]
            groups, e0 = [], 0
            for g0 in range(0, len(live), batch):
                ws = live[g0:g0 + batch]
                runs = []                                                     # one cut per run of adjacent windows
                for t in ws:
                    if runs and t == runs[-1][0] + runs[-1][1]:
                        runs[-1][1] += 1
                    else:
                        runs.append([t, 1])
                q = cut(runs)
                pad = batch - len(ws)                                         # padding: the last window again, no candidate
                group = (tuple(ws) + (ws[-1],) * pad, tuple(sets[t] for t in ws) + ((),) * pad)
                r = self.segment_candidates(support, q, group[1], None, r_threshold=r_threshold, threshold=threshold,
                                            entry_batch=entry_batch, labels="set", captured=captured)
                n = r["seg_u8"].shape[0]                                      # the group's entries, window-major
                ent[e0:e0 + n].copy_(r["seg_u8"])                             # before the next call overwrites it
                e0 += n
                groups.append(group)
            labels, counts, mx, area = ops.tiles_labels_cand(cplan, ent, tab, tab_host, N, None if gt is None else gt_dev[0],
                                                             r_threshold, threshold, want_area=True)
            return dict(labels=labels, counts=counts, mx=mx, area=area, plan=plan, groups=groups,
                        entries=[(t, c) for t, cs in enumerate(sets) for c in cs], offsets=ct["tab"][:T + 1].tolist())
        win = torch.empty(N, T, 3, th, tw, dtype=torch.uint8, device=dev)
        for first in range(0, T, batch):
            count = min(batch, T - first)
            q = cut([(first, count)])
            if nway:
                r = self.segment_classes(support, q, None, r_threshold=r_threshold, threshold=threshold,
                                         max_batch=max_batch, captured=captured)
                win[:, first:first + count].copy_(r["seg_u8"][:, :count])
            else:
                r = self.segment_queries(support, q, None, r_threshold=r_threshold, threshold=threshold, captured=captured)
                win[0, first:first + count].copy_(r["seg_u8"][:count])
        seg_u8, mx = ops.tiles_merge(cplan, win)
        labels, counts = ops.seg_labels(seg_u8.view(N, 1, 3, h, w), mx, gt_dev, r_threshold, threshold, False)
        out = dict(seg_u8=seg_u8, labels=labels[0], mx=mx, plan=plan,
                   counts=None if counts is None else (counts[0] if nway else counts.view(4)))
        if not nway:
            out["pred"] = out["labels"]
        return out

    @torch.no_grad()
    def propose_tile_candidates(self, library, image, overlap=None, ramp=None, min_pixels=1, margin=1,
                                **segment_classes_flags):
        """The simplest way to CHOOSE segment_tiled's candidates: one coarse pass over the whole image.  `image` (PIL /
        uint8 [h, w, 3]) is squeezed to the processing size `library` (a SupportBankSet) was prepared at by
        DeviceImageTransform, ONE segment_classes call with b = 1 (`segment_classes_flags` are its keywords) labels it
        against all N classes, the labels are brought to the host -- the one host synchronisation of this call -- and
        TilePlan.candidates_from_labels(labels, min_pixels, margin) reads off, per window of the plan segment_tiled will
        build for the same `overlap` / `ramp`, the classes seen inside the window's footprint (grown by `margin` pixels of
        the coarse map).

        Returns (plan_args, lists): plan_args = dict(overlap=, ramp=) and lists = T lists of set indices, usable as
        segment_tiled(library, image, **plan_args, candidates=lists).  A composition of existing calls; how good the
        proposals are depends on the weights and is not claimed here."""
        from .input_pipeline import DeviceImageTransform, TilePlan
        from .unet import SupportBankSet
        if not isinstance(library, SupportBankSet):
            raise ValueError("propose_tile_candidates needs a SupportBankSet (prepare_support_classes)")
        th, tw = library.hw[0] * self._vae_factor, library.hw[1] * self._vae_factor
        img = DeviceImageTransform.as_rgb_bytes(image)
        overlap = min(th, tw) // 8 if overlap is None else overlap
        plan = TilePlan(img.shape[:2], (th, tw), overlap, ramp)
        q = DeviceImageTransform((th, tw), self.device).image(img)
        r = self.segment_classes(library, q[None], None, **segment_classes_flags)
        coarse = r["labels"][0].cpu()                                          # the one host synchronisation
        return dict(overlap=overlap, ramp=ramp), plan.candidates_from_labels(coarse.numpy(), min_pixels, margin)

    @torch.no_grad()
    def objects(self, result, gt=None, key="labels", **kw):
        """The objects of a route's result: objects.label_objects on result["native"][key] when the route ran at native
        size (a list of [h_i, w_i] maps, one call per item), otherwise on result[key].  key: "labels" for the N-way,
        candidate and tiled routes, "pred" for the binary routes (their 0 / 1 mask is a one-class label map).  gt and the
        keywords (connectivity, min_area, max_components, nlabels, buffers) are label_objects'.  Returns its dict."""
        from .objects import label_objects
        src = result.get("native") or result
        if src.get(key) is None:
            raise KeyError(f"the result holds no {key!r} map (binary routes: key='pred')")
        return label_objects(src[key], gt, **kw)

    def object_runs(self, o, **kw):
        """The run-length encoding of every object of pipe.objects' result: objects.object_runs(o, **kw) -- order
        ("column", COCO's, or "row"), max_runs, buffers.  Returns its dict; objects.runs_to_host brings it to the host."""
        from .objects import object_runs
        return object_runs(o, **kw)

    def object_contours(self, o, **kw):
        """The outline of every object of pipe.objects' (or pipe.fill_holes') result as rings of corner points:
        objects.object_contours(o, **kw) -- connectivity, max_edges, buffers, and tolerance (pixels) for the simplified
        rings next to them, result["simplified"]."""
        from .objects import object_contours
        return object_contours(o, **kw)

    def match_objects(self, o_pred, o_gt, **kw):
        """The objects of a prediction matched to those of a ground truth: objects.match_objects(o_pred, o_gt, **kw) on two
        pipe.objects / label_objects results -- skip, iou, nlabels, buffers.  Returns its dict; objects.matches_to_host
        brings it to the host and metrics.panoptic_quality turns its pq table into PQ, SQ and RQ."""
        from .objects import match_objects
        return match_objects(o_pred, o_gt, **kw)

    def object_scores(self, result, o, candidates=None, labels="global", key=None, buffers=None):
        """How sure the model is of every object of pipe.objects' result o: objects.object_scores on the mask planes the
        route's `result` kept and the plane table that belongs to them --
          segment_queries / run_episodes / segment_routed   seg_u8 [b, 3, H, W], objects.planes_for_binary(b)
          segment_classes                                   seg_u8 [N, b, 3, H, W], objects.planes_for_classes(N, b)
          segment_candidates                                seg_u8 [E, 3, H, W], objects.planes_for_candidates of
                                                            `candidates` (the lists the route was given) and `labels`
                                                            ("global": label = 1 + set index, the route's "set"; "local")
          dense segment_tiled                               seg_u8 [N, 3, h, w], objects.planes_for_classes(N, 1)
          the binary native route                           result["native"]["seg_u8"], a list of [3, h_i, w_i], one call
                                                            per item with objects.planes_for_binary(1)
        key (optional): the map o was made from, as given to pipe.objects; KeyError when the result holds none.
        ValueError, naming the reason, for the routes that keep no planes at the label map's size: the N-way and candidate
        native routes (their planes stay at the processing size) and segment_tiled with candidates (the merged image is
        never built); and for a candidate result without `candidates`.  Returns objects.object_scores' dict;
        objects.scores_to_host brings it to the host."""
        from . import objects as ob
        nat = result.get("native")
        src = nat or result
        if key is not None and src.get(key) is None:
            raise KeyError(f"the result holds no {key!r} map (binary routes: key='pred')")
        if nat:
            if nat.get("labels") is not None:
                raise ValueError("object_scores: the N-way and candidate native routes keep their planes at the processing "
                                 "size only; there are no planes at the native label maps' sizes to score")
            if nat.get("seg_u8") is None:
                raise ValueError("object_scores: the native result holds no seg_u8 planes (ops.seg_native want_u8=False)")
            return ob.object_scores(o, [p.contiguous() for p in nat["seg_u8"]], ob.planes_for_binary(1), buffers)
        seg_u8 = result.get("seg_u8")
        if "plan" in result:
            if seg_u8 is None:
                raise ValueError("object_scores: segment_tiled with candidates never builds the merged planes; there is "
                                 "nothing at the label map's size to score")
            return ob.object_scores(o, seg_u8, ob.planes_for_classes(seg_u8.shape[0], 1), buffers)
        if seg_u8 is None:
            raise ValueError("object_scores: the result holds no seg_u8 planes")
        if "entries" in result:
            if candidates is None:
                raise ValueError("object_scores: a segment_candidates result needs candidates=, the lists the route was given")
            lists = [sorted(int(c) for c in (cs.tolist() if isinstance(cs, torch.Tensor) else cs)) for cs in candidates]
            nlabels = max([len(cs) if labels == "local" else 1 + max(cs, default=0) for cs in lists] + [1])
            return ob.object_scores(o, seg_u8, ob.planes_for_candidates(lists, nlabels, labels), buffers)
        if seg_u8.dim() == 5:
            return ob.object_scores(o, seg_u8, ob.planes_for_classes(seg_u8.shape[0], seg_u8.shape[1]), buffers)
        return ob.object_scores(o, seg_u8, ob.planes_for_binary(seg_u8.shape[0]), buffers)

    def fill_holes(self, o, **kw):
        """Fills the holes of the objects of pipe.objects' result: objects.fill_holes(o, **kw) -- max_area, connectivity,
        gt, nlabels, buffers.  Returns a result of the same form (plus `holes`), which every object stage takes."""
        from .objects import fill_holes
        return fill_holes(o, **kw)

    def object_boundaries(self, o, **kw):
        """The boundary bands of pipe.objects' result: objects.object_boundaries(o, **kw) -- d, ratio, dmax, buffers,
        metric.  Returns dict(labels, ids, d); the band of the ids goes to pipe.match_objects for per-object Boundary IoU."""
        from .objects import object_boundaries
        return object_boundaries(o, **kw)

    def object_thickness(self, o, **kw):
        """The largest inscribed circle of every object of pipe.objects' (or pipe.fill_holes') result:
        objects.object_thickness(o, **kw) -- dmax, buffers.  Returns dict(dist2, peaks, n, dmax, shape) on the device;
        objects.thickness_to_host brings radius and centre of every object to the host."""
        from .objects import object_thickness
        return object_thickness(o, **kw)

    def object_cores(self, o, radius, **kw):
        """The cores of the objects of pipe.objects' result, labelled again: objects.object_cores(o, radius, **kw)."""
        from .objects import object_cores
        return object_cores(o, radius, **kw)

    def split_objects(self, o, radius, **kw):
        """Touching objects of pipe.objects' (or pipe.fill_holes') result as separate instances: objects.split_objects(o,
        radius, **kw) -- reach, passes, min_area, buffers, connectivity.  Returns a label_objects result, which every later
        stage takes, with parent, cores and nearest."""
        from .objects import split_objects
        return split_objects(o, radius, **kw)

    def boundary_counts(self, result, gt, nlabels, key="labels", **kw):
        """Boundary IoU counts of a route's label map against a ground truth: objects.boundary_bands on
        result["native"][key] when the route ran at native size (lists, one call per item), otherwise on result[key],
        and on gt, then objects.boundary_counts.  key: "labels" for the N-way, candidate and tiled routes, "pred" for the
        binary routes, as in pipe.objects.  gt: uint8, shaped like the map (a list for a native result).  The keywords (d,
        ratio, dmax) are boundary_bands'.  Returns counts int64 [.., 2, nlabels + 1]; metrics.boundary_iou reads them."""
        from .objects import boundary_bands, boundary_counts
        src = result.get("native") or result
        if src.get(key) is None:
            raise KeyError(f"the result holds no {key!r} map (binary routes: key='pred')")
        pred = src[key]
        bp = boundary_bands(pred, **kw)
        kw["d"] = bp["d"]
        bg = boundary_bands(gt, **kw)
        return boundary_counts(bp, bg, pred, gt, nlabels)

    def _replay(self, key, step, ins):
        """HIP-graph cache of the fused step: capture once per key into static input buffers, then one
        graph launch per call (the eager path pays ~750 ctypes launches of host time per step)."""
        ent = self._graphs.get(key)
        if ent is None:
            # a host input (segment_routed's pinned route table) gets a device buffer: one H2D copy into it per call
            static_in = {k: (None if v is None else v.clone() if v.is_cuda else v.to(self.device)) for k, v in ins.items()}
            cur = torch.cuda.current_stream(self.device)
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):           # eager warm-up: allocator pools, per-batch folded rows
                step(**static_in)
            cur.wait_stream(side)
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph(keep_graph=True)   # keep the hipGraph_t for the node-type check below
            # thread_local: other host threads (the EpisodeLoader's producer allocates first-use slots and pinned
            # buffers and synchronises its copy events while this thread captures) must neither fail nor invalidate
            # the capture -- the default 'global' mode turns any hipMalloc / hipHostMalloc / event sync of ANY thread
            # into hipErrorStreamCaptureUnsupported
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                out = step(**static_in)
            self.graph_nodes = _assert_no_memset_nodes(graph)
            graph.instantiate()
            ent = (graph, static_in, out)
            self._graphs[key] = ent
        graph, static_in, out = ent
        for k, v in ins.items():
            if v is not None and v.data_ptr() != static_in[k].data_ptr():
                static_in[k].copy_(v, non_blocking=True)
        graph.replay()
        return out

    def episode_input_buffers(self, b, nshot, res, with_gt=True, r_threshold=0.25, threshold=0.0, batch_max=False):
        """Static input tensors of the captured step for this shape (after its first captured call): a
        producer (e.g. the input pipeline) may write episodes straight into them and pass them to
        run_episodes(captured=True), which then skips the staging copy."""
        for key, (_, static_in, _) in self._graphs.items():
            if key[0] == (b * nshot, 3, res, res) and key[1] == (b, 3, res, res) and key[2] == with_gt \
                    and key[3] == (float(r_threshold), float(threshold), bool(batch_max)):
                return static_in
        return None

    # ------------------------------------------------------------------ __call__ (P:223-583)
    @torch.no_grad()
    def __call__(self, input_images, denoising_steps=10, ensemble_size=10, processing_res=768,
                 match_input_res=True, batch_size=0, color_map="Spectral", show_progress_bar=True,
                 ensemble_kwargs=None, mode="depth", rgb_paths=[], seed=None):
        from PIL import Image
        if mode == "depth":
            raise NotImplementedError("only the few-shot segmentation path of DiffewS is implemented")
        if not match_input_res:
            assert processing_res is not None
        assert processing_res >= 0 and denoising_steps >= 1 and ensemble_size >= 1   # P:295-297
        if not all(torch.is_tensor(t) for t in input_images) or len(input_images) != 3:
            raise TypeError("input_images must be [support_imgs, query_img, support_masks] tensors (E:106-110)")
        sup, qry, msk = (t.to(self.device) for t in input_images)
        lo = torch.stack([t.min() for t in (sup, qry, msk)]).min()
        hi = torch.stack([t.max() for t in (sup, qry, msk)]).max()
        assert float(lo) >= -1.0 and float(hi) <= 1.0          # P:309 (one sync instead of six)
        input_size = tuple(qry.shape[-2:])                      # P:307
        bs_imgs = qry.shape[0]                                  # P:308
        s = sup.shape[0] // bs_imgs
        inner = batch_size if batch_size and batch_size > 0 else bs_imgs
        preds = []
        for i0 in range(0, bs_imgs, inner):                     # P:425-442 (explicit batch, no VRAM table)
            i1 = min(bs_imgs, i0 + inner)
            if denoising_steps == 1:
                r = self.run_episodes(sup[i0 * s:i1 * s], qry[i0:i1], msk[i0 * s:i1 * s])
                seg = (r["dec"] * 0.5 + 0.5) * 255              # P:790-795
            else:
                seg = self.single_infer(sup[i0 * s:i1 * s], qry[i0:i1], msk[i0 * s:i1 * s],
                                        num_inference_steps=denoising_steps)
            preds.append(seg)
        one = torch.cat(preds, dim=0)                           # [bs_imgs, 3, H, W]
        # the episode is deterministic (no noise is drawn, P:675), so the ensemble members are equal
        depth_preds = torch.stack([one] * ensemble_size).mean(dim=0)   # P:446, 468
        if match_input_res and tuple(depth_preds.shape[-2:]) != input_size:
            depth_preds = F.interpolate(depth_preds, input_size, mode="nearest")   # P:474
        seg_colored = depth_preds.clip(0, 255).cpu().numpy().astype(np.uint8)       # P:534
        imgs = [Image.fromarray(chw2hwc(seg_colored[i])).resize((input_size[1], input_size[0]))
                for i in range(seg_colored.shape[0])]                               # P:537-540
        return MarigoldSegOutput(seg_colored=imgs[0] if len(imgs) == 1 else imgs, uncertainty=None)


MarigoldPipeline = MarigoldPipelineRGBLatentNoise  # alias used by evaluation_util/main_oss.py:24
