"""GPU tests of the shared support bank: fsa_attention(bank_shared=True) against the same launch with the bank
materialised per query (exact), per element against the fp64 bound of tests/attention_bound.py, with the bank at the very
end of its allocation; SupportBank / prepare_bank / forward_queries against the two-pass path (exact at b = 1) and the
fp32 oracle; pipe.prepare_support / segment_queries against the oracle and run_episodes with replicated supports, reuse
of one bank, captured replays, stale handles, and the SD-2.1 / 512 x 512 shapes.

The oracle side relies on test_support_bank_cpu.test_oracle_shared_support_set_equals_replicated_supports: b queries
against one support set == the reference's batched call with the supports replicated b times."""
import pytest
import torch

import test_attention_plans_gpu as plans

pytestmark = pytest.mark.gpu

TOL_Z0 = {torch.float16: 2e-3, torch.bfloat16: 2e-2}       # tests/test_model_gpu.py TOL_Z0: one UNet pass vs the fp32 oracle
TOL_EP = {torch.float16: 3.5e-3, torch.bfloat16: 2.9e-2}   # tests/test_model_gpu.py TOL_EP: whole episode z0 vs the fp32 oracle
DTYPES = [torch.bfloat16, torch.float16]


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------ the op

@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


def _qkv(B, N, heads, dtype, g):
    """q (pre-scaled magnitudes of tests/test_attention_plans_gpu.py), k, v: column slices of one fused [B, N, 3C] buffer."""
    C = heads * 64
    buf = torch.randn(B, N, 3 * C, generator=g, device="cuda")
    buf[..., :C] *= plans.QSCALE * 2
    buf = buf.to(dtype)
    return buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:]


def _bank(s, N, heads, dtype, g):
    """[s, N, 2C] K | V buffer as prepare_bank leaves it -> (k_bank, v_bank) column views."""
    C = heads * 64
    kv = torch.randn(s, N, 2 * C, generator=g, device="cuda").to(dtype)
    return kv[..., :C], kv[..., C:]


HEADS, TOKENS, SHOTS, BATCHES = (5, 10, 20), (4096, 1024, 256, 64, 1100), (1, 2, 5), (1, 3, 4, 8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_shared_bank_equals_repeated_bank_exactly(ops, dtype):
    """fsa_attention(..., kb, vb, nshot=s, bank_shared=True) is torch.equal to the unshared launch on kb.repeat(B, 1, 1):
    same kernel, same key order, same split plan (it depends only on fields both calls share) -- only the bank image index
    differs.  heads x tokens x shots x batch as the UNet uses them (and off its grid: 1100 tokens), key split off and by
    default; the set reaches the 8-wave and 4-wave kernels, +split and +xcd plans, asserted through dfw_fsa_kernel_name."""
    from diffews_amd import _lib as L
    g = torch.Generator(device="cuda").manual_seed(11)
    reached = set()
    for heads in HEADS:
        for N in TOKENS:
            q8, k8, v8 = _qkv(max(BATCHES), N, heads, dtype, g)
            for s in SHOTS:
                kb, vb = _bank(s, N, heads, dtype, g)
                for B in BATCHES:
                    q, k, v = q8[:B], k8[:B], v8[:B]
                    kr, vr = kb.repeat(B, 1, 1), vb.repeat(B, 1, 1)
                    for key_split in (False, True):
                        with plans.fsa_names(ops, L) as names:
                            y = ops.fsa_attention(q, k, v, heads, kb, vb, nshot=s, q_prescaled=True, key_split=key_split,
                                                  bank_shared=True)
                            ref = ops.fsa_attention(q, k, v, heads, kr, vr, nshot=s, q_prescaled=True, key_split=key_split)
                        what = (heads, N, s, B, key_split)
                        assert names[0] == names[1] + "+shared", (what, names)
                        assert key_split or "+split" not in names[0], (what, names)
                        assert torch.equal(y, ref), (what, names, rel(y, ref))
                        reached.add(names[0])
                    del kr, vr
    assert any(",8,1," in n for n in reached) and any(",4,1," in n for n in reached), reached
    assert any("+split" in n for n in reached) and any("+xcd" in n for n in reached), reached
    assert any("+xcd" in n and "+split" in n for n in reached), reached


BOUND_CASES = [   # (id, B, heads, N, n_bank, s): ragged tiles, a split plan on each kernel, a bank of another length
    ("nw8_ragged_shot2", 3, 1, 1100, 1100, 2),
    ("nw8_split_shot5", 2, 2, 2048, 2048, 5),
    ("nw4_split_shot2_nbank4100", 3, 2, 256, 4100, 2),
    ("nw4_shot1_heads5", 4, 5, 200, 321, 1),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", BOUND_CASES, ids=[c[0] for c in BOUND_CASES])
def test_shared_bank_per_element_bound(ops, case, dtype):
    """Every output element and every lse of the shared launch against the fp64 reference and error allowance of
    tests/attention_bound.py, the key segments built from the shared bank (the repeated bank handed to key_segments)."""
    from diffews_amd import _lib as L
    cid, B, heads, N, nb, s = case
    g = torch.Generator(device="cuda").manual_seed(5)
    q, k, v = _qkv(B, N, heads, dtype, g)
    kb, vb = _bank(s, nb, heads, dtype, g)
    lse = torch.empty(B, heads, N, dtype=torch.float32, device="cuda")
    with plans.fsa_names(ops, L) as names:
        y = ops.fsa_attention(q, k, v, heads, kb, vb, nshot=s, q_prescaled=True, lse=lse, bank_shared=True)
    name = names[0]
    assert name.endswith("+shared")
    if "split" in cid:
        assert "+split" in name, name
    fcase = plans.Fsa(cid, B, heads, N, N, name, nshot=s, n_plain=0, n_bank=nb)
    inp = dict(q=q, k=k, v=v, kb=kb.repeat(B, 1, 1), vb=vb.repeat(B, 1, 1), lse=lse)
    w, wl = plans.fsa_check(fcase, dtype, inp, y, name.replace("+shared", ""), f"shared {cid}")
    print(f"[shared-bank] {cid} {dtype}: {name}: worst out {w:.3f}, worst lse {wl:.3f} of the allowance")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_shared_bank_at_the_end_of_its_allocation(ops, dtype):
    """The bank's buffer descriptor spans nshot images, not batch * nshot: (i) a bank that is the LAST bytes of its
    allocation, B = 4, gives the result of the repeated bank; (ii) a bank whose image stride is so large that batch * nshot
    images would pass the 2^31-byte descriptor limit (DFW_ERANGE) while nshot images do not is still accepted."""
    g = torch.Generator(device="cuda").manual_seed(3)
    B, heads, N, s = 4, 5, 1024, 2
    C = heads * 64
    q, k, v = _qkv(B, N, heads, dtype, g)
    big = torch.randn(3 * s * N * 2 * C, generator=g, device="cuda").to(dtype)
    kv = big[-s * N * 2 * C:].view(s, N, 2 * C)                  # ends exactly where the allocation ends
    assert kv.data_ptr() + kv.numel() * kv.element_size() == big.data_ptr() + big.numel() * big.element_size()
    kb, vb = kv[..., :C], kv[..., C:]
    y = ops.fsa_attention(q, k, v, heads, kb, vb, nshot=s, q_prescaled=True, bank_shared=True)
    ref = ops.fsa_attention(q, k, v, heads, kb.repeat(B, 1, 1), vb.repeat(B, 1, 1), nshot=s, q_prescaled=True)
    assert torch.equal(y, ref)
    # (ii) image stride 150 M elements: 2 images span 150 M + N * 2C elements (< 2^30), 8 would span 1.05 G (>= 2^30)
    bs = 150 * (1 << 20)
    wide = torch.empty(bs + N * 2 * C, dtype=dtype, device="cuda")
    kvw = wide.as_strided((s, N, 2 * C), (bs, 2 * C, 1))
    kvw.copy_(kv)
    y2 = ops.fsa_attention(q, k, v, heads, kvw[..., :C], kvw[..., C:], nshot=s, q_prescaled=True, bank_shared=True)
    assert torch.equal(y2, ref)


# ------------------------------------------------------------------------------------------------ UNet and pipeline

def _kw(cfg):
    return {k: v for k, v in cfg.items() if not k.startswith("_")}


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def models(request, hip_lib):
    """The tiny-config engine + fp32 oracle pair of tests/test_model_gpu.py (same seeds, weights rounded to the dtype)."""
    from diffews_amd import config, weights
    from diffews_amd.unet import MyUNet2DConditionModel
    from diffews_amd.vae import AutoencoderKL
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise
    from diffews_amd.scheduler import DDIMSchedulerCustomized
    from oracle.unet import OracleUNet
    from oracle.vae import OracleVAE
    dt = request.param
    ucfg, vcfg = config.get("tiny_unet"), config.get("tiny_vae")
    usd = weights.synthetic_unet_state_dict(ucfg, round_to=dt)
    vsd = weights.synthetic_vae_state_dict(vcfg, round_to=dt)
    te = weights.synthetic_text_embed(ucfg).to(dt).float()
    ou = OracleUNet(**_kw(ucfg)); ou.load_state_dict(usd); ou.eval()
    ov = OracleVAE(**_kw(vcfg)); ov.load_state_dict(vsd); ov.eval()
    unet = MyUNet2DConditionModel(ucfg, usd, torch_dtype=dt)
    vae = AutoencoderKL(vcfg, vsd, torch_dtype=dt)
    sched = DDIMSchedulerCustomized(**_kw(config.get("scheduler")))
    pipe = MarigoldPipelineRGBLatentNoise(unet, vae, sched, text_embeds=te)
    return dict(dt=dt, ou=ou, ov=ov, unet=unet, vae=vae, pipe=pipe, te=te, ucfg=ucfg)


def _support_set(s, H, seed):
    """One support set: images and 3-channel masks in [-1, 1] (the mask recipe of tests/test_model_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    sup = torch.rand(s, 3, H, H, generator=g) * 2 - 1
    m = torch.zeros(s, 1, H, H)
    m[:, :, H // 4:3 * H // 4, H // 4:3 * H // 4] = 1
    m = (m + (torch.rand(s, 1, H, H, generator=g) < 0.02).float()) % 2
    return sup, m.repeat(1, 3, 1, 1) * 2 - 1


def _queries(b, H, seed):
    return torch.rand(b, 3, H, H, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _rep(t, b):
    return t.repeat(b, *([1] * (t.dim() - 1)))


def test_forward_queries_equals_two_pass_at_b1(models):
    """prepare_bank + forward_queries with ONE query launch exactly what the two-pass path launches (the bank copy aside):
    torch.equal to unet(zr, is_target=False) then unet(zq), with the prompt passed and with the folded conditioning; the
    module's own bank is neither used nor touched."""
    unet, te, dt = models["unet"], models["te"], models["dt"]
    g = torch.Generator().manual_seed(13)
    ted = te.cuda()
    unet.fold_conditioning(1, te)
    for s, hw in ((1, 16), (2, 16), (3, 8)):
        zr = (torch.randn(s, 8, hw, hw, generator=g) * 0.5).cuda()
        zq = (torch.randn(1, 4, hw, hw, generator=g) * 0.5).cuda()
        for prompt, ehs_r, ehs in ((ted, ted.repeat(s, 1, 1), ted), (None, None, None)):
            unet.clear_attn_bank()
            unet(zr, 1, ehs_r, is_target=False)
            two = unet(zq, 1, ehs).sample
            unet.clear_attn_bank()
            bank = unet.prepare_bank(zr, 1, prompt)
            assert all(t.k_bank is None and t.v_bank is None for t in unet._transformers())
            assert bank.nshot == s and bank.hw == (hw, hw) and bank.dtype == dt
            one = unet.forward_queries(zq, 1, bank, prompt)
            assert one.dtype == torch.float32 and torch.equal(one, two), (s, hw, prompt is None, rel(one, two))
            assert all(t.k_bank is None for t in unet._transformers())
    # a bank is bound to its conditioning, latent size and weights
    with pytest.raises(ValueError, match="fold key"):
        unet.forward_queries(zq, 1, bank, ted)            # prepared folded, used with an explicit prompt
    with pytest.raises(ValueError, match=r"\(h, w\)"):
        unet.forward_queries(torch.zeros(1, 4, 16, 16).cuda(), 1, bank)


def test_forward_queries_vs_oracle(models):
    """b = 3 queries, one s = 2 support set: forward_queries against the fp32 oracle's two-pass graph with the supports
    replicated; bound = TOL_Z0 of tests/test_model_gpu.py (one UNet pass)."""
    ou, unet, te, dt = models["ou"], models["unet"], models["te"], models["dt"]
    g = torch.Generator().manual_seed(17)
    b, s, hw = 3, 2, 16
    zr = torch.randn(s, 8, hw, hw, generator=g) * 0.5
    zq = torch.randn(b, 4, hw, hw, generator=g) * 0.5
    with torch.no_grad():
        ou.clear_attn_bank()
        ou(_rep(zr, b), 1, te.repeat(b * s, 1, 1), is_target=False)
        ref = ou(zq, 1, te.repeat(b, 1, 1))
        ou.clear_attn_bank()
    ted = te.cuda()
    out = unet.forward_queries(zq.cuda(), 1, unet.prepare_bank(zr.cuda(), 1, ted), ted)
    e = rel(out, ref)
    print(f"[shared-bank] forward_queries b=3 s=2 {dt}: rel L2 vs fp32 oracle {e:.3e}")
    assert out.shape == ref.shape and e < TOL_Z0[dt], e
    neg = unet.forward_queries(zq.cuda(), 1, unet.prepare_bank(zr.cuda(), 1, ted), ted, out_scale=-1.0)
    assert torch.equal(neg, -out)


@pytest.mark.parametrize("b,s", [(1, 1), (3, 1), (2, 2)])
def test_segment_queries_vs_oracle(models, b, s):
    """segment_queries(prepare_support(sup, msk), qry) at 64 x 64 against oracle.pipeline.pipeline_call with the supports
    replicated: the bounds of test_model_gpu.test_episode_vs_oracle (z0 < TOL_EP, mean |delta| of the decoded [0, 255] image
    < 1.0 fp16 / 4.0 bf16); against run_episodes with replicated supports z0 within 1.5 x TOL_EP (two independently rounded
    evaluations: the margin of test_folded_conditioning)."""
    from oracle import pipeline as op
    pipe, dt = models["pipe"], models["dt"]
    sup, msk = _support_set(s, 64, seed=30 + b + s)
    qry = _queries(b, 64, seed=40 + b + s)
    masks, ref = op.pipeline_call(models["ou"], models["ov"], [_rep(sup, b), qry, _rep(msk, b)], models["te"])
    gt = (torch.rand(b, 64, 64, generator=torch.Generator().manual_seed(1)) > 0.5).to(torch.uint8).cuda()
    bank = pipe.prepare_support(sup.cuda(), msk.cuda())
    r = pipe.segment_queries(bank, qry.cuda(), gt)
    assert bank.nshot == s and set(r) == {"z0", "dec", "seg_u8", "counts"}
    e_z0 = rel(r["z0"], ref["z0"])
    seg = (r["dec"].cpu() * 0.5 + 0.5) * 255
    d_seg = float((seg - ref["seg"]).abs().mean())
    full = pipe.run_episodes(_rep(sup, b).cuda(), qry.cuda(), _rep(msk, b).cuda(), gt)
    e_full = rel(r["z0"], full["z0"])
    print(f"[shared-bank] segment_queries b={b} s={s} {dt}: z0 vs oracle {e_z0:.3e}, decoded mean |d| {d_seg:.3f}, "
          f"z0 vs run_episodes {e_full:.3e}")
    assert e_z0 < TOL_EP[dt], e_z0
    assert d_seg < (1.0 if dt == torch.float16 else 4.0), d_seg
    assert e_full < 1.5 * TOL_EP[dt], e_full
    assert r["seg_u8"].shape == (b, 3, 64, 64) and r["seg_u8"].dtype == torch.uint8
    assert r["counts"].shape == (b, 4) and (r["counts"].sum(1) == 2 * 64 * 64).all()
    assert pipe.segment_queries(bank, qry.cuda())["counts"] is None


def test_bank_reuse_leaves_bank_and_module_state_alone(models):
    """One bank, three query batches (different sizes), then the first again: first and last results identical, every bank
    tensor unchanged, whatever ran in between (run_episodes, clear_attn_bank, a reference-style two-pass)."""
    pipe, unet, te = models["pipe"], models["unet"], models["te"]
    sup, msk = _support_set(2, 64, seed=51)
    bank = pipe.prepare_support(sup.cuda(), msk.cuda())
    before = [t.clone() for t in bank.tensors()]
    batches = [_queries(2, 64, 61).cuda(), _queries(3, 64, 62).cuda(), _queries(1, 64, 63).cuda()]
    first = {k: v.clone() for k, v in pipe.segment_queries(bank, batches[0]).items() if v is not None}
    pipe.run_episodes(_rep(sup, 2).cuda(), batches[0], _rep(msk, 2).cuda())
    pipe.segment_queries(bank, batches[1])
    unet.clear_attn_bank()
    ted = te.cuda()
    unet(torch.randn(2, 8, 8, 8).cuda(), 1, ted.repeat(2, 1, 1), is_target=False)      # fills the MODULE bank
    assert all(t.k_bank is not None for t in unet._transformers())
    pipe.segment_queries(bank, batches[2])                                             # ... which a SupportBank pass ignores
    assert all(t.k_bank is not None and t.k_bank.shape[0] == 2 for t in unet._transformers())
    unet(torch.randn(2, 4, 8, 8).cuda(), 1, ted.repeat(2, 1, 1))
    unet.clear_attn_bank()
    last = pipe.segment_queries(bank, batches[0])
    for k, v in first.items():
        assert torch.equal(v, last[k]), k
    for a, b_ in zip(before, bank.tensors()):
        assert torch.equal(a, b_)


def test_segment_queries_captured_equals_eager(models):
    """captured=True replays the same kernels: identical bits on every output, with and without ground truth, over three
    input sets; two banks of the same shape used alternately each give their own eager result (the bank is part of the graph
    key, its tensors are read in place); the captured query step has fewer nodes than the captured run_episodes step of the
    same (b, s) -- the support work is not replayed -- and no memset node (checked at capture, _assert_no_memset_nodes);
    the number of cached query graphs is bounded."""
    pipe = models["pipe"]
    pipe._graphs = {}
    b, s = 2, 2
    gt = (torch.rand(b, 64, 64, generator=torch.Generator().manual_seed(2)) > 0.5).to(torch.uint8).cuda()
    sets = [tuple(t.cuda() for t in _support_set(s, 64, seed=70 + i)) for i in range(2)]
    banks = [pipe.prepare_support(*st) for st in sets]
    for use_gt in (gt, None):
        for seed in (1, 2, 3):
            qry = _queries(b, 64, 80 + seed).cuda()
            for bank in (banks[seed % 2], banks[1 - seed % 2]):
                e = {k: (None if v is None else v.clone()) for k, v in pipe.segment_queries(bank, qry, use_gt, captured=False).items()}
                c = pipe.segment_queries(bank, qry, use_gt, captured=True)
                for k in ("z0", "dec", "seg_u8", "counts"):
                    assert (e[k] is None and c[k] is None) or torch.equal(e[k], c[k]), (seed, k, use_gt is None)
    assert len(pipe._graphs) == 4          # 2 banks x (gt, no gt), each captured once
    q_nodes = pipe.graph_nodes
    assert q_nodes > 0
    qry = _queries(b, 64, 90).cuda()
    pipe.run_episodes(_rep(sets[0][0], b), qry, _rep(sets[0][1], b), gt, captured=True)
    full_nodes = pipe.graph_nodes
    print(f"[shared-bank] captured step nodes: segment_queries {q_nodes}, run_episodes {full_nodes} (b={b}, s={s})")
    assert q_nodes < full_nodes
    # the two banks differ: neither replay can have read the other's tensors
    r0 = pipe.segment_queries(banks[0], qry, gt, captured=True)["z0"].clone()
    r1 = pipe.segment_queries(banks[1], qry, gt, captured=True)["z0"].clone()
    assert not torch.equal(r0, r1)
    # bounded cache: more banks than MAX_QUERY_GRAPHS never keep more query graphs than that, and old keys still work
    for i in range(pipe.MAX_QUERY_GRAPHS + 1):
        bk = pipe.prepare_support(*(t.cuda() for t in _support_set(s, 64, seed=100 + i)))
        pipe.segment_queries(bk, qry, captured=True)
    assert sum(1 for k in pipe._graphs if k[0] == "queries") == pipe.MAX_QUERY_GRAPHS
    assert torch.equal(pipe.segment_queries(banks[0], qry, gt, captured=True)["z0"], r0)
    pipe._graphs = {}


def test_stale_bank_raises(models):
    """A bank used after the residual-stream mode, the test timestep or the resolution changed raises ValueError (on the
    host, before anything is launched), eager and captured."""
    pipe = models["pipe"]
    sup, msk = _support_set(1, 64, seed=5)
    qry = _queries(2, 64, 6).cuda()
    bank = pipe.prepare_support(sup.cuda(), msk.cuda())
    pipe.segment_queries(bank, qry)
    try:
        pipe.set_residual_dtype(torch.float32)
        for cap in (False, True):
            with pytest.raises(ValueError, match="residual"):
                pipe.segment_queries(bank, qry, captured=cap)
        bank32 = pipe.prepare_support(sup.cuda(), msk.cuda())
        assert torch.isfinite(pipe.segment_queries(bank32, qry)["z0"]).all()
    finally:
        pipe.set_residual_dtype(None)
    with pytest.raises(ValueError, match="residual"):
        pipe.segment_queries(bank32, qry)
    pipe.segment_queries(bank, qry)                      # back in its mode: valid again
    try:
        pipe.test_timestep = 3
        with pytest.raises(ValueError, match="fold key"):
            pipe.segment_queries(bank, qry)
    finally:
        pipe.test_timestep = 1
    bank = pipe.prepare_support(sup.cuda(), msk.cuda())
    big_sup, big_msk = _support_set(1, 128, seed=5)
    bank128 = pipe.prepare_support(big_sup.cuda(), big_msk.cuda())
    with pytest.raises(ValueError, match=r"\(h, w\)"):
        pipe.segment_queries(bank128, qry)
    assert torch.isfinite(pipe.segment_queries(bank128, _queries(1, 128, 7).cuda())["z0"]).all()
    pipe.segment_queries(bank, qry)


# ------------------------------------------------------------------------------------------------ SD-2.1 size

@pytest.fixture(scope="module")
def sd21(hip_lib):
    """SD-2.1 UNet + SD VAE, bf16, seeded synthetic weights (the pipeline of tests/test_fullsize_gpu.py)."""
    from diffews_amd import config, weights
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise
    from diffews_amd.scheduler import DDIMSchedulerCustomized
    from diffews_amd.unet import MyUNet2DConditionModel
    from diffews_amd.vae import AutoencoderKL
    dt = torch.bfloat16
    ucfg, vcfg = config.get("sd21_unet"), config.get("sd_vae")
    unet = MyUNet2DConditionModel(ucfg, weights.synthetic_unet_state_dict(ucfg), torch_dtype=dt)
    vae = AutoencoderKL(vcfg, weights.synthetic_vae_state_dict(vcfg), torch_dtype=dt)
    return MarigoldPipelineRGBLatentNoise(unet, vae, DDIMSchedulerCustomized(**_kw(config.get("scheduler"))),
                                          text_embeds=weights.synthetic_text_embed(ucfg).cuda())


@pytest.mark.parametrize("b,s", [(4, 1), (2, 5)])
def test_fullsize_segment_queries_512(sd21, b, s):
    """configs[1] / configs[2] shapes (512 x 512, SD-2.1, bf16) against run_episodes with the supports replicated.  Bound on
    z0: 3e-2, the full-size bound tests/test_fullsize_gpu.py::test_fullsize_episode_512 sets for two bf16 evaluations of the
    same episode by this engine (fused path vs single_infer).  The fraction of seg_u8 values that differ is printed, not
    asserted (no existing check bounds it between two engine evaluations).
    Measured on MI355X: z0 1.38e-2 (b 4, 1-shot) / 1.42e-2 (b 2, 5-shot); 73-74 % of the uint8 values differ (the decoded
    image of random weights is noise-like, a 1 % change of z0 moves most values by a level) while the thresholded
    inter / union counts agree to 1e-4 of the pixels."""
    from diffews_amd.episodes import make_episode_batch
    st = make_episode_batch(1, s, 512, seed=70 + s, device="cuda")
    qb = make_episode_batch(b, 1, 512, seed=80 + b, device="cuda")
    sup, msk, qry, gt = st["support_imgs"], st["support_masks"], qb["query_img"], qb["query_mask"]
    bank = sd21.prepare_support(sup, msk)
    assert bank.nshot == s and bank.hw == (64, 64) and bank.nbytes() == s * 46202880
    r = sd21.segment_queries(bank, qry, gt)
    full = sd21.run_episodes(_rep(sup, b), qry, _rep(msk, b), gt)
    e = rel(r["z0"], full["z0"])
    frac = float((r["seg_u8"] != full["seg_u8"]).float().mean())
    print(f"[shared-bank] full size b={b} s={s}: z0 vs run_episodes {e:.3e}, seg_u8 values that differ {frac:.3e}, "
          f"counts {r['counts'].tolist()} vs {full['counts'].tolist()}")
    assert r["z0"].shape == (b, 4, 64, 64) and torch.isfinite(r["z0"]).all()
    assert e < 3e-2, e
    c = r["counts"].cpu()
    assert (c[:, 0] <= c[:, 2]).all() and (c[:, 1] <= c[:, 3]).all() and (c.sum(1) == 2 * 512 * 512).all()
