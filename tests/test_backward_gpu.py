"""Per-op parity of the training step's backward kernels (BASELINE configs[4]) against torch
autograd of the same op in fp32 on the same (storage-dtype-rounded) inputs.

Tolerances, relative L2: gradients that are fp32 sums of exact 16-bit products (weight / bias gradients, column
sums, loss) 2e-5; gradients stored in the storage dtype or passing through 16-bit intermediates: TOL[dtype].
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
TOL = {torch.float16: 1.5e-3, torch.bfloat16: 1.2e-2}


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


@pytest.fixture(scope="module")
def B(hip_lib):
    from diffews_amd import ops, ops_bwd
    return ops, ops_bwd


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(4096, 320, 320), (1000, 64, 1280), (8, 1280, 320), (50000, 8, 128), (333, 640, 64)])
def test_linear_wgrad(B, dtype, M, N, K):
    """dW = dY^T X (nn.Linear weight gradient): ragged M (zero-filled rows), tiny M (the time-embedding MLP, one
    row per image), N = 8 (padded conv_out channels)."""
    ops, ob = B
    dy, x = rnd((M, N), dtype, 1), rnd((M, K), dtype, 2)
    ref = dy.float().t() @ x.float()
    g = ob.gemm_tn(dy.cuda(), x.cuda())
    assert g.shape == (1, N, 1, K) and rel(g.view(N, K), ref) < 2e-5
    acc = torch.ones(1, N, 1, K, device="cuda")
    ob.gemm_tn(dy.cuda(), x.cuda(), out=acc, accumulate=True, scale=0.5)
    assert rel(acc.view(N, K), 1 + 0.5 * ref) < 2e-5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Bn,H,W,Cin,Cout,stride,ups", [(2, 16, 16, 64, 128, 1, 0), (1, 24, 40, 128, 64, 1, 0),
                                                      (2, 16, 16, 64, 64, 2, 0), (1, 8, 8, 64, 128, 1, 1),
                                                      (3, 4, 4, 128, 128, 1, 0),
                                                      (1, 12, 20, 64, 64, 2, 0), (1, 6, 10, 64, 128, 1, 1)])
def test_conv3x3_backward(B, dtype, Bn, H, W, Cin, Cout, stride, ups):
    """Weight gradient (TN GEMM over the forward's im2col addressing) and data gradient (the forward conv kernel
    on mirrored weights; stride 2 through zero-stuffing, the fused upsample through 2x2 pooling) of every conv
    form in the UNet (ResnetBlock2D convs, Downsample2D stride 2 pad 1, Upsample2D nearest-2x + conv)."""
    ops, ob = B
    from diffews_amd.packing import pack_conv3x3, pack_conv3x3_dgrad, unpack_conv3x3_grad
    x = rnd((Bn, Cin, H, W), dtype, 1)
    w = rnd((Cout, Cin, 3, 3), dtype, 2, (9 * Cin) ** -0.5)
    xr, wr = x.float().requires_grad_(), w.float().requires_grad_()
    xin = F.interpolate(xr, scale_factor=2.0, mode="nearest") if ups else xr
    if ups:
        xin.retain_grad()
    y = F.conv2d(xin, wr, None, stride=stride, padding=1)
    dy = rnd(tuple(y.shape), dtype, 3)
    y.backward(dy.float())
    Ho, Wo = y.shape[-2:]
    xh = x.permute(0, 2, 3, 1).contiguous().cuda()
    dyh = dy.permute(0, 2, 3, 1).contiguous().cuda()
    gw = ob.gemm_tn(dyh, xh, taps=9, geom=(H, W, Ho, Wo, stride, 1, ups))
    assert rel(unpack_conv3x3_grad(gw.view(Cout, 9, Cin)), wr.grad) < 2e-5
    wd = pack_conv3x3_dgrad(w).cuda()
    if stride == 2:
        dx = ops.conv3x3(ob.zero_stuff2x(dyh), wd, Cin)
    elif ups:
        dx = ob.pool2x2_sum(ops.conv3x3(dyh, wd, Cin))
    else:
        dx = ops.conv3x3(dyh, wd, Cin)
    assert dx.shape == (Bn, H, W, Cin) and rel(dx.permute(0, 3, 1, 2), xr.grad) < TOL[dtype]
    # Border rows and columns per pixel (where a swap of H and W, or the padding of the transposed conv, goes wrong): dx is
    # an fp32 sum of exact 16-bit products rounded once to the storage dtype, so |dx - ref| <= u |ref|; the upsample form
    # rounds each of the four full-resolution values before pool2x2_sum adds them, which adds u * sum |part|.  Both sides
    # accumulate n = 9 Cout terms in fp32 in their own order: 2 n 2^-24 * sum |dy| |w| covers that.
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    ref = xr.grad
    mag = ref.abs() + (4 * F.avg_pool2d(xin.grad.abs(), 2) if ups else 0)
    terms = torch.autograd.grad(F.conv2d(xin, w.float().abs(), None, stride=stride, padding=1), xr, dy.float().abs())[0]
    bound = u * mag + 2 * 9 * Cout * 2.0 ** -24 * terms
    err = (dx.permute(0, 3, 1, 2).float().cpu() - ref).abs()
    edge = torch.zeros(H, W, dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    over = (err - bound)[:, :, edge]
    print(f"[conv3x3-bwd border] {dtype} {(Bn, H, W, Cin, Cout, stride, ups)}: worst err / bound on the border "
          f"{float((err / bound)[:, :, edge].max()):.3f}")
    assert float(over.max()) <= 0, float((err / bound)[:, :, edge].max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_dgrad_and_colsum(B, dtype):
    ops, ob = B
    M, N, K = 3000, 640, 320
    dy, w = rnd((M, N), dtype, 1), rnd((N, K), dtype, 2, N ** -0.5)
    dx = ops.linear(dy.cuda(), w.t().contiguous().cuda())       # dX = dY W: the forward kernel on W^T
    assert rel(dx, dy.float() @ w.float()) < TOL[dtype]
    assert rel(ob.colsum(dy.cuda()).view(-1), dy.float().sum(0)) < 2e-5
    per_img = ob.colsum(dy.cuda(), segs=3)                      # per-image sums: d(time-embedding projection)
    assert rel(per_img, dy.float().view(3, 1000, N).sum(1)) < 2e-5
    acc = torch.full((1, N), 2.0, device="cuda")
    ob.colsum(dy.cuda(), out=acc, accumulate=True, scale=0.25)
    assert rel(acc.view(-1), 2 + 0.25 * dy.float().sum(0)) < 2e-5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("Bn,HW,C", [(2, 256, 64), (3, 100, 320), (1, 4096, 128), (2, 4, 1280)])
def test_groupnorm_backward(B, dtype, silu, Bn, HW, C):
    ops, ob = B
    G = 32
    x, dy = rnd((Bn, HW, C), dtype, 1) + 0.5, rnd((Bn, HW, C), dtype, 2)
    gamma, beta = torch.randn(C) * 0.5 + 1.0, torch.randn(C) * 0.2
    xr, gr, br = x.float().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    z = F.group_norm(xr.transpose(1, 2), G, gr, br, 1e-5).transpose(1, 2)
    (F.silu(z) if silu else z).backward(dy.float())
    y, mr = ops.groupnorm(x.cuda(), gamma.cuda(), beta.cuda(), G, 1e-5, silu=silu, return_stats=True)
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx = ob.groupnorm_bwd(x.cuda(), dy.cuda(), mr, gamma.cuda(), beta.cuda(), G, silu, dg, db)
    assert rel(dx, xr.grad) < 2 * TOL[dtype]
    # dx_add: the gradient x already has from its other consumer, summed inside the kernel (fp32, one rounding)
    prev = rnd(tuple(x.shape), dtype, 9).cuda()
    dx2 = ob.groupnorm_bwd(x.cuda(), dy.cuda(), mr, gamma.cuda(), beta.cuda(), G, silu, dx_add=prev)
    assert rel(dx2, xr.grad + prev.float().cpu()) < 2 * TOL[dtype]
    assert rel(dg, gr.grad) < 2e-3 and rel(db, br.grad) < 2e-3      # fp32 sums of fp32 terms (xhat from 16-bit x)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C", [(4096, 320), (777, 640), (64, 1280), (5, 64)])
def test_layernorm_backward(B, dtype, rows, C):
    ops, ob = B
    x, dy = rnd((rows, C), dtype, 1) + 0.3, rnd((rows, C), dtype, 2)
    gamma, beta = torch.randn(C) * 0.5 + 1.0, torch.randn(C) * 0.2
    xr, gr, br = x.float().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    F.layer_norm(xr, (C,), gr, br, 1e-5).backward(dy.float())
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx = ob.layernorm_bwd(x.cuda(), dy.cuda(), gamma.cuda(), dg, db)
    assert rel(dx, xr.grad) < TOL[dtype]
    prev = rnd(tuple(x.shape), dtype, 9).cuda()
    dg2, db2 = torch.zeros_like(dg), torch.zeros_like(db)
    dx2 = ob.layernorm_bwd(x.cuda(), dy.cuda(), gamma.cuda(), dg2, db2, dx_add=prev)
    assert rel(dx2, xr.grad + prev.float().cpu()) < TOL[dtype] and torch.equal(dg2, dg)
    assert rel(dg, gr.grad) < 1e-4 and rel(db, br.grad) < 1e-4


@pytest.mark.parametrize("dtype", DTYPES)
def test_geglu_forward_backward(B, dtype):
    """Packed-column GEGLU (packing.pack_geglu) == x * gelu(gate) of diffusers' GEGLU, forward and backward."""
    ops, ob = B
    from diffews_amd.packing import geglu_perm
    rows, H = 500, 256
    pre = rnd((rows, 2 * H), dtype, 1)                      # natural order: [value | gate]
    perm = geglu_perm(H)
    packed = pre[:, perm].contiguous()
    pr = pre.float().requires_grad_()
    a, g = pr.chunk(2, dim=-1)
    out = a * F.gelu(g)
    dout = rnd((rows, H), dtype, 2)
    out.backward(dout.float())
    ff = ob.geglu_fwd(packed.cuda())
    assert rel(ff, out) < TOL[dtype]
    dpre = ob.geglu_bwd(packed.cuda(), dout.cuda())
    assert rel(dpre, pr.grad[:, perm]) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_elementwise_and_loss(B, dtype):
    ops, ob = B
    a, b = rnd((2, 6, 10, 64), dtype, 1), rnd((2, 6, 10, 64), dtype, 2)
    assert rel(ob.add(a.cuda(), b.cuda()), a.float() + b.float()) < TOL[dtype]
    wide = rnd((2, 6, 10, 192), dtype, 3)
    assert torch.equal(ob.slice_channels(wide.cuda(), 64, 128).cpu(), wide[..., 64:192])
    z = ob.zero_stuff2x(a.cuda()).cpu()
    assert z.shape == (2, 12, 20, 64) and torch.equal(z[:, ::2, ::2], a) and float(z.float().abs().sum()) == float(a.float().abs().sum())
    big = rnd((2, 12, 20, 64), dtype, 4)
    ref = big.float().view(2, 6, 2, 10, 2, 64).sum((2, 4))
    assert rel(ob.pool2x2_sum(big.cuda()), ref) < TOL[dtype]
    lat = torch.randn(3, 4, 8, 8)
    nh = ob.nchw_to_nhwc(lat.cuda(), dtype, cp=8).cpu()
    assert nh.shape == (3, 8, 8, 8) and torch.equal(nh[..., :4], lat.permute(0, 2, 3, 1).to(dtype)) and float(nh[..., 4:].abs().sum()) == 0
    pred, tgt = torch.randn(2, 4, 16, 16), torch.randn(2, 4, 16, 16)
    pr = pred.clone().requires_grad_()
    l = F.mse_loss(pr, tgt)
    l.backward()
    loss, dpred = ob.mse_loss(pred.cuda(), tgt.cuda(), dtype, loss_scale=8.0)
    assert abs(float(loss) - float(l)) < 1e-5 * float(l)
    assert rel(dpred[..., :4].permute(0, 3, 1, 2), 8.0 * pr.grad) < TOL[dtype] and float(dpred[..., 4:].abs().sum()) == 0


def test_adamw_and_clip_match_torch(B):
    """One fused AdamW step on a flat fp32 vector == torch.optim.AdamW after clip_grad_norm_ (T:1186-1194, T:1393)."""
    ops, ob = B
    n = 100_003
    g = torch.Generator().manual_seed(0)
    p0, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    tp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([tp], lr=3e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    pc, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in (1, 2, 3):
        tp.grad = gr.clone() * step
        torch.nn.utils.clip_grad_norm_([tp], 1.0)
        opt.step()
        gc = (gr * step).cuda()
        ss = ob.sumsq(gc)
        assert abs(float(ss) - float((gr * step).pow(2).sum())) < 1e-4 * float(ss)
        ob.adamw(pc, gc, m, v, step, 3e-4, grad_sumsq=ss, max_grad_norm=1.0)
        assert rel(pc, tp.detach()) < 1e-6


def _attn_ref(qkv, heads, b, nshot):
    """fp32 autograd reference of the lock-step KV-fusion attention: image i < b*nshot (support) attends over its own
    keys; query image j over [own ; its episode's support images] (A:251-267)."""
    from diffews_amd.ops import FSA_QSCALE
    n_ref = b * nshot
    Bt, N, C3 = qkv.shape
    C = C3 // 3
    x = qkv.float().requires_grad_()
    q, k, v = x[..., :C] / FSA_QSCALE, x[..., C:2 * C], x[..., 2 * C:]          # q back to unscaled units
    sh = lambda t: t.reshape(t.shape[0], -1, heads, 64).transpose(1, 2)
    outs = []
    if n_ref:
        outs.append(F.scaled_dot_product_attention(sh(q[:n_ref]), sh(k[:n_ref]), sh(v[:n_ref])).transpose(1, 2).reshape(n_ref, N, C))
    for j in range(Bt - n_ref):
        kk, vv = k[n_ref + j:n_ref + j + 1], v[n_ref + j:n_ref + j + 1]
        if nshot:
            kk = torch.cat([kk, k[j * nshot:(j + 1) * nshot].reshape(1, nshot * N, C)], 1)
            vv = torch.cat([vv, v[j * nshot:(j + 1) * nshot].reshape(1, nshot * N, C)], 1)
        outs.append(F.scaled_dot_product_attention(sh(q[n_ref + j:n_ref + j + 1]), sh(kk), sh(vv)).transpose(1, 2).reshape(1, N, C))
    return x, torch.cat(outs, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,nshot,heads,N", [(2, 0, 1, 64), (1, 1, 2, 256), (2, 2, 1, 100), (1, 3, 2, 200), (2, 1, 5, 64),
                                             (1, 7, 2, 1100)])      # the last one takes the key-split path (fwd and dQ)
def test_fsa_attention_backward(B, dtype, b, nshot, heads, N):
    """Forward with the per-row log-sum-exp + the two flash backward kernels vs torch autograd: dq / dk / dv of the
    lock-step batch, the support images' dk / dv collecting BOTH their own pass and their episode's query pass."""
    ops, ob = B
    from diffews_amd.ops import FSA_QSCALE
    n_ref, C = b * nshot, heads * 64
    Bt = n_ref + b
    qkv = rnd((Bt, N, 3 * C), dtype, 5)
    qkv[..., :C] = (qkv[..., :C].float() * FSA_QSCALE * 2).to(dtype)      # pre-scaled q
    x, out_ref = _attn_ref(qkv, heads, b, nshot)
    dout = rnd((Bt, N, C), dtype, 6)
    out_ref.backward(dout.float())
    dref = x.grad.clone()
    dref[..., :C] = dref[..., :C] * FSA_QSCALE      # the reference's gradient is w.r.t. the PRE-SCALED q: undo -> d(unscaled)
    qg = qkv.cuda()
    q, k, v = qg[..., :C], qg[..., C:2 * C], qg[..., 2 * C:]
    lse = torch.empty(Bt, heads, N, dtype=torch.float32, device="cuda")
    if nshot:
        out = ops.fsa_attention(q, k, v, heads, k[:n_ref], v[:n_ref], nshot=nshot, n_plain=n_ref, q_prescaled=True, lse=lse)
    else:
        out = ops.fsa_attention(q, k, v, heads, q_prescaled=True, lse=lse)
    assert rel(out, out_ref) < 1.5 * TOL[dtype]
    dqkv = ob.fsa_attention_bwd(qg, out, dout.cuda(), lse, heads, nshot=nshot, n_plain=n_ref)
    want_q = dref[..., :C]          # d(unscaled projection output) = QSCALE * d(q_pre), converted above
    assert rel(dqkv[..., C:2 * C], dref[..., C:2 * C]) < 2 * TOL[dtype], "dk"
    assert rel(dqkv[..., 2 * C:], dref[..., 2 * C:]) < 2 * TOL[dtype], "dv"
    assert rel(dqkv[..., :C], want_q) < 2 * TOL[dtype], "dq"


# ------------------------------------------------------------------------------------------------ whole step
def flat_norm_ref(gref):
    return torch.sqrt(sum((v.double() ** 2).sum() for v in gref.values()))


def _train_setup(dtype, b, nshot, seed=0):
    from diffews_amd import config, weights
    from oracle.unet import OracleUNet
    ucfg = config.get("tiny_unet")
    kw = {k: v for k, v in ucfg.items() if not k.startswith("_")}
    usd = weights.synthetic_unet_state_dict(ucfg, round_to=dtype)
    ou = OracleUNet(**kw)
    ou.load_state_dict(usd)
    ou.train()
    g = torch.Generator().manual_seed(seed)
    h = 16
    z_refcat = torch.randn(b * nshot, 8, h, h, generator=g) * 0.5
    z_tag = torch.randn(b, 4, h, h, generator=g) * 0.5
    target = torch.randn(b, 4, h, h, generator=g) * 0.5
    ehs = (torch.randn(1, 77, ucfg["cross_attention_dim"], generator=g)).to(dtype).float()   # 77-token prompt (T:1368)
    return ucfg, usd, ou, z_refcat, z_tag, target, ehs


def _oracle_step(ou, z_refcat, z_tag, target, ehs, b, nshot):
    """T:1374-1384 on the oracle with autograd: support pass fills the banks (graph kept), query pass reads them."""
    ou.zero_grad()
    ou.clear_attn_bank()
    ou(z_refcat, 1, ehs.repeat(b * nshot, 1, 1), is_target=False)
    pred = ou(z_tag, 1, ehs.repeat(b, 1, 1), is_target=True)
    ou.clear_attn_bank()
    loss = F.mse_loss(pred.float(), target.float())
    loss.backward()
    return float(loss), pred.detach(), {k: p.grad.detach().clone() for k, p in ou.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dtype,b,nshot", [(torch.bfloat16, 1, 1), (torch.bfloat16, 1, 2), (torch.bfloat16, 2, 1),
                                           (torch.float16, 1, 2)])
def test_training_step_gradients_vs_oracle_autograd(hip_lib, dtype, b, nshot):
    """Whole training micro-step on the tiny UNet: lock-step forward, MSE(pred, -z_mask_tag), hand-written backward ==
    torch autograd of the oracle's two-pass graph (banks with grad), for every parameter of the diffusers layout:
    the support pass' conv_in_ref, all 16 transformer blocks (self-attention dk / dv through the bank), resnets, time
    MLP + the fused time projections, the prompt K / V projections, samplers, conv_out.  fp16 runs with a loss scale."""
    from diffews_amd.train import UNetTrainer
    ucfg, usd, ou, z_refcat, z_tag, target, ehs = _train_setup(dtype, b, nshot)
    loss_ref, pred_ref, gref = _oracle_step(ou, z_refcat, z_tag, target, ehs, b, nshot)
    tr = UNetTrainer(ucfg, usd, torch_dtype=dtype, loss_scale=1.0 if dtype == torch.bfloat16 else 1024.0)
    assert set(tr.state_dict()) == set(usd) and all(torch.equal(tr.state_dict()[k].cpu(), usd[k].float()) for k in usd)
    loss, pred = tr.forward_backward(z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
    tol = 3e-2 if dtype == torch.bfloat16 else 6e-3
    assert rel(pred, pred_ref) < tol
    assert abs(float(loss) - loss_ref) < 3 * tol * loss_ref
    g = tr.grad_dict()
    assert set(g) == set(gref), set(gref) ^ set(g)
    # every tensor close in relative L2 (bf16 activations / activation gradients: a few % per tensor), the flat
    # gradient as a whole much closer in direction
    # The tiny model's per-tensor band is wide because its tensors are tiny (16 x 16 latents, 32-128 channels: a bias gradient
    # is a sum over a few hundred 16-bit-rounded values); the five worst are printed on every run so that a wrong scale on a
    # small tensor cannot hide in the band.  At SD-2.1 size every tensor is within 2.1 % (bf16) / 0.5 % (fp16):
    # tests/test_fullsize_gpu.py::test_fullsize_training_step_against_oracle_autograd.
    gtol = 0.12 if dtype == torch.bfloat16 else 0.03
    ranked = sorted(((rel(g[k], gref[k]), k, float(gref[k].norm())) for k in gref), reverse=True)
    for e, k, n in ranked[:5]:
        print(f"[tiny-train-parity] {str(dtype):15s} b={b} {nshot}-shot worst tensor {k:64s} rel L2 {e:.3e} |g_ref| {n:.3e}")
    worst = ranked[0]
    assert worst[0] < gtol, worst[:2]
    # no tensor with a non-negligible gradient may be off by a SCALE factor: compare norms, not only directions
    total_ref = float(flat_norm_ref(gref))
    for k in gref:
        nr = float(gref[k].norm())
        if nr > 1e-3 * total_ref:
            ratio = float(g[k].float().norm().cpu()) / nr
            assert abs(ratio - 1.0) < (0.06 if dtype == torch.bfloat16 else 0.015), (k, ratio)
    flat = torch.cat([g[k].float().cpu().reshape(-1) for k in sorted(gref)])
    flat_ref = torch.cat([gref[k].reshape(-1) for k in sorted(gref)])
    cos = float(F.cosine_similarity(flat, flat_ref, dim=0))
    assert cos > (0.998 if dtype == torch.bfloat16 else 0.9999), cos
    assert rel(flat, flat_ref) < (0.06 if dtype == torch.bfloat16 else 0.012)
    # a second call accumulates (gradient accumulation, T:1323) when zero_grad=False
    tr.forward_backward(z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda(), zero_grad=False)
    g2 = tr.grad_dict()
    assert rel(g2["conv_out.weight"], 2 * g["conv_out.weight"]) < 1e-5


def test_training_loop_loss_decreases_and_matches_torch_adamw(hip_lib):
    """Five optimizer steps (clip 1.0 + AdamW + poly LR) on one tiny episode: the loss falls, and the trajectory
    follows the oracle trained by torch.optim.AdamW on the same data (bf16 forward/backward vs fp32: loose)."""
    from diffews_amd.train import UNetTrainer, poly_lr
    dtype, b, nshot = torch.bfloat16, 1, 1
    ucfg, usd, ou, z_refcat, z_tag, target, ehs = _train_setup(dtype, b, nshot, seed=3)
    tr = UNetTrainer(ucfg, usd, torch_dtype=dtype)
    tr.train()
    assert tr.module is tr and len(tr.parameters()) == 1 and tr.enable_gradient_checkpointing() is None
    opt = torch.optim.AdamW(ou.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    ours, theirs = [], []
    for step in range(5):
        lr = poly_lr(1e-4, step, 100)
        loss, _ = tr.forward_backward(z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
        tr.optimizer_step(lr, max_grad_norm=1.0)
        ours.append(float(loss))
        for gparam in opt.param_groups:
            gparam["lr"] = lr
        l, _, _ = _oracle_step(ou, z_refcat, z_tag, target, ehs, b, nshot)
        torch.nn.utils.clip_grad_norm_(ou.parameters(), 1.0)
        opt.step()
        theirs.append(l)
    assert ours[-1] < ours[0] and theirs[-1] < theirs[0]
    # AdamW's first updates are ~sign(g) * lr: 16-bit noise on near-zero gradients flips signs, so the two runs drift by
    # a few % in the loss (measured <= 6.3 %) while following the same curve
    assert all(abs(a - c) < 0.10 * c for a, c in zip(ours, theirs)), (ours, theirs)
    assert poly_lr(1e-4, 100, 100) == pytest.approx(1e-7) and poly_lr(1e-4, 5, 100, warmup_steps=10) == pytest.approx(5e-5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Bn,heads,N,Lc", [(2, 2, 256, 77), (1, 1, 100, 2), (3, 4, 64, 77), (2, 5, 1000, 130), (1, 2, 4096, 77)])
def test_attention_backward_separate_kv(B, dtype, Bn, heads, N, Lc):
    """attn2 of the training step on the MFMA path: flash forward (n_kv = 77 prompt tokens, ragged second tile) with the
    row log-sum-exp + dfw_attention_bwd (queries and keys / values in their own tensors) vs torch autograd of SDPA; K | V
    and dK | dV are column slices of wider rows, as the fused prompt-K/V buffers of all 16 layers are laid out."""
    ops, ob = B
    from diffews_amd.ops import FSA_QSCALE
    C = heads * 64
    q = (rnd((Bn, N, C), dtype, 1).float() * FSA_QSCALE * 2).to(dtype)          # pre-scaled q
    dout = rnd((Bn, N, C), dtype, 2)
    kv = rnd((Bn, Lc, 2 * C + 64), dtype, 3)
    qr, kvr = q.float().requires_grad_(), kv.float().requires_grad_()
    sh = lambda t: t.reshape(Bn, -1, heads, 64).transpose(1, 2)
    o = F.scaled_dot_product_attention(sh(qr / FSA_QSCALE * 64 ** -0.5), sh(kvr[..., :C]), sh(kvr[..., C:2 * C]),
                                       scale=1.0).transpose(1, 2).reshape(Bn, N, C)
    o.backward(dout.float())
    want_dq = qr.grad * FSA_QSCALE      # autograd's gradient is w.r.t. the pre-scaled q; the kernel returns d(unscaled)
    qg, kvg = q.cuda(), kv.cuda()
    lse = torch.empty(Bn, heads, N, dtype=torch.float32, device="cuda")
    out = ops.fsa_attention(qg, kvg[..., :C], kvg[..., C:2 * C], heads, q_prescaled=True, lse=lse)
    assert rel(out, o.detach()) < 1.5 * TOL[dtype]
    dkv = torch.zeros_like(kvg)
    dq = ob.attention_bwd(qg, kvg[..., :C], kvg[..., C:2 * C], out, dout.cuda(), lse, heads, dkv[..., :C], dkv[..., C:2 * C])
    assert rel(dq, want_dq) < 2 * TOL[dtype], "dq"
    assert rel(dkv[..., :C], kvr.grad[..., :C]) < 2 * TOL[dtype], "dk"
    assert rel(dkv[..., C:2 * C], kvr.grad[..., C:2 * C]) < 2 * TOL[dtype], "dv"
    assert float(dkv[..., 2 * C:].abs().sum()) == 0
    # the dK/dV query split (short key axis, dfw_attn_bwd_args.workspace): same numbers up to the fp32 summation order of
    # the chunks, and bit-identical from run to run (chunks are folded in order, no atomics)
    dkv1, dkv2 = torch.zeros_like(kvg), torch.zeros_like(kvg)
    ob.attention_bwd(qg, kvg[..., :C], kvg[..., C:2 * C], out, dout.cuda(), lse, heads, dkv1[..., :C], dkv1[..., C:2 * C], q_split=False)
    ob.attention_bwd(qg, kvg[..., :C], kvg[..., C:2 * C], out, dout.cuda(), lse, heads, dkv2[..., :C], dkv2[..., C:2 * C])
    assert torch.equal(dkv2, dkv) and rel(dkv1, dkv) < 0.5 * TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Bn,heads,N,Lc", [(2, 2, 256, 77), (1, 1, 100, 2), (3, 4, 64, 77)])
def test_cross_attention_backward(B, dtype, Bn, heads, N, Lc):
    """attn2 backward (77-token prompt in training, T:1368; 2 tokens at inference) vs torch autograd of SDPA; dk / dv are
    written into column slices of a wider buffer, as the fused prompt-K/V gradient of all 16 layers is laid out."""
    ops, ob = B
    C = heads * 64
    q, dout = rnd((Bn, N, C), dtype, 1), rnd((Bn, N, C), dtype, 2)
    kv = rnd((Bn, Lc, 2 * C + 64), dtype, 3)          # this layer's K | V columns inside a wider row
    qr, kvr = q.float().requires_grad_(), kv.float().requires_grad_()
    sh = lambda t: t.reshape(Bn, -1, heads, 64).transpose(1, 2)
    o = F.scaled_dot_product_attention(sh(qr), sh(kvr[..., :C]), sh(kvr[..., C:2 * C])).transpose(1, 2).reshape(Bn, N, C)
    o.backward(dout.float())
    kvg = kv.cuda()
    out = ops.cross_attention(q.cuda(), kvg[..., :C], kvg[..., C:2 * C], heads)
    assert rel(out, o.detach()) < TOL[dtype]
    dkv = torch.zeros_like(kvg)
    dq = ob.cross_attention_bwd(q.cuda(), kvg[..., :C], kvg[..., C:2 * C], dout.cuda(), heads, dkv[..., :C], dkv[..., C:2 * C])
    assert rel(dq, qr.grad) < 2 * TOL[dtype]
    assert rel(dkv[..., :2 * C], kvr.grad[..., :2 * C]) < 2 * TOL[dtype] and float(dkv[..., 2 * C:].abs().sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_relayout(B, dtype):
    """Device re-layouts of the 16-bit weights for the data-gradient GEMMs == the host packing functions."""
    ops, ob = B
    from diffews_amd.packing import pack_conv3x3, pack_conv3x3_dgrad
    w = rnd((320, 1288), dtype, 1)
    assert torch.equal(ob.linear_wt(w.cuda()).cpu(), w.t().contiguous())
    cw = rnd((128, 64, 3, 3), dtype, 2)
    assert torch.equal(ob.conv3x3_wd(pack_conv3x3(cw).cuda(), 128).cpu(), pack_conv3x3_dgrad(cw))
    cw = rnd((8, 320, 3, 3), dtype, 3)
    assert torch.equal(ob.conv3x3_wd(pack_conv3x3(cw).cuda(), 8).cpu(), pack_conv3x3_dgrad(cw))


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_relayout_batch_equals_single_launches(B, dtype):
    """The one-launch table form (every derived copy of a training step) writes the same bits as the per-weight launches,
    and re-running it after the sources changed refreshes the copies in place."""
    ops, ob = B
    ws = [rnd((320, 1280), dtype, 1).cuda(), rnd((64, 9 * 128), dtype, 2).cuda(), rnd((8, 72), dtype, 3).cuda(),
          rnd((1280, 320), dtype, 4).cuda()]
    kinds = ["T", "D", "T", "T"]
    singles = [ob.linear_wt(w) if k == "T" else ob.conv3x3_wd(w, w.shape[0]) for k, w in zip(kinds, ws)]
    ys = [torch.zeros_like(s) for s in singles]
    table = ob.relayout_table(list(zip(kinds, ws, ys)), "cuda")
    ob.weight_relayout_batch(table)
    for y, s in zip(ys, singles):
        assert torch.equal(y, s)
    for w in ws:
        w.mul_(-2)
    ob.weight_relayout_batch(table)
    for k, w, y in zip(kinds, ws, ys):
        assert torch.equal(y, ob.linear_wt(w) if k == "T" else ob.conv3x3_wd(w, w.shape[0]))


# ------------------------------------------------------------------------------------------------ launcher surface
@pytest.mark.parametrize("dtype,nshot", [(torch.bfloat16, 1), (torch.float16, 1), (torch.bfloat16, 2)])
def test_training_loop_literal_launcher_calls(hip_lib, dtype, nshot):
    """T:1374-1396 LITERALLY on UNetTrainer: two `unet(...)` calls (support with is_target=False, then query), the
    launcher's own loss expression under torch autograd, `loss.backward()`, `clip_grad_norm_(unet.parameters(), 1.0)`,
    `torch.optim.AdamW(unet.parameters()).step()`, `optimizer.zero_grad()`.  The gradient equals forward_backward's
    bit for bit (1-shot: same rounded dpred; n-shot: torch's broadcast of `pred + pred_ref * 0` sums nshot copies of
    grad / nshot, a last-ulp difference before the 16-bit rounding), and the torch optimizer's in-place update of the flat
    master is picked up by the next forward (shadow refresh through the version counter)."""
    from diffews_amd.train import UNetTrainer
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, nshot, seed=5)
    ls = 1.0 if dtype == torch.bfloat16 else 1024.0
    ref = UNetTrainer(ucfg, usd, torch_dtype=dtype, loss_scale=ls, dynamic_loss_scale=False)
    loss_ref, pred_ref = ref.forward_backward(z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
    unet = UNetTrainer(ucfg, usd, torch_dtype=dtype, loss_scale=ls, dynamic_loss_scale=False)
    unet.train()
    params = list(unet.parameters())
    assert len(params) == 1 and isinstance(params[0], torch.nn.Parameter) and params[0].grad is None
    optimizer = torch.optim.AdamW(unet.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    timesteps = torch.tensor([1]).long().repeat(1).cuda()                                    # T:1365
    ehs_c = ehs.cuda()
    ehs_nshot = ehs_c.repeat(nshot, 1, 1)                                                    # T:1369
    model_pred_cond_ref = unet(z_refcat.cuda(), timesteps, ehs_nshot, is_target=False).sample   # T:1374
    model_pred = unet(z_tag.cuda(), timesteps, ehs_c, is_target=True).sample                    # T:1375
    unet.module.clear_attn_bank() if hasattr(unet, "module") else unet.clear_attn_bank()     # T:1376-1379
    assert model_pred_cond_ref.shape == (nshot, 4, 16, 16) and model_pred_cond_ref.grad_fn is not None
    assert float(model_pred_cond_ref.abs().max()) == 0.0 and model_pred.grad_fn is not None
    assert torch.equal(model_pred.detach(), pred_ref)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # n-shot: mse_loss warns about the [s,...] vs [1,...] broadcast, as in the reference
        model_pred = model_pred.float() + model_pred_cond_ref.float() * 0.                   # T:1381
        loss = F.mse_loss(model_pred.float(), target.cuda().float(), reduction="mean")       # T:1384
    loss.backward()                                                                          # T:1391
    g = unet.parameters()[0].grad
    assert g is not None and g.data_ptr() == unet.P.grad.data_ptr()
    assert abs(float(loss) - float(loss_ref)) < 1e-6 * max(1.0, abs(float(loss_ref)))
    if nshot == 1:
        assert torch.equal(g, ref.P.grad)
    else:
        assert rel(g, ref.P.grad) < 1e-3
    torch.nn.utils.clip_grad_norm_(unet.parameters(), 1.0)                                   # T:1393
    before = unet.P.master.clone()
    optimizer.step()                                                                         # T:1394
    optimizer.zero_grad()                                                                    # T:1396
    assert unet.parameters()[0].grad is None and not torch.equal(before, unet.P.master)
    # the next forward sees the updated weights: its prediction == a fresh trainer built from the updated state_dict
    pred2 = unet(z_tag.cuda(), timesteps, ehs_c, is_target=True).sample.detach()            # 0-shot call form also works
    fresh = UNetTrainer(ucfg, {k: v.cpu() for k, v in unet.state_dict().items()}, torch_dtype=dtype, loss_scale=ls)
    c = fresh._forward(z_tag.new_zeros(0, 8, 16, 16).cuda(), z_tag.cuda(), 1, ehs_c)
    assert torch.equal(pred2, c["pred"])


def test_optimizer_skips_overflow_and_halves_the_loss_scale(hip_lib):
    """fp16 with a dynamic loss scale (accelerate mixed_precision='fp16', T:1017): one inf in the gradient must leave
    master, both moments and the 16-bit shadow untouched (GradScaler's skipped step), halve the scale and not count as a
    step; the following clean step updates as usual."""
    from diffews_amd.train import UNetTrainer
    dtype = torch.float16
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, 1, seed=7)
    tr = UNetTrainer(ucfg, usd, torch_dtype=dtype, loss_scale=1024.0)
    assert tr.dynamic_loss_scale
    args = (z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
    tr.forward_backward(*args)
    tr.optimizer_step(1e-4)
    snap = [t.clone() for t in (tr.P.master, tr.P.exp_avg, tr.P.exp_avg_sq, tr.P.shadow)]
    tr.forward_backward(*args)
    tr.P.grad[12345] = float("inf")
    tr.optimizer_step(1e-4)
    torch.cuda.synchronize()
    for a, b_ in zip(snap, (tr.P.master, tr.P.exp_avg, tr.P.exp_avg_sq, tr.P.shadow)):
        assert torch.equal(a, b_)
    tr.forward_backward(*args)                       # resolves the flag: scale halves, the skipped step is not counted
    assert tr.loss_scale == 512.0 and tr.skipped_steps == 1 and tr.step_count == 1
    tr.optimizer_step(1e-4)
    torch.cuda.synchronize()
    assert not torch.equal(snap[0], tr.P.master) and torch.isfinite(tr.P.master).all()
    tr._resolve_overflow()
    assert tr.step_count == 2 and tr.skipped_steps == 1
    # NaN gradient in bf16 (fixed scale): skipped as well
    tb = UNetTrainer(ucfg, usd, torch_dtype=torch.bfloat16)
    tb.forward_backward(*args)
    m0 = tb.P.master.clone()
    tb.P.grad[7] = float("nan")
    tb.optimizer_step(1e-4)
    tb._resolve_overflow()
    assert torch.equal(m0, tb.P.master) and tb.skipped_steps == 1 and tb.step_count == 0 and tb.loss_scale == 1.0


def test_step_guard_skips_an_overflowed_fp16_step_on_the_autograd_surface(hip_lib):
    """INTEGRATION.md path (a) under fp16: `loss.backward()` -> `unet.step_guard()` -> clip + `torch.optim` step.  A huge
    loss scale overflows the fp16 backward: the guard reports it, zeroes the gradient and halves the scale; the launcher
    skips `optimizer.step()` and the fp32 master stays finite and unchanged.  The next (clean) step passes the guard."""
    import torch.nn.functional as F
    from diffews_amd.train import UNetTrainer
    dtype = torch.float16
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, 1, seed=17)
    unet = UNetTrainer(ucfg, usd, torch_dtype=dtype, loss_scale=65536.0 * 65536.0)
    optimizer = torch.optim.AdamW(unet.parameters(), lr=1e-4)
    ts = torch.tensor([1]).long().cuda()

    def launcher_step():
        pr = unet(z_refcat.cuda(), ts, ehs.cuda(), is_target=False).sample
        pq = unet(z_tag.cuda(), ts, ehs.cuda(), is_target=True).sample
        loss = F.mse_loss(pq.float() + pr.float() * 0., target.cuda().float(), reduction="mean")
        loss.backward()
        took = unet.step_guard()
        if took:
            torch.nn.utils.clip_grad_norm_(unet.parameters(), 1.0)
            optimizer.step()
        optimizer.zero_grad()
        return took
    m0 = unet.P.master.clone()
    assert launcher_step() is False
    assert unet.loss_scale == 65536.0 * 32768.0 and unet.skipped_steps == 1 and torch.equal(unet.P.master, m0)
    unet.loss_scale = 1024.0
    assert launcher_step() is True
    assert torch.isfinite(unet.P.master).all() and not torch.equal(unet.P.master, m0)


def test_trainer_state_resume_is_bit_exact(hip_lib, tmp_path):
    """save_state / load_state (accelerator.save_state / load_state, T:1281-1309, T:1407-1431): weights in the diffusers
    layout + optimizer state; a trainer rebuilt from the checkpoint continues the SAME trajectory bit for bit."""
    from diffews_amd import weights
    from diffews_amd.train import UNetTrainer, poly_lr
    dtype = torch.bfloat16
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, 1, seed=9)
    args = (z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
    a = UNetTrainer(ucfg, usd, torch_dtype=dtype)
    for step in range(2):
        a.forward_backward(*args)
        a.optimizer_step(poly_lr(1e-4, step, 100))
    ck = str(tmp_path / "checkpoint-2")
    a.save_state(ck)
    b = UNetTrainer(weights.load_config(ck, "unet"), weights.load_state_dict(ck, "unet"), torch_dtype=dtype)
    b.load_state(ck)
    assert b.step_count == 2 and torch.equal(a.P.master, b.P.master) and torch.equal(a.P.shadow, b.P.shadow)
    for step in range(2, 4):
        la, _ = a.forward_backward(*args)
        a.optimizer_step(poly_lr(1e-4, step, 100))
        lb, _ = b.forward_backward(*args)
        b.optimizer_step(poly_lr(1e-4, step, 100))
        assert torch.equal(la, lb)
    assert torch.equal(a.P.master, b.P.master) and torch.equal(a.P.exp_avg_sq, b.P.exp_avg_sq)
    with pytest.raises(ValueError):
        sd = a.optimizer_state_dict()
        sd["layout"] = "other"
        b.load_optimizer_state_dict(sd)


def test_gradient_buckets_are_reduced_after_their_last_writer(hip_lib):
    """Overlapped gradient all-reduce (GradBucketReducer): every bucket's collective must see the FINAL gradients of the
    bucket.  The injected 'collective' snapshots the bucket on the comm stream; after the step the snapshots equal the
    final flat gradient bit for bit (a bucket fired before its last writer would hold stale or partial values), all
    buckets fired from the end of the buffer towards its start, and the loss rode in the last range's tail slot."""
    from diffews_amd.train import UNetTrainer, GradBucketReducer, ParamStore
    dtype = torch.bfloat16
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, 2, seed=11)
    tr = UNetTrainer(ucfg, usd, torch_dtype=dtype)
    args = (z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
    tr.forward_backward(*args)                       # warm-up (lazy derived weights)
    for name in tr.P.spec:                           # poison every parameter's gradient: a too-early snapshot would hold NaNs
        tr.P.g(name).fill_(float("nan"))             # (the 64-float alignment pads between entries stay zero, as always)
    snaps = {}
    spec = {k: (off, max(1, int(torch.tensor(shape).prod()))) for k, (off, shape) in tr.P.spec.items()}
    red = GradBucketReducer(tr.P.grad_buf, spec, bucket_elems=1 << 21, world_size=2,
                            collective=lambda t: snaps.__setitem__(t.data_ptr(), t.clone()))
    nb = len(red.ranges)
    assert nb >= 8
    loss, _ = tr.forward_backward(*args, reducer=red)
    avg = red.finish()
    torch.cuda.synchronize()
    assert sorted(red.fired_order) == list(range(nb))
    # the layout is forward-ordered: the backward completes buckets from the end towards the start (the first buckets hold
    # the conditioning parameters, whose gradients are the last to be written)
    assert red.fired_order[0] == nb - 1 and red.fired_order[-1] in (0, 1)
    assert sum(1 for a, b_ in zip(red.fired_order, red.fired_order[1:]) if b_ > a) <= 2
    base = tr.P.grad_buf.data_ptr()
    final = tr.P.grad_buf * 2.0                      # the fp32 path multiplied each bucket by 1 / world AFTER the snapshot
    for (s0, s1) in red.ranges:
        snap = snaps[base + 4 * s0]
        n = min(s1, tr.P.numel) - s0
        assert torch.isfinite(snap[:n]).all()
        assert torch.equal(snap[:n], final[s0:s0 + n])
    assert float(avg) == pytest.approx(float(loss) * 0.5)     # "sum" over one rank, times 1 / world
    assert ParamStore.TAIL >= 1


def test_autograd_surface_reduces_every_bucket_with_attached_reducer(hip_lib):
    """`trainer.reducer = trainer.make_reducer(...)` + the launcher's own `unet(...)` / `loss.backward()` (T:1374-1391): the
    backward of the query pass must BEGIN the reducer, so that every gradient bucket goes through the collective during the
    tape walk (round-3 defect: nothing called begin(), mark() returned silently and each rank kept its local gradient).
    Injected collective = x2 (a 2-rank SUM of equal gradients): after finish() the flat gradient, averaged by 1 / world,
    equals the unreduced one bit for bit and every bucket fired; a reducer that was never begun refuses to finish()."""
    import torch.nn.functional as F
    from diffews_amd.train import UNetTrainer
    dtype = torch.bfloat16
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, 2, seed=21)
    ref = UNetTrainer(ucfg, usd, torch_dtype=dtype)
    ref.forward_backward(z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
    unet = UNetTrainer(ucfg, usd, torch_dtype=dtype)
    calls = []

    def fake_sum(t):
        calls.append(t.numel())
        t.mul_(2.0)
    red = unet.make_reducer(bucket_elems=1 << 21, world_size=2, collective=fake_sum)
    unet.reducer = red
    with pytest.raises(RuntimeError):
        red.finish()                                  # nothing begun yet
    ts = torch.tensor([1]).long().cuda()
    ehs_c = ehs.cuda()
    pred_ref = unet(z_refcat.cuda(), ts, ehs_c.repeat(2, 1, 1), is_target=False).sample
    pred = unet(z_tag.cuda(), ts, ehs_c, is_target=True).sample
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = F.mse_loss(pred.float() + pred_ref.float() * 0., target.cuda().float(), reduction="mean")
    loss.backward()
    assert red.steps_begun == 1 and red.active
    red.finish()
    torch.cuda.synchronize()
    nb = len(red.ranges)
    assert nb >= 8 and sorted(red.fired_order) == list(range(nb)) and len(calls) == nb
    g = unet.parameters()[0].grad
    assert rel(g, ref.P.grad) < 1e-3 and torch.isfinite(g).all()     # (x2, then x1/2: exact in fp32)
    with pytest.raises(RuntimeError):
        red.mark(["conv_out.weight"])                 # a walk that reports to a reducer nobody began


def test_segmented_training_step_equals_eager_overlapped(hip_lib):
    """forward_backward_segmented (multi-GPU form of the captured step, round 4): forward + backward as a CHAIN of HIP graphs cut
    where a gradient bucket becomes final, the reducer firing between segments == the eager overlapped step bit for bit -- loss,
    prediction, the whole reduced flat gradient, the firing order -- over optimizer steps and new inputs; every bucket's collective
    sees its final values (the injected collective doubles what it is given: a 2-rank SUM of equal gradients); no memset node."""
    from diffews_amd.train import UNetTrainer
    dtype = torch.bfloat16
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, 2, seed=23)
    a = UNetTrainer(ucfg, usd, torch_dtype=dtype)
    b = UNetTrainer(ucfg, usd, torch_dtype=dtype)
    ra = a.make_reducer(bucket_elems=1 << 21, world_size=2, collective=lambda t: t.mul_(2.0))
    rb = b.make_reducer(bucket_elems=1 << 21, world_size=2, collective=lambda t: t.mul_(2.0))
    nb = len(ra.ranges)
    assert nb >= 8
    for step in range(3):
        zr, zt, tg = z_refcat.cuda() * (1 + 0.1 * step), z_tag.cuda() + 0.01 * step, target.cuda()
        la, pa = a.forward_backward(zr, zt, tg, 1, ehs.cuda(), reducer=ra)
        la = ra.finish().clone()
        order_a = list(ra.fired_order)
        lb, pb = b.forward_backward_segmented(zr, zt, tg, 1, ehs.cuda(), rb)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb) and torch.equal(la, lb), step
        assert torch.equal(a.P.grad, b.P.grad), step
        assert list(rb.fired_order) == order_a and sorted(order_a) == list(range(nb)), step
        a.optimizer_step(1e-4)
        b.optimizer_step(1e-4)
        assert torch.equal(a.P.master, b.P.master)
    key = [k for k in b._graphs if k[0] == "segmented"]
    assert len(key) == 1 and 2 <= len(b._graphs[key[0]][0]) <= nb + 1 and b.graph_nodes > 500


def test_captured_training_step_equals_eager(hip_lib):
    """forward_backward_captured: fwd + bwd replayed as one HIP graph == the eager step bit for bit (loss, pred, the whole
    flat gradient), over optimizer steps in between (the derived weight copies are refreshed inside the graph) and with new
    inputs per step; the capture holds no memset node."""
    from diffews_amd.train import UNetTrainer
    dtype = torch.bfloat16
    ucfg, usd, _, z_refcat, z_tag, target, ehs = _train_setup(dtype, 1, 2, seed=13)
    a = UNetTrainer(ucfg, usd, torch_dtype=dtype)
    b = UNetTrainer(ucfg, usd, torch_dtype=dtype)
    for step in range(3):
        zr, zt, tg = z_refcat.cuda() * (1 + 0.1 * step), z_tag.cuda() + 0.01 * step, target.cuda()
        la, pa = a.forward_backward(zr, zt, tg, 1, ehs.cuda())
        lb, pb = b.forward_backward_captured(zr, zt, tg, 1, ehs.cuda())
        assert torch.equal(la, lb) and torch.equal(pa, pb), step
        assert torch.equal(a.P.grad, b.P.grad), step
        a.optimizer_step(1e-4)
        b.optimizer_step(1e-4)
        assert torch.equal(a.P.master, b.P.master)
    assert len(b._graphs) == 1 and b.graph_nodes > 500
    # a loss-scale change (dynamic scale: every overflow halves it) must REPLACE the captured step, not add a second graph
    # with its own activation pool; the re-captured step is again the eager step bit for bit
    for scale in (4.0, 2.0, 4.0):
        a.loss_scale = b.loss_scale = scale
        la, pa = a.forward_backward(z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
        lb, pb = b.forward_backward_captured(z_refcat.cuda(), z_tag.cuda(), target.cuda(), 1, ehs.cuda())
        assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(a.P.grad, b.P.grad), scale
        assert len(b._graphs) == 1
    assert b.graph_recaptures == 3
