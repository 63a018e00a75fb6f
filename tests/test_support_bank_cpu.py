"""CPU tests (no GPU) of the shared support bank: the `bank_shared` field of dfw_fsa_args through the host-only queries
(validation, kernel name, workspace), the SupportBank handle's validation on host tensors, and -- with the oracle -- the
equivalence the GPU tests of tests/test_support_bank_gpu.py rely on: a batch of queries against ONE support set is, per
query, the reference's two-pass graph, and equals the reference's batched call with the supports replicated."""
import ctypes as C

import pytest
import torch

DFW_EINVAL = -1


def _fsa_args(L, dtype=None, pre=1, **kw):
    a = L.FsaArgs()
    a.q = a.k = a.v = a.out = a.k_bank = a.v_bank = 4096      # never dereferenced: host-side queries only
    a.dtype, a.q_prescaled = L.BF16 if dtype is None else dtype, pre
    for key, val in kw.items():
        setattr(a, key, val)
    a.ldq = a.ldk = a.ldv = a.ldo = a.ldkb = a.ldvb = a.heads * 64
    return a


def _name(L, a):
    buf = C.create_string_buffer(96)
    L.check(L.lib().dfw_fsa_kernel_name(C.byref(a), buf, 96), "dfw_fsa_kernel_name")
    return buf.value.decode()


def _with_workspace(L, a):
    nb = L.lib().dfw_fsa_workspace_bytes(C.byref(a))
    if nb:
        a.workspace, a.workspace_bytes = 4096, nb
    return a


def test_header_and_ctypes_agree_on_bank_shared():
    """The field exists on both sides and is the LAST one (a library built before the field reads a prefix of the struct:
    the DFW_LIB A/B of two builds stays possible).  Names / order / sizeof are test_host_cpu's layout tests."""
    import os
    import re
    from diffews_amd import _lib as L
    assert L.FsaArgs._fields_[-1] == ("bank_shared", C.c_int32)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffews_hip.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\}\s*dfw_fsa_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert body.split(";")[-2].split() == ["int32_t", "bank_shared"]


def test_shared_bank_argument_validation(hip_lib):
    """dfw_fsa_attention validates on the host before any launch (safe without a GPU): bank_shared outside {0, 1}, a
    shared bank with no shots, and a shared bank next to plain entries (a shared launch is a query-only launch: rejected)
    are DFW_EINVAL; so say the plan queries."""
    from diffews_amd import _lib as L
    h = L.lib()
    ok = dict(batch=3, heads=2, n_q=128, n_kv=128, n_bank=128, nshot=2)
    for bad in (dict(ok, bank_shared=1, nshot=0, n_bank=0), dict(ok, bank_shared=2), dict(ok, bank_shared=-1),
                dict(ok, bank_shared=1, n_plain=1), dict(batch=3, heads=2, n_q=128, n_kv=128, bank_shared=1)):
        a = _fsa_args(L, **bad)
        assert h.dfw_fsa_attention(C.byref(a), None) == DFW_EINVAL, bad
        buf = C.create_string_buffer(96)
        assert h.dfw_fsa_kernel_name(C.byref(a), buf, 96) == DFW_EINVAL, bad
    a = _fsa_args(L, **dict(ok, bank_shared=1))
    assert "+shared" in _name(L, a)
    with pytest.raises(ValueError, match=r"fsa_attention: k_bank must hold 1 images \(nshot, one shared set\), got 3"):     # ops: the bank of a shared launch holds exactly nshot images
        from diffews_amd import ops
        q = torch.zeros(3, 128, 128, dtype=torch.bfloat16)
        ops.fsa_attention(q, q, q, 2, q, q, nshot=1, bank_shared=True)


# dfw_fsa_kernel_name of the commit BEFORE the bank_shared field, recorded from that build: key = (dtype code, q_prescaled,
# batch, heads, n_q = n_kv = n_bank, nshot, n_plain, workspace passed).  Lock-step launches of configs[1] (b 4, 1 shot) and
# configs[2] (b 2, 5 shots) at the four UNet levels (64^2 x 5 heads ... 8^2 x 20 heads), the two-pass read launches
# (n_plain = 0) of the same, with and without the key-split workspace, plus the launch-rule corner cases.
PARENT_NAMES = {
    (0, 1, 8, 5, 4096, 1, 4, 0): "fsa_ring_kernel<bf16,8,1,pre>+xcd",
    (0, 1, 4, 5, 4096, 1, 0, 0): "fsa_ring_kernel<bf16,8,1,pre>",
    (0, 1, 8, 5, 4096, 1, 4, 1): "fsa_ring_kernel<bf16,8,1,pre>+xcd",
    (0, 1, 4, 5, 4096, 1, 0, 1): "fsa_ring_kernel<bf16,8,1,pre>",
    (0, 1, 8, 10, 1024, 1, 4, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 4, 10, 1024, 1, 0, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 8, 10, 1024, 1, 4, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 4, 10, 1024, 1, 0, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 8, 20, 256, 1, 4, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 4, 20, 256, 1, 0, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 8, 20, 256, 1, 4, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 4, 20, 256, 1, 0, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 8, 20, 64, 1, 4, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 4, 20, 64, 1, 0, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 8, 20, 64, 1, 4, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 4, 20, 64, 1, 0, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 12, 5, 4096, 5, 10, 0): "fsa_ring_kernel<bf16,8,1,pre>",
    (0, 1, 2, 5, 4096, 5, 0, 0): "fsa_ring_kernel<bf16,8,1,pre>",
    (0, 1, 12, 5, 4096, 5, 10, 1): "fsa_ring_kernel<bf16,8,1,pre>+split2",
    (0, 1, 2, 5, 4096, 5, 0, 1): "fsa_ring_kernel<bf16,8,1,pre>+split3",
    (0, 1, 12, 10, 1024, 5, 10, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 2, 10, 1024, 5, 0, 0): "fsa_ring_kernel<bf16,4,1,pre>",
    (0, 1, 12, 10, 1024, 5, 10, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 2, 10, 1024, 5, 0, 1): "fsa_ring_kernel<bf16,4,1,pre>",
    (0, 1, 12, 20, 256, 5, 10, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 2, 20, 256, 5, 0, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 12, 20, 256, 5, 10, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 2, 20, 256, 5, 0, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 12, 20, 64, 5, 10, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 2, 20, 64, 5, 0, 0): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 12, 20, 64, 5, 10, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 1, 2, 20, 64, 5, 0, 1): "fsa_ring_kernel<bf16,4,1,pre>+xcd",
    (0, 0, 1, 1, 1025, 0, 0, 0): "fsa_ring_kernel<bf16,8,1,scale>",
    (0, 1, 8, 2, 1024, 7, 7, 1): "fsa_ring_kernel<bf16,4,1,pre>+split8",
}


def _args_of(L, key):
    dtype, pre, batch, heads, n, nshot, n_plain, ws = key
    a = _fsa_args(L, dtype=dtype, pre=pre, batch=batch, heads=heads, n_q=n, n_kv=n, n_bank=n if nshot else 0, nshot=nshot,
                  n_plain=n_plain)
    return _with_workspace(L, a) if ws else a


def test_unshared_kernel_names_are_unchanged(hip_lib):
    """Unshared arguments plan and NAME exactly what they did before the field existed (both dtypes: the f16 names are the
    bf16 ones with the type swapped, as recorded from the same build)."""
    from diffews_amd import _lib as L
    for key, want in PARENT_NAMES.items():
        assert _name(L, _args_of(L, key)) == want, key
        f16 = (L.F16,) + key[1:]
        assert _name(L, _args_of(L, f16)) == want.replace("<bf16,", "<f16,"), f16


def test_shared_kernel_name_and_workspace(hip_lib):
    """A shared launch is the two-pass read launch (n_plain = 0) of the same batch / nshot / n_q / heads with another bank
    index: same kernel, same split count, same partial buffer (still per query image) -- its name is that launch's name
    plus '+shared', its workspace that launch's workspace."""
    from diffews_amd import _lib as L
    seen = set()
    for key, want in PARENT_NAMES.items():
        dtype, pre, batch, heads, n, nshot, n_plain, ws = key
        if n_plain or not nshot:
            continue
        a, s = _args_of(L, key), _args_of(L, key)
        s.bank_shared = 1
        assert L.lib().dfw_fsa_workspace_bytes(C.byref(s)) == L.lib().dfw_fsa_workspace_bytes(C.byref(a)), key
        if ws:
            s.workspace_bytes = L.lib().dfw_fsa_workspace_bytes(C.byref(s))
        name = _name(L, s)
        assert name == want + "+shared", key
        seen.add(name)
    assert any("+split" in n for n in seen) and any("+xcd" in n for n in seen)
    assert any(",8,1," in n for n in seen) and any(",4,1," in n for n in seen)
    # 5 shots at the 64^2 level really take a workspace (the split count is that of the unshared launch)
    a = _args_of(L, (0, 1, 2, 5, 4096, 5, 0, 0))
    a.bank_shared = 1
    assert L.lib().dfw_fsa_workspace_bytes(C.byref(a)) == 2 * 3 * 5 * 4096 * 68 * 4


def test_oracle_shared_support_set_equals_replicated_supports():
    """The definition of the feature, in the reference's own arithmetic (fp32 oracle, tiny config): b = 3 queries against
    ONE s = 2 support set, each run through the two-pass graph alone (batch 1), give the z0 of ONE call with the supports
    replicated to b * s (support image of episode e, shot j = j-th image of the set)."""
    from diffews_amd import config, weights
    from oracle import pipeline as op
    from oracle.unet import OracleUNet
    from oracle.vae import OracleVAE
    kw = lambda c: {k: v for k, v in c.items() if not k.startswith("_")}
    ucfg, vcfg = config.get("tiny_unet"), config.get("tiny_vae")
    ou = OracleUNet(**kw(ucfg)); ou.load_state_dict(weights.synthetic_unet_state_dict(ucfg)); ou.eval()
    ov = OracleVAE(**kw(vcfg)); ov.load_state_dict(weights.synthetic_vae_state_dict(vcfg)); ov.eval()
    te = weights.synthetic_text_embed(ucfg).float()
    g = torch.Generator().manual_seed(7)
    b, s, H = 3, 2, 64
    sup = torch.rand(s, 3, H, H, generator=g) * 2 - 1
    msk = (torch.rand(s, 1, H, H, generator=g) > 0.5).float().repeat(1, 3, 1, 1) * 2 - 1
    qry = torch.rand(b, 3, H, H, generator=g) * 2 - 1
    rep = op.single_infer(ou, ov, sup.repeat(b, 1, 1, 1), qry, msk.repeat(b, 1, 1, 1), te)["z0"]
    one = torch.cat([op.single_infer(ou, ov, sup, qry[i:i + 1], msk, te)["z0"] for i in range(b)])
    assert rep.dtype == torch.float32 and rep.shape == one.shape
    assert torch.allclose(one, rep, rtol=1e-5, atol=1e-5 * float(rep.abs().max()))


def test_support_bank_handle_validation():
    """SupportBank validates what it is given, on host tensors: wrong (h, w), dtype or nshot raise ValueError naming the
    mismatch; a consistent handle is immutable and reports the K/V bytes it owns; check() names what no longer matches."""
    from diffews_amd import config
    from diffews_amd.unet import SupportBank, bank_layout
    cfg = config.get("tiny_unet")
    dt, s, hw = torch.bfloat16, 2, (8, 8)
    layout = bank_layout(cfg, *hw)

    def kv(layout, nshot=s, dtype=dt):
        return [torch.zeros(nshot, n, c, dtype=dtype) for n, c in layout]

    def make(k, v, nshot=s, hw=hw, dtype=dt):
        return SupportBank(k, v, nshot, hw, dtype, dtype, (1.0, "folded", 1), 1, bank_layout(cfg, *hw))

    bank = make(kv(layout), kv(layout))
    assert bank.nshot == s and bank.hw == hw and bank.dtype == dt and len(bank.k) == len(layout)
    assert bank.nbytes() == 2 * 2 * s * sum(n * c for n, c in layout)
    with pytest.raises(AttributeError):
        bank.nshot = 3
    with pytest.raises(ValueError, match=r"\(h, w\)"):
        make(kv(bank_layout(cfg, 16, 16)), kv(bank_layout(cfg, 16, 16)))           # tensors of another latent size
    with pytest.raises(ValueError, match="dtype"):
        make(kv(layout, dtype=torch.float16), kv(layout, dtype=torch.float16))
    with pytest.raises(ValueError, match="nshot"):
        make(kv(layout, nshot=3), kv(layout, nshot=3))
    with pytest.raises(ValueError, match="layers"):
        make(kv(layout)[:-1], kv(layout)[:-1])
    bank.check(hw=hw, dtype=dt, residual_dtype=dt, fold_key=(1.0, "folded", 1), weights_id=1)
    for bad, word in ((dict(hw=(16, 16)), r"\(h, w\)"), (dict(dtype=torch.float16), "storage dtype"),
                      (dict(residual_dtype=torch.float32), "residual"), (dict(fold_key=(3.0, "folded", 2)), "fold key"),
                      (dict(weights_id=2), "weights")):
        with pytest.raises(ValueError, match=word):
            bank.check(**bad)
    # the SD-2.1 figure of the docstring: 16 layers, 11.55 M elements per image, 46.2 MB of K and V
    full = bank_layout(config.get("sd21_unet"), 64, 64)
    assert len(full) == 16 and sum(n * c for n, c in full) == 11550720
