"""CPU tests (no GPU) of N-way segmentation: the grouped-bank entry points of the attention kernel and dfw_seg_labels
through the header, the ctypes table and the host-only queries (validation, kernel name, workspace); the definition of the
feature in the oracle's arithmetic; known answers of the label rule (tests/nway_ref.py, the reference the GPU tests of
tests/test_nway_gpu.py compare with exactly) and of metrics.nway_iou; the SupportBankSet handle on host tensors."""
import ctypes as C
import os
import re

import pytest
import torch

import nway_ref
import test_support_bank_cpu as sb

DFW_EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sets_name(L, a, group):
    buf = C.create_string_buffer(96)
    L.check(L.lib().dfw_fsa_sets_kernel_name(C.byref(a), group, buf, 96), "dfw_fsa_sets_kernel_name")
    return buf.value.decode()


def test_header_ctypes_and_symbols(hip_lib):
    """The three new entry points are declared in the header with the issue's signatures, bound in _lib.SYMBOLS with
    matching argument lists and exported; dfw_fsa_args is untouched (bank_shared still its last field)."""
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int dfw_fsa_attention_sets(const dfw_fsa_args* a, int32_t group, dfw_stream_t stream);" in flat
    assert "int dfw_fsa_sets_kernel_name(const dfw_fsa_args* a, int32_t group, char* buf, size_t n);" in flat
    assert re.search(r"int dfw_seg_labels\(const uint8_t\* seg_u8, const uint32_t\* mx, const uint8_t\* gt, uint8_t\* labels, "
                     r"int64_t\* counts, int32_t N, int32_t B, int32_t H, int32_t Wd, float r_threshold, float threshold, "
                     r"int32_t batch_max, dfw_stream_t stream\);", flat)
    i32, vp, f32 = C.c_int32, C.c_void_p, C.c_float
    assert L.SYMBOLS["dfw_fsa_attention_sets"] == (i32, [C.POINTER(L.FsaArgs), i32, vp])
    assert L.SYMBOLS["dfw_fsa_sets_kernel_name"] == (i32, [C.POINTER(L.FsaArgs), i32, C.c_char_p, C.c_size_t])
    assert L.SYMBOLS["dfw_seg_labels"] == (i32, [vp] * 5 + [i32] * 4 + [f32, f32, i32, vp])
    for name in ("dfw_fsa_attention_sets", "dfw_fsa_sets_kernel_name", "dfw_seg_labels"):
        assert getattr(hip_lib, name) is not None
    assert L.FsaArgs._fields_[-1] == ("bank_shared", i32)
    assert hip_lib.dfw_version() >= 104


def test_host_validation(hip_lib):
    """Everything that is not a sets launch is DFW_EINVAL from both attention entry points, on the host, before any launch
    (safe without a GPU): group = 0 (and below), batch % group != 0, n_plain > 0, bank_shared = 1, nshot = 0.  dfw_seg_labels
    rejects N = 0 and N = 255 (and null pointers, a ground truth without counts, the dynamic threshold without maxima)."""
    from diffews_amd import _lib as L
    h = L.lib()
    ok = dict(batch=6, heads=2, n_q=128, n_kv=128, n_bank=128, nshot=2)
    buf = C.create_string_buffer(96)
    for group in (1, 2, 3, 6):
        a = sb._fsa_args(L, **ok)
        assert h.dfw_fsa_sets_kernel_name(C.byref(a), group, buf, 96) == 0, group
    for bad, group in ((ok, 0), (ok, -2), (ok, 4), (ok, 12), (dict(ok, n_plain=2), 2), (dict(ok, bank_shared=1), 2),
                       (dict(ok, bank_shared=1), 6), (dict(ok, nshot=0, n_bank=0), 2),
                       (dict(batch=6, heads=2, n_q=128, n_kv=128), 1)):
        a = sb._fsa_args(L, **bad)
        assert h.dfw_fsa_attention_sets(C.byref(a), group, None) == DFW_EINVAL, (bad, group)
        assert h.dfw_fsa_sets_kernel_name(C.byref(a), group, buf, 96) == DFW_EINVAL, (bad, group)
    p = 4096          # never dereferenced: rejected on the host
    lab = lambda N, u8=p, mx=p, gt=None, out=p, cnt=None, r=0.25: h.dfw_seg_labels(u8, mx, gt, out, cnt, N, 2, 8, 8, r, 0.0,
                                                                                     0, None)
    for N in (0, 255, -1, 1000):
        assert lab(N) == DFW_EINVAL, N
    assert lab(3, u8=None) == DFW_EINVAL and lab(3, out=None) == DFW_EINVAL
    assert lab(3, gt=p, cnt=None) == DFW_EINVAL
    assert lab(3, mx=None) == DFW_EINVAL            # dynamic threshold needs the maxima
    from diffews_amd import ops
    q = torch.zeros(4, 128, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"fsa_attention: k_bank must hold 2 images \(nshot for each of the B // group sets\), got 3"):     # ops: the stack holds exactly (B // group) * nshot images
        ops.fsa_attention_sets(q, q, q, 2, q[:3], q[:3], nshot=1, group=2)
    with pytest.raises(ValueError):
        ops.fsa_attention_sets(q, q, q, 2, q, q, nshot=0, group=2)


def test_sets_kernel_name_and_workspace(hip_lib):
    """A sets launch is the two-pass read launch (n_plain = 0) of the same fields with another bank index: for every
    bank-reading n_plain == 0 key of the recorded parent names and every group that divides its batch, the name is the
    recorded name + '+sets'; the workspace query does not know the group at all (it is dfw_fsa_workspace_bytes)."""
    from diffews_amd import _lib as L
    seen, n = set(), 0
    for key, want in sb.PARENT_NAMES.items():
        dtype, pre, batch, heads, ntok, nshot, n_plain, ws = key
        if n_plain or not nshot:
            continue
        for group in (1, 2, 4, batch):
            if batch % group:
                continue
            for dt in (L.BF16, L.F16):
                a = sb._args_of(L, (dt,) + key[1:])
                name = _sets_name(L, a, group)
                assert name == sb._name(L, a) + "+sets", (key, group)
                assert name == want.replace("<bf16,", "<bf16," if dt == L.BF16 else "<f16,") + "+sets", (key, group)
                seen.add(name)
                n += 1
    assert n >= 40
    assert any("+split" in s for s in seen) and any("+xcd" in s for s in seen)
    assert any(",8,1," in s for s in seen) and any(",4,1," in s for s in seen)


def _oracle():
    from diffews_amd import config, weights
    from oracle.unet import OracleUNet
    from oracle.vae import OracleVAE
    kw = lambda c: {k: v for k, v in c.items() if not k.startswith("_")}
    ucfg, vcfg = config.get("tiny_unet"), config.get("tiny_vae")
    ou = OracleUNet(**kw(ucfg)); ou.load_state_dict(weights.synthetic_unet_state_dict(ucfg)); ou.eval()
    ov = OracleVAE(**kw(vcfg)); ov.load_state_dict(weights.synthetic_vae_state_dict(vcfg)); ov.eval()
    return ou, ov, weights.synthetic_text_embed(ucfg).float()


def test_oracle_definition_of_nway():
    """The definition of the feature, in the reference's own arithmetic (fp32 oracle, tiny config, N = 2 classes, s = 2,
    b = 2): z0[c] is the reference's call for class c with its supports replicated per query; ONE class-major call -- the
    queries repeated per class, entry c*b + i reading the supports of class c -- gives the same z0 (what the grouped bank
    index computes); and the label map of nway_ref on the quantised decoded masks agrees with the reference's binary
    prediction per class (oracle.pipeline.threshold_mask): background exactly where no class predicts foreground, a
    label only where its class does, and never a class of smaller score than another foreground class."""
    import numpy as np
    from oracle import pipeline as op
    ou, ov, te = _oracle()
    g = torch.Generator().manual_seed(11)
    N, s, b, H = 2, 2, 2, 64
    sup = torch.rand(N, s, 3, H, H, generator=g) * 2 - 1
    msk = (torch.rand(N, s, 1, H, H, generator=g) > 0.5).float().repeat(1, 1, 3, 1, 1) * 2 - 1
    qry = torch.rand(b, 3, H, H, generator=g) * 2 - 1
    per = [op.single_infer(ou, ov, sup[c].repeat(b, 1, 1, 1), qry, msk[c].repeat(b, 1, 1, 1), te) for c in range(N)]
    z0 = torch.stack([r["z0"] for r in per])                                           # [N, b, 4, h, w]: the definition
    one = op.single_infer(ou, ov, torch.cat([sup[c].repeat(b, 1, 1, 1) for c in range(N)]), qry.repeat(N, 1, 1, 1),
                          torch.cat([msk[c].repeat(b, 1, 1, 1) for c in range(N)]), te)
    assert z0.dtype == torch.float32 and one["z0"].shape == (N * b, *z0.shape[2:])
    assert torch.allclose(one["z0"].view_as(z0), z0, rtol=1e-5, atol=1e-5 * float(z0.abs().max()))
    seg_u8 = torch.stack([torch.from_numpy(r["seg"].clip(0, 255).numpy().astype(np.uint8)) for r in per])   # P:534
    lab = nway_ref.labels(seg_u8)
    sc = nway_ref.scores(seg_u8)
    binary = torch.stack([torch.stack([op.threshold_mask(np.moveaxis(seg_u8[c, i].numpy(), 0, -1))[0] for i in range(b)])
                          for c in range(N)]).bool()                                   # [N, b, H, W]
    assert torch.equal(nway_ref.foreground(seg_u8), binary)
    assert torch.equal(lab == 0, ~binary.any(0))
    for c in range(N):
        mine = lab == c + 1
        assert bool(binary[c][mine].all())
        for o in range(N):
            assert bool((sc[c][mine] >= sc[o][mine])[binary[o][mine]].all())
    # N = 1: the labels ARE the binary prediction
    assert torch.equal(nway_ref.labels(seg_u8[:1]).bool(), binary[0])


def test_label_rule_known_answers():
    """A hand-built 2 x 4 example, N = 3, fixed threshold 0.5 (scores are (u0 + u1 + u2) / 765):
        px 0: class 0 and class 1 both at 1.0               -> tie, lowest class: label 1
        px 1: class 1 and class 2 tie at 0.8, class 0 below -> label 2
        px 2: every class below the threshold               -> background 0
        px 3: class 2 highest                               -> label 3, gt 255: dropped from the counts
        px 4: class 0 highest, gt 4 (> N)                   -> label 1, dropped from the counts
        px 5: class 1 only                                  -> label 2, gt 2: an intersection
        px 6: every class below the threshold, gt 0         -> 0, an intersection of the background
        px 7: class 0 at 0.4 below, class 2 at 1.0          -> label 3, gt 1: a miss
    and a score equal to the threshold is not foreground (the comparison is strict, in fp32)."""
    N, B, H, W = 3, 1, 2, 4
    u = torch.zeros(N, B, 3, H, W, dtype=torch.uint8)
    px = lambda c, i, val: u[c, 0, :, i // W, i % W].fill_(val)
    px(0, 0, 255); px(1, 0, 255); px(2, 0, 100)
    px(0, 1, 100); px(1, 1, 204); px(2, 1, 204)
    px(0, 2, 10); px(1, 2, 100); px(2, 2, 127)
    px(0, 3, 200); px(1, 3, 201); px(2, 3, 250)
    px(0, 4, 250); px(1, 4, 200); px(2, 4, 128)
    px(0, 5, 0); px(1, 5, 129); px(2, 5, 0)
    px(0, 6, 100); px(1, 6, 100); px(2, 6, 100)
    px(0, 7, 102); px(1, 7, 0); px(2, 7, 255)
    gt = torch.tensor([[[1, 2, 0, 255], [4, 2, 0, 1]]], dtype=torch.uint8)
    lab, cnt = nway_ref.seg_labels(u, gt, r_threshold=0.0, threshold=0.5)
    assert lab.tolist() == [[[1, 2, 0, 3], [1, 2, 0, 3]]]
    # kept pixels 0 1 2 5 6 7: labels 1 2 0 2 0 3, gt 1 2 0 2 0 1
    assert cnt.tolist() == [[[2, 1, 2, 0], [2, 2, 2, 1]]]
    # the threshold is strict, in fp32: a score equal to it is background
    px(0, 6, 153); px(1, 6, 153); px(2, 6, 153)
    thr = float(nway_ref.scores(u)[0, 0, 1, 2])
    assert nway_ref.labels(u, 0.0, thr)[0, 1, 2] == 0 and nway_ref.labels(u, 0.0, thr - 1e-6)[0, 1, 2] == 1
    # dynamic threshold: per image 0.25 * max / 255; batch_max takes the class' maximum over the batch
    u2 = torch.zeros(1, 2, 3, 1, 2, dtype=torch.uint8)
    u2[0, 0, :, 0, 0], u2[0, 0, :, 0, 1] = 40, 8          # image 0: max 40 -> thr 0.0392; 8 / 255 = 0.0314 is background
    u2[0, 1, :, 0, 0], u2[0, 1, :, 0, 1] = 200, 40        # image 1: max 200 -> thr 0.196; 40 / 255 = 0.157 is background
    assert nway_ref.labels(u2).tolist() == [[[1, 0]], [[1, 0]]]
    assert nway_ref.labels(u2, batch_max=True).tolist() == [[[0, 0]], [[1, 0]]]


def test_nway_iou_known_answer():
    """counts of two images, N = 3: label 0 IoU 6/10, label 1 5/10, label 2 0/4, label 3 never predicted nor present (union
    0: left out of the mean)."""
    from diffews_amd.metrics import nway_iou
    counts = torch.tensor([[[4, 2, 0, 0], [6, 5, 1, 0]],
                           [[2, 3, 0, 0], [4, 5, 3, 0]]], dtype=torch.int64)
    iou, miou = nway_iou(counts)
    assert iou.tolist() == [60.0, 50.0, 0.0, 0.0]
    assert miou == 25.0
    iou2, miou2 = nway_iou(counts.sum(0))
    assert torch.equal(iou, iou2) and miou2 == miou
    assert nway_iou(torch.zeros(1, 2, 3, dtype=torch.int64))[1] == 0.0
    with pytest.raises(ValueError):
        nway_iou(torch.zeros(2, 4, dtype=torch.int64)[:, :1])


def test_support_bank_set_handle():
    """SupportBankSet on host tensors: validation names the mismatch, the handle is immutable and reports its bytes,
    .bank(c) is a SupportBank of zero-copy slices (the same handle on every call), stack() copies banks into a set and
    names the first field in which a bank differs."""
    from diffews_amd import config
    from diffews_amd.unet import SupportBank, SupportBankSet, bank_layout
    cfg = config.get("tiny_unet")
    dt, N, s, hw = torch.bfloat16, 3, 2, (8, 8)
    layout = bank_layout(cfg, *hw)
    key = (1.0, "folded", 1)

    def kv(n_img, layout=layout, dtype=dt):
        return [torch.randn(n_img, n, c).to(dtype) for n, c in layout]

    k, v = kv(N * s), kv(N * s)
    st = SupportBankSet(k, v, N, s, hw, dt, dt, key, 1, layout)
    assert st.nsets == N and st.nshot == s and st.hw == hw and st.dtype == dt and len(st.k) == len(layout)
    assert st.nbytes() == 2 * 2 * N * s * sum(n * c for n, c in layout)
    with pytest.raises(AttributeError):
        st.nsets = 4
    st.check(hw=hw, dtype=dt, residual_dtype=dt, fold_key=key, weights_id=1)
    for bad, word in ((dict(hw=(16, 16)), r"\(h, w\)"), (dict(dtype=torch.float16), "storage dtype"),
                      (dict(residual_dtype=torch.float32), "residual"), (dict(fold_key=(3.0, "folded", 2)), "fold key"),
                      (dict(weights_id=2), "weights")):
        with pytest.raises(ValueError, match=word):
            st.check(**bad)
    with pytest.raises(ValueError, match="images"):
        SupportBankSet(kv(N * s + 1), kv(N * s + 1), N, s, hw, dt, dt, key, 1, layout)
    with pytest.raises(ValueError, match="dtype"):
        SupportBankSet(kv(N * s, dtype=torch.float16), kv(N * s, dtype=torch.float16), N, s, hw, dt, dt, key, 1, layout)
    with pytest.raises(ValueError, match=r"\(h, w\)"):
        SupportBankSet(kv(N * s, bank_layout(cfg, 16, 16)), kv(N * s, bank_layout(cfg, 16, 16)), N, s, hw, dt, dt, key, 1, layout)
    with pytest.raises(ValueError):
        SupportBankSet(k, v, 0, s, hw, dt, dt, key, 1, layout)
    # .bank(c): a SupportBank aliasing the stack
    uids = {st.uid}
    for c in range(N):
        bk = st.bank(c)
        assert isinstance(bk, SupportBank) and bk is st.bank(c) and bk.nshot == s and bk.hw == hw
        bk.check(hw=hw, dtype=dt, residual_dtype=dt, fold_key=key, weights_id=1)
        for i in range(len(layout)):
            assert bk.k[i].data_ptr() == k[i][c * s].data_ptr() and bk.v[i].data_ptr() == v[i][c * s].data_ptr()
            assert torch.equal(bk.k[i], k[i][c * s:(c + 1) * s])
        uids.add(bk.uid)
    assert len(uids) == N + 1                      # a set and its banks never share a captured-graph key
    with pytest.raises(IndexError):
        st.bank(N)
    # stack(): copies, set-major
    banks = [SupportBank(kv(s), kv(s), s, hw, dt, dt, key, 1, layout) for _ in range(N)]
    st2 = SupportBankSet.stack(banks)
    assert st2.nsets == N and st2.nshot == s and st2.uid != st.uid
    for c in range(N):
        for i in range(len(layout)):
            assert torch.equal(st2.bank(c).k[i], banks[c].k[i]) and torch.equal(st2.bank(c).v[i], banks[c].v[i])
            assert st2.bank(c).k[i].data_ptr() != banks[c].k[i].data_ptr()
    other = lambda **kw: SupportBank(kv(kw.get("s", s), bank_layout(cfg, *kw.get("hw", hw)), kw.get("dt", dt)),
                                     kv(kw.get("s", s), bank_layout(cfg, *kw.get("hw", hw)), kw.get("dt", dt)), kw.get("s", s),
                                     kw.get("hw", hw), kw.get("dt", dt), kw.get("rd", dt), kw.get("key", key), kw.get("wid", 1),
                                     bank_layout(cfg, *kw.get("hw", hw)))
    for bad, word in ((other(s=3), "nshot"), (other(hw=(16, 16)), r"\(h, w\)"), (other(dt=torch.float16), "storage dtype"),
                      (other(rd=torch.float32), "residual"), (other(key=(2.0, "folded", 1)), "fold key"),
                      (other(wid=7), "weights")):
        with pytest.raises(ValueError, match=word):
            SupportBankSet.stack([banks[0], bad])
    # the FIRST mismatch is the one named: nshot before dtype
    with pytest.raises(ValueError, match="bank 2 differs from bank 0 in nshot"):
        SupportBankSet.stack([banks[0], banks[1], other(s=3, dt=torch.float16)])
    with pytest.raises(ValueError):
        SupportBankSet.stack([])
