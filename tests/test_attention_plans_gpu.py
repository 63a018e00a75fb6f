"""Plan matrix of the attention kernels, forward and backward, in both storage dtypes, checked element by element.

Each forward case of dfw_fsa_attention names the launch it must take -- asserted through the host-only dfw_fsa_kernel_name
query on the arguments ops.fsa_attention passes (ops._fsa_call), and without a GPU by tests/test_attention_plans_cpu.py,
which also proves that the cases together reach all 8 fsa_ring_kernel instantiations and every split / combine / XCD-remap
variant.  Backward cases state the dQ key split / dK-dV query split they must take (read from the workspace queries).
Every output element, and every row's lse, is compared with an fp64 reference within the bound of
tests/attention_bound.py; `-s` prints the path and the worst err / bound ratio of every case.

Edges: the NW = 4 / 8 boundary (n_q 1024 / 1025), n_q % 128 in {1, 127}, n_q < 32, n_kv % 64 in {1, 63}, n_kv = 77 with
separate K / V, n_bank != n_kv, nshot 0 / 1 / 2 / 7 in the lock-step and the two-pass form, key splits whose instances walk
several segments (own + bank) and counts that do not divide 1 + nshot, column slices of one fused QKV buffer with
ld > 3C and padded batch strides, heads 1 / 5 / 10, the deferred-rescale ramps (rising and falling); cross-attention
L in {1, 2, 63, 64, 65, 77, 128}; VAE batches above 8 (the second round of its XCD grid), ragged N, the restart path,
padded batch strides; backward with ragged n, dQ split on / forced / off, dK/dV query split on / off, and gradients
written into column slices whose neighbouring columns must stay untouched.
"""
import contextlib
import ctypes as C
import math
from dataclasses import dataclass, field

import pytest
import torch

import attention_bound as ab

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
TNAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
QSCALE = 64 ** -0.5 * math.log2(math.e)       # ops.FSA_QSCALE
VQSCALE = 512 ** -0.5 * math.log2(math.e)     # ops.VATTN_QSCALE
SENTINEL = 3.0


@contextlib.contextmanager
def configured(L, cfg):
    L.configure()
    try:
        if cfg:
            L.configure(**cfg)
        yield
    finally:
        L.configure()


@contextlib.contextmanager
def fsa_names(ops, L, launch=True):
    """Record dfw_fsa_kernel_name of every dfw_fsa_attention call ops makes (and launch it unless launch=False)."""
    names, orig, device_rule = [], ops._fsa_call, ops._Args.device

    def rec(a):
        buf = C.create_string_buffer(96)
        L.check(L.lib().dfw_fsa_kernel_name(C.byref(a), buf, 96), "dfw_fsa_kernel_name")
        names.append(buf.value.decode())
        if launch:
            orig(a)

    ops._fsa_call = rec
    if not launch:
        ops._Args.device = lambda self: None          # planning on host tensors: nothing is launched
    try:
        yield names
    finally:
        ops._fsa_call, ops._Args.device = orig, device_rule


def _strided(B, n, width, pad, dtype, device, g=None, fill=True):
    """[B, n, width] view of a flat buffer with image stride n * width + pad (pad elements between images)."""
    bs = n * width + pad
    flat = (torch.randn(B * bs, generator=g) if fill else torch.empty(B * bs)).to(dtype)
    return flat.to(device).as_strided((B, n, width), (bs, width, 1))


# ------------------------------------------------------------------------------------------------ forward cases

@dataclass
class Fsa:
    id: str
    B: int                   # batch entries of the launch (lock-step: n_plain support images, then the query images)
    heads: int
    n_q: int
    n_kv: int
    expect: str              # planned launch, {T} = bf16 | f16
    nshot: int = 0
    n_plain: int = 0
    n_bank: int = 0          # > 0: a separate bank of that many keys per image; 0: the bank is k[:n_plain] (lock-step)
    pre: bool = True
    cfg: dict = field(default_factory=dict)
    key_split: bool = True
    ramp: float = 0.0        # != 0: the deferred-rescale ramp of test_ops_gpu (B = heads = 1)


FSA_CASES = [
    Fsa("nshot0_nq1025_nw8", 1, 1, 1025, 1025, "fsa_ring_kernel<{T},8,1,pre>"),
    Fsa("nshot0_nq1024_heads5", 2, 5, 1024, 1024, "fsa_ring_kernel<{T},4,1,pre>"),
    Fsa("nq129_nkv65_scale", 2, 5, 129, 65, "fsa_ring_kernel<{T},4,1,scale>", pre=False),
    Fsa("nq17_nkv127_heads10", 4, 10, 17, 127, "fsa_ring_kernel<{T},4,1,pre>+xcd"),
    Fsa("attn2_nkv77", 2, 5, 300, 77, "fsa_ring_kernel<{T},4,1,pre>"),
    Fsa("nq1151_nkv1087_nw8_scale", 2, 1, 1151, 1087, "fsa_ring_kernel<{T},8,1,scale>", pre=False),
    Fsa("twopass_shot1", 2, 2, 1024, 1024, "fsa_ring_kernel<{T},4,1,pre>", nshot=1, n_bank=1024),
    Fsa("twopass_shot2_nbank321", 2, 2, 200, 200, "fsa_ring_kernel<{T},4,1,pre>", nshot=2, n_bank=321),
    Fsa("twopass_shot7_scale", 1, 2, 320, 320, "fsa_ring_kernel<{T},4,1,scale>", nshot=7, n_bank=320, pre=False),
    Fsa("lockstep_shot1_scale", 2, 4, 384, 384, "fsa_ring_kernel<{T},4,1,scale>+xcd", nshot=1, n_plain=1, pre=False),
    Fsa("lockstep_shot2_nw8_scale", 3, 1, 1151, 1151, "fsa_ring_kernel<{T},8,1,scale>", nshot=2, n_plain=2, pre=False),
    Fsa("lockstep_shot3_nbank63", 4, 2, 256, 256, "fsa_ring_kernel<{T},4,1,pre>+xcd", nshot=3, n_plain=3, n_bank=63),
    Fsa("lockstep_shot7_nw8_split8", 8, 2, 1100, 1100, "fsa_ring_kernel<{T},8,1,pre>+split8", nshot=7, n_plain=7),
    Fsa("lockstep_shot7_xcd_split8", 8, 8, 1024, 1024, "fsa_ring_kernel<{T},4,1,pre>+xcd+split8", nshot=7, n_plain=7),
    Fsa("lockstep_shot7_forced3", 8, 1, 1024, 1024, "fsa_ring_kernel<{T},4,1,pre>+split3", nshot=7, n_plain=7,
        cfg=dict(fsa_force_splits=3)),
    Fsa("lockstep_shot7_forced3_xcd_scale", 8, 4, 1024, 1024, "fsa_ring_kernel<{T},4,1,scale>+xcd+split3", nshot=7,
        n_plain=7, pre=False, cfg=dict(fsa_force_splits=3)),
    Fsa("lockstep_shot7_unsplit", 8, 1, 1024, 1024, "fsa_ring_kernel<{T},4,1,pre>+xcd", nshot=7, n_plain=7,
        key_split=False),
    Fsa("twopass_shot2_split3", 2, 2, 256, 2730, "fsa_ring_kernel<{T},4,1,pre>+split3", nshot=2, n_bank=2731),
    Fsa("twopass_shot2_forced2_xcd", 2, 2, 256, 2730, "fsa_ring_kernel<{T},4,1,pre>+xcd+split2", nshot=2, n_bank=2731,
        cfg=dict(fsa_force_splits=2)),
] + [Fsa(f"ramp{step:+g}_{'pre' if pre else 'scale'}", 1, 1, 1024, 1024,
         f"fsa_ring_kernel<{{T}},4,1,{'pre' if pre else 'scale'}>", pre=pre, ramp=step)
     for step in (0.5, 2.0, 5.0, 12.0, -3.0) for pre in (True, False)]


def _ramp_qkv(step):
    """test_ops_gpu.test_fsa_attention_deferred_rescale_ramp's rows: the score maximum climbs by `step` log2 units per
    64-key tile (-3: falls 45 units below the first tile's; 5: also a falling tail)."""
    N, Cc = 1024, 64
    g = torch.Generator().manual_seed(int(abs(step) * 10))
    q = torch.randn(1, N, Cc, generator=g)
    q = q / q.norm(dim=-1, keepdim=True) * 8.0
    k = torch.randn(1, N, Cc, generator=g) * 0.05
    v = torch.randn(1, N, Cc, generator=g)
    q[..., 0] = 4.0
    c = (64 ** -0.5) * 1.4426950408889634
    tile = (torch.arange(N) // 64).float()
    k[0, :, 0] = tile * step / (4.0 * c)
    half = N // 2
    k[0, half:, 0] = k[0, half:, 0].flip(0) if step == 5.0 else k[0, half:, 0]
    return q, k, v


def make_fsa_inputs(case, dtype, device, seed=0, fill=True):
    """q / k / v: column slices of ONE fused buffer [B, n, 3C + 64] with padded image stride when n_q == n_kv, else q
    from its own padded buffer and k / v from a [B, n_kv, 2C + 64] one; a separate bank likewise (n_bank > 0)."""
    g = torch.Generator().manual_seed(seed)
    Cc = case.heads * 64
    qs = QSCALE * 2 if case.pre else 2.0
    inp = {}
    if case.n_q == case.n_kv:
        buf = _strided(case.B, case.n_q, 3 * Cc + 64, 64, torch.float32, "cpu", g, fill)
        if case.ramp:
            q, k, v = _ramp_qkv(case.ramp)
            buf[..., :Cc], buf[..., Cc:2 * Cc], buf[..., 2 * Cc:3 * Cc] = q * (QSCALE if case.pre else 1.0), k, v
        else:
            buf[..., :Cc] *= qs
        buf = buf.to(dtype)
        b = torch.empty_strided(buf.shape, buf.stride(), dtype=dtype, device=device)
        b.copy_(buf) if fill else None
        inp["q"], inp["k"], inp["v"] = b[..., :Cc], b[..., Cc:2 * Cc], b[..., 2 * Cc:3 * Cc]
    else:
        qb = _strided(case.B, case.n_q, Cc + 64, 64, torch.float32, "cpu", g, fill)
        qb[..., :Cc] *= qs
        kb = _strided(case.B, case.n_kv, 2 * Cc + 64, 128, torch.float32, "cpu", g, fill)
        qd = torch.empty_strided(qb.shape, qb.stride(), dtype=dtype, device=device)
        kd = torch.empty_strided(kb.shape, kb.stride(), dtype=dtype, device=device)
        if fill:
            qd.copy_(qb.to(dtype))
            kd.copy_(kb.to(dtype))
        inp["q"], inp["k"], inp["v"] = qd[..., :Cc], kd[..., :Cc], kd[..., Cc:2 * Cc]
    if case.nshot:
        if case.n_bank:
            nb = (case.B - case.n_plain) * case.nshot
            bb = _strided(nb, case.n_bank, 2 * Cc + 64, 64, torch.float32, "cpu", g, fill)
            bd = torch.empty_strided(bb.shape, bb.stride(), dtype=dtype, device=device)
            bd.copy_(bb.to(dtype)) if fill else None
            inp["kb"], inp["vb"] = bd[..., :Cc], bd[..., Cc:2 * Cc]
        else:
            inp["kb"], inp["vb"] = inp["k"][:case.n_plain], inp["v"][:case.n_plain]
    inp["lse"] = torch.empty(case.B, case.heads, case.n_q, dtype=torch.float32, device=device)
    return inp


def run_fsa(ops, case, inp):
    return ops.fsa_attention(inp["q"], inp["k"], inp["v"], case.heads, k_bank=inp.get("kb"), v_bank=inp.get("vb"),
                             nshot=case.nshot, n_plain=case.n_plain, q_prescaled=case.pre, lse=inp["lse"],
                             key_split=case.key_split)


def expected(case, dtype):
    return case.expect.replace("{T}", TNAME[dtype])


def fsa_check(case, dtype, inp, y, name, label):
    """Every output element and every lse against the fp64 reference; returns (worst out ratio, worst lse ratio)."""
    nsplit = int(name.split("+split")[1]) if "+split" in name else 1
    rows = 256 if ",8,1," in name else 128
    c = 1.0 if case.pre else 64 ** -0.5 * math.log2(math.e)
    B, H, n = case.B, case.heads, case.n_q
    dev = y.device
    r = torch.empty(B, n, H * 64, dtype=ab.F64, device=dev)
    e = torch.empty_like(r)
    lr = torch.empty(B, H, n, dtype=ab.F64, device=dev)
    le = torch.empty_like(lr)
    for b in range(B):
        segs = ab.key_segments(inp["k"], inp["v"], b, case.n_plain, case.nshot, inp.get("kb"), inp.get("vb"))
        ns = nsplit if (case.nshot and b >= case.n_plain) else 1
        for h in range(H):
            sl = slice(h * 64, (h + 1) * 64)
            K = torch.cat([s[1][:, sl] for s in segs])
            V = torch.cat([s[2][:, sl] for s in segs])
            r[b, :, sl], e[b, :, sl], lr[b, h], le[b, h] = ab.fwd_ref(inp["q"][b][:, sl], K, V, dtype, c=c, nsplit=ns)
    w = ab.check(y, r, e, dtype, where=ab.Where(n, H, rows), label=label)
    wl = ab.check(inp["lse"], lr, le, torch.float32, where=ab.Where(n, H, rows, lse=True), label=label + " lse")
    return w, wl


@pytest.fixture(scope="module")
def ops(hip_lib):
    from diffews_amd import ops
    return ops


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", FSA_CASES, ids=[c.id for c in FSA_CASES])
def test_fsa_plan(ops, case, dtype):
    from diffews_amd import _lib as L
    want = expected(case, dtype)
    inp = make_fsa_inputs(case, dtype, "cuda", seed=sum(map(ord, case.id)))
    with configured(L, case.cfg), fsa_names(ops, L) as names:
        y = run_fsa(ops, case, inp)
    torch.cuda.synchronize()
    assert names == [want], names
    w, wl = fsa_check(case, dtype, inp, y, want, f"{case.id} {want}")
    print(f"{case.id:36s} {want:44s} worst err/bound {w:.3f}  lse {wl:.3f}")


# ------------------------------------------------------------------------------------------------ cross-attention

@dataclass
class Xa:
    id: str
    B: int
    heads: int
    n_q: int
    L: int


XA_CASES = [Xa("L1", 2, 3, 300, 1), Xa("L2", 2, 2, 257, 2), Xa("L63", 1, 2, 511, 63), Xa("L64", 2, 1, 255, 64),
            Xa("L65", 1, 3, 513, 65), Xa("L77", 2, 2, 300, 77), Xa("L128", 2, 2, 129, 128)]


def make_xa_inputs(case, dtype, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    Cc = case.heads * 64
    q = (torch.randn(case.B, case.n_q, Cc, generator=g) * 2).to(dtype).to(device)
    kv = _strided(case.B, case.L, 2 * Cc + 64, 64, dtype, device, g)
    do = torch.randn(case.B, case.n_q, Cc, generator=g).to(dtype).to(device)
    return q, kv[..., :Cc], kv[..., Cc:2 * Cc], do


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", XA_CASES, ids=[c.id for c in XA_CASES])
def test_cross_attention_plan(ops, case, dtype):
    q, k, v, _ = make_xa_inputs(case, dtype, "cuda", seed=sum(map(ord, case.id)))
    y = ops.cross_attention(q, k, v, case.heads)
    torch.cuda.synchronize()
    r = torch.empty(y.shape, dtype=ab.F64, device=y.device)
    e = torch.empty_like(r)
    c = 64 ** -0.5 * math.log2(math.e)
    for b in range(case.B):
        for h in range(case.heads):
            sl = slice(h * 64, (h + 1) * 64)
            r[b, :, sl], e[b, :, sl], _, _ = ab.fwd_ref(q[b][:, sl], k[b][:, sl], v[b][:, sl], dtype, c=c,
                                                        round_p=False, tile=1, xattn=True)
    w = ab.check(y, r, e, dtype, where=ab.Where(case.n_q, case.heads, 256), label=f"xattn {case.id}")
    print(f"xattn {case.id:30s} xattn_kernel<{TNAME[dtype]}> L={case.L:3d} worst err/bound {w:.3f}")


# ------------------------------------------------------------------------------------------------ VAE mid-block

@dataclass
class Va:
    id: str
    B: int
    N: int
    pad: int = 0             # elements between images (padded batch stride)
    spike: tuple = None      # (image, key): a key ~40 log2 units above every earlier score for 120 query rows


VA_CASES = [Va("B1_N4096", 1, 4096), Va("B9_N100", 9, 100), Va("B12_N1056", 12, 1056), Va("B2_N1000_pad", 2, 1000, 512),
            Va("B1_restart_last_key", 1, 2048, spike=(0, 2047)), Va("B9_restart_image8", 9, 256, 512, spike=(8, 200))]


def make_va_inputs(case, dtype, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    buf = _strided(case.B, case.N, 1536, case.pad, torch.float32, "cpu", g)
    if case.spike:
        buf *= 0.3
        u = torch.randn(512, generator=g)
        u = u / u.norm()
        b, key = case.spike
        rows = slice(min(60, case.N - 120), min(60, case.N - 120) + 120)
        buf[b, rows, :512] += 25.0 * u
        buf[b, key, 512:1024] += 25.0 * u
    buf[..., :512] *= VQSCALE                                  # what linear(..., colscale=(512, VATTN_QSCALE)) hands over
    d = torch.empty_strided(buf.shape, buf.stride(), dtype=dtype, device=device)
    d.copy_(buf.to(dtype))
    return d[..., :512], d[..., 512:1024], d[..., 1024:]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", VA_CASES, ids=[c.id for c in VA_CASES])
def test_vae_attention_plan(ops, case, dtype):
    q, k, v = make_va_inputs(case, dtype, "cuda", seed=sum(map(ord, case.id)))
    y = ops.vae_attention(q, k, v)
    torch.cuda.synchronize()
    r = torch.empty(y.shape, dtype=ab.F64, device=y.device)
    e = torch.empty_like(r)
    for b in range(case.B):
        r[b], e[b], _, _ = ab.fwd_ref(q[b], k[b], v[b], dtype, tile=32)
    w = ab.check(y, r, e, dtype, where=ab.Where(case.N, 1, 128, D=512), label=f"vae {case.id}")
    print(f"vae {case.id:32s} vattn_kernel<{TNAME[dtype]}> worst err/bound {w:.3f}")


# ------------------------------------------------------------------------------------------------ backward

@dataclass
class FsaBwd:
    id: str
    b: int                   # episodes (nshot == 0: plain images)
    nshot: int
    heads: int
    N: int
    splits: int              # dQ key split the launch must take
    cfg: dict = field(default_factory=dict)
    key_split: bool = True


FSA_BWD_CASES = [
    FsaBwd("nshot0", 2, 0, 1, 100, 1),
    FsaBwd("shot1", 2, 1, 2, 129, 1),
    FsaBwd("shot2", 1, 2, 5, 72, 1),
    FsaBwd("shot3", 1, 3, 2, 200, 1),
    FsaBwd("shot4", 1, 4, 1, 65, 1),
    FsaBwd("shot5", 1, 5, 2, 96, 1),
    FsaBwd("shot6", 1, 6, 1, 150, 1),
    FsaBwd("shot7_split8", 1, 7, 2, 1100, 8),
    FsaBwd("shot7_forced3", 1, 7, 2, 1100, 3, cfg=dict(fsa_force_splits=3)),
    FsaBwd("shot7_unsplit", 1, 7, 2, 1100, 1, key_split=False),
]


def fsa_bwd_splits(L, case, dtype_code):
    """The dQ key split dfw_fsa_attention_bwd takes for this case (from dfw_fsa_attention_bwd_workspace_bytes)."""
    n_plain = case.b * case.nshot
    a = L.FsaBwdArgs()
    a.batch, a.heads, a.n, a.nshot, a.n_plain, a.dtype = n_plain + case.b, case.heads, case.N, case.nshot, n_plain, dtype_code
    nbytes = L.lib().dfw_fsa_attention_bwd_workspace_bytes(C.byref(a)) if (case.nshot >= 2 and case.key_split) else 0
    return nbytes // (case.b * case.N * case.heads * 64 * 4) if nbytes else 1


def _fsa_case_of(case):
    n_plain = case.b * case.nshot
    return Fsa(case.id, n_plain + case.b, case.heads, case.N, case.N, "", nshot=case.nshot, n_plain=n_plain,
               key_split=case.key_split)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", FSA_BWD_CASES, ids=[c.id for c in FSA_BWD_CASES])
def test_fsa_attention_bwd_plan(ops, case, dtype):
    from diffews_amd import _lib as L, ops_bwd as ob
    g = torch.Generator().manual_seed(sum(map(ord, case.id)))
    H, N, Cc = case.heads, case.N, case.heads * 64
    n_plain = case.b * case.nshot
    Bt = n_plain + case.b
    qkv = torch.randn(Bt, N, 3 * Cc, generator=g)
    qkv[..., :Cc] *= QSCALE * 2
    qkv = qkv.to(dtype).cuda()
    dout = torch.randn(Bt, N, Cc, generator=g).to(dtype).cuda()
    q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
    fcase = _fsa_case_of(case)
    inp = {"q": q, "k": k, "v": v, "lse": torch.empty(Bt, H, N, dtype=torch.float32, device="cuda")}
    if case.nshot:
        inp["kb"], inp["vb"] = k[:n_plain], v[:n_plain]
    with configured(L, case.cfg):
        assert fsa_bwd_splits(L, case, L.BF16 if dtype == torch.bfloat16 else L.F16) == case.splits
        with fsa_names(ops, L) as names:
            out = run_fsa(ops, fcase, inp)
        dqkv = ob.fsa_attention_bwd(qkv, out, dout, inp["lse"], H, nshot=case.nshot, n_plain=n_plain,
                                    key_split=case.key_split)
    torch.cuda.synchronize()
    wf, wl = fsa_check(fcase, dtype, inp, out, names[0], f"{case.id} forward {names[0]}")
    accs = [[ab.BwdAcc(N, 64, qkv.device) for _ in range(H)] for _ in range(Bt)]
    dq = torch.empty(Bt, N, Cc, dtype=ab.F64, device=qkv.device)
    edq = torch.empty_like(dq)
    for b in range(Bt):
        segs = ab.key_segments(k, v, b, n_plain, case.nshot, k, v)
        ns = case.splits if (case.nshot and b >= n_plain) else 1
        for h in range(H):
            sl = slice(h * 64, (h + 1) * 64)
            dq[b, :, sl], edq[b, :, sl] = ab.bwd_ref(q[b][:, sl], [(K[:, sl], V[:, sl], accs[img][h]) for img, K, V in segs],
                                                     out[b][:, sl], dout[b][:, sl], inp["lse"][b, h], dtype, dq_splits=ns)
    dk, edk, dv, edv = (torch.empty_like(dq) for _ in range(4))
    for b in range(Bt):
        for h in range(H):
            sl = slice(h * 64, (h + 1) * 64)
            dk[b, :, sl], edk[b, :, sl], dv[b, :, sl], edv[b, :, sl] = accs[b][h].finish()
    label = f"{case.id} fsa_bwd split{case.splits}"
    wq = ab.check(dqkv[..., :Cc], dq, edq, dtype, where=ab.Where(N, H, 128), label=label + " dq")
    wk = ab.check(dqkv[..., Cc:2 * Cc], dk, edk, dtype, where=ab.Where(N, H, 64, what="key"), label=label + " dk")
    wv = ab.check(dqkv[..., 2 * Cc:], dv, edv, dtype, where=ab.Where(N, H, 64, what="key"), label=label + " dv")
    print(f"fsa_bwd {case.id:28s} dq split{case.splits}  fwd {wf:.3f} lse {wl:.3f}  dq {wq:.3f} dk {wk:.3f} dv {wv:.3f}")


@dataclass
class AttnBwd:
    id: str
    B: int
    heads: int
    n_q: int
    n_kv: int
    q_split: bool
    qsplit: int              # dK/dV query split the launch must take


ATTN_BWD_CASES = [
    AttnBwd("nkv2_qsplit", 1, 1, 1000, 2, True, 8),
    AttnBwd("nkv2_noqsplit", 1, 1, 1000, 2, False, 1),
    AttnBwd("nkv77_qsplit", 2, 2, 300, 77, True, 2),
    AttnBwd("nkv77_noqsplit", 2, 2, 300, 77, False, 1),
    AttnBwd("nkv77_nq4097_qsplit", 1, 2, 4097, 77, True, 32),
    AttnBwd("nkv130_qsplit", 2, 5, 1000, 130, True, 8),
    AttnBwd("nkv130_noqsplit", 2, 5, 1000, 130, False, 1),
]


def attn_bwd_qsplit(L, case, dtype_code):
    a = L.AttnBwdArgs()
    a.batch, a.heads, a.n_q, a.n_kv, a.dtype = case.B, case.heads, case.n_q, case.n_kv, dtype_code
    nbytes = L.lib().dfw_attention_bwd_workspace_bytes(C.byref(a)) if case.q_split else 0
    return nbytes // (2 * case.B * case.n_kv * case.heads * 64 * 4) if nbytes else 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", ATTN_BWD_CASES, ids=[c.id for c in ATTN_BWD_CASES])
def test_attention_bwd_plan(ops, case, dtype):
    from diffews_amd import _lib as L, ops_bwd as ob
    g = torch.Generator().manual_seed(sum(map(ord, case.id)))
    H, Cc = case.heads, case.heads * 64
    assert attn_bwd_qsplit(L, case, L.BF16 if dtype == torch.bfloat16 else L.F16) == case.qsplit
    qb = _strided(case.B, case.n_q, Cc + 64, 64, torch.float32, "cpu", g)
    qb[..., :Cc] *= QSCALE * 2
    qd = torch.empty_strided(qb.shape, qb.stride(), dtype=dtype, device="cuda")
    qd.copy_(qb.to(dtype))
    q = qd[..., :Cc]
    kv = torch.randn(case.B, case.n_kv, 2 * Cc + 64, generator=g).to(dtype).cuda()
    k, v = kv[..., :Cc], kv[..., Cc:2 * Cc]
    dout = torch.randn(case.B, case.n_q, Cc, generator=g).to(dtype).cuda()
    fcase = Fsa(case.id, case.B, H, case.n_q, case.n_kv, "")
    inp = {"q": q, "k": k, "v": v, "lse": torch.empty(case.B, H, case.n_q, dtype=torch.float32, device="cuda")}
    with fsa_names(ops, L) as names:
        out = run_fsa(ops, fcase, inp)
    dkv = torch.full_like(kv, SENTINEL)
    dq = ob.attention_bwd(q, k, v, out, dout, inp["lse"], H, dkv[..., :Cc], dkv[..., Cc:2 * Cc], q_split=case.q_split)
    torch.cuda.synchronize()
    wf, wl = fsa_check(fcase, dtype, inp, out, names[0], f"{case.id} forward {names[0]}")
    assert (dkv[..., 2 * Cc:] == SENTINEL).all(), "dK/dV stores outside their column slices"
    rq = torch.empty(case.B, case.n_q, Cc, dtype=ab.F64, device="cuda")
    eq = torch.empty_like(rq)
    rk, ek, rv, ev = (torch.empty(case.B, case.n_kv, Cc, dtype=ab.F64, device="cuda") for _ in range(4))
    for b in range(case.B):
        for h in range(H):
            sl = slice(h * 64, (h + 1) * 64)
            acc = ab.BwdAcc(case.n_kv, 64, "cuda")
            rq[b, :, sl], eq[b, :, sl] = ab.bwd_ref(q[b][:, sl], [(k[b][:, sl], v[b][:, sl], acc)], out[b][:, sl],
                                                    dout[b][:, sl], inp["lse"][b, h], dtype)
            rk[b, :, sl], ek[b, :, sl], rv[b, :, sl], ev[b, :, sl] = acc.finish(case.qsplit)
    label = f"{case.id} attention_bwd qsplit{case.qsplit}"
    wq = ab.check(dq, rq, eq, dtype, where=ab.Where(case.n_q, H, 128), label=label + " dq")
    wk = ab.check(dkv[..., :Cc], rk, ek, dtype, where=ab.Where(case.n_kv, H, 64, what="key"), label=label + " dk")
    wv = ab.check(dkv[..., Cc:2 * Cc], rv, ev, dtype, where=ab.Where(case.n_kv, H, 64, what="key"), label=label + " dv")
    print(f"attn_bwd {case.id:27s} qsplit{case.qsplit}  fwd {wf:.3f} lse {wl:.3f}  dq {wq:.3f} dk {wk:.3f} dv {wv:.3f}")


XB_CASES = [Xa("L1", 2, 2, 300, 1), Xa("L2", 1, 3, 65, 2), Xa("L16", 2, 1, 64, 16), Xa("L17", 1, 2, 129, 17),
            Xa("L77", 2, 2, 200, 77), Xa("L80", 1, 4, 100, 80)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", XB_CASES, ids=[c.id for c in XB_CASES])
def test_cross_attention_bwd_plan(ops, case, dtype):
    from diffews_amd import ops_bwd as ob
    q, k, v, do = make_xa_inputs(case, dtype, "cuda", seed=sum(map(ord, case.id)))
    Cc = case.heads * 64
    dkv = torch.full((case.B, case.L, 2 * Cc + 64), SENTINEL, dtype=dtype, device="cuda")
    dq = ob.cross_attention_bwd(q, k, v, do, case.heads, dkv[..., :Cc], dkv[..., Cc:2 * Cc])
    torch.cuda.synchronize()
    assert (dkv[..., 2 * Cc:] == SENTINEL).all(), "dK/dV stores outside their column slices"
    rq = torch.empty(dq.shape, dtype=ab.F64, device="cuda")
    eq = torch.empty_like(rq)
    rk, ek, rv, ev = (torch.empty(case.B, case.L, Cc, dtype=ab.F64, device="cuda") for _ in range(4))
    for b in range(case.B):
        for h in range(case.heads):
            sl = slice(h * 64, (h + 1) * 64)
            rq[b, :, sl], eq[b, :, sl], rk[b, :, sl], ek[b, :, sl], rv[b, :, sl], ev[b, :, sl] = ab.xattn_bwd_ref(
                q[b][:, sl], k[b][:, sl], v[b][:, sl], do[b][:, sl])
    chunks = -(-case.n_q // 64)
    label = f"{case.id} xattn_bwd chunks{chunks}"
    wq = ab.check(dq, rq, eq, dtype, where=ab.Where(case.n_q, case.heads, 64), label=label + " dq")
    wk = ab.check(dkv[..., :Cc], rk, ek, dtype, where=ab.Where(case.L, case.heads, 16, what="key"), label=label + " dk")
    wv = ab.check(dkv[..., Cc:2 * Cc], rv, ev, dtype, where=ab.Where(case.L, case.heads, 16, what="key"),
                  label=label + " dv")
    print(f"xattn_bwd {case.id:26s} fold of {chunks} chunks  dq {wq:.3f} dk {wk:.3f} dv {wv:.3f}")
