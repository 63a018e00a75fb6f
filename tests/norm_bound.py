"""Per-element error bounds of the norm, reduction and pointwise kernels (csrc/norm.hip, backward.hip, misc.hip) against
fp64 references of the same operations.

Every reference is plain fp64 tensor algebra on the exact operands the kernel reads (16-bit or fp32 x, fp32 gamma / beta,
and for the GroupNorm backward the forward's own (mean, rstd) buffer); nothing goes through F.group_norm, F.layer_norm or
autograd.  One function per operation returns (r, e): the reference and the error allowance of every output element, to
which check() adds the output rounding u_T |r| and the subnormal floor of the output type (elementwise_bound.check).

Constants.  C_ACC, U, FLOOR, SILU_SLOPE, GELU_SLOPE, ERF_AS are elementwise_bound's.  u = 2^-24 is the fp32 unit roundoff;
every fp32 add, multiply, fma, IEEE divide and sqrtf (hipcc rounds `/` and sqrtf correctly by default) costs one u.
TRANS = 4 u is the relative error allowed to one hardware transcendental: v_exp_f32, v_rcp_f32 and v_rsq_f32 are specified
to 1 ulp (= 2 u) in AMD's "CDNA3 / CDNA4 Instruction Set Architecture" reference guides, and HIP's math-API table gives
__expf, rsqrtf and exp2f at most 2 ulp for the OCML wrappers (range scaling for denormals) around them.  exp(x) evaluated
as exp2(x log2 e) adds |x| u for the rounded product, as elementwise_bound's SiLU term does.  Nothing here was fitted to a
measurement; all constants were fixed before the first GPU run.

A sum of n fp32 terms accumulated along a path of fold levels with n_1, n_2, ... terms per accumulator is allowed
acc(path) sum|terms| = C_ACC u sqrt(n_1 + n_2 + ...) sum|terms| (errors of the levels add in quadrature; n_i are read off
the launch geometry, restated below from the host code: gn_geometry, gnb_geometry, lnb_blocks, colsum_plan).

GroupNorm statistics.  gn_stats_kernel keeps one fp32 (sum, sum of squares) per thread and channel over
ceil(ppc / slots) pixels, folds slots x cpg of them per group and chunk, and gn_finalize_kernel folds the chunks in fp64:
    e_S = acc([ppc / slots, slots cpg]) sum|x|,    e_Q = the same of sum x^2      (per image and group, n = HW cpg)
    e_mean = e_S / n                               e_var = e_Q / n + 2 |mean| e_S / n
    e_rstd / rstd = e_var / (2 (var + eps))
With sum x^2 / n = mean^2 + var this is  acc (mean^2 + var) / (2 (var + eps))  plus the mean term: the single-pass
variance E[x^2] - mean^2 amplifies the accumulation error by (mean^2 + var) / (var + eps) -- the cancellation term, written
out in gn_stats_ref.  Statistics fused into the producing conv (pre_partial) use elementwise_bound.gn_chunk_check's own
tolerance, n_chunk u and (n_chunk + 1) u, for the chunk sums instead of acc().

GroupNorm apply evaluates x rs + (beta - mean rs), rs = rstd gamma, in fp32: 3 u (|x rs| + |mean rs| + |beta|) (rs, the
product mean rs, the shift, the final fma), plus the propagated statistics error |gamma| (rstd e_mean + |xhat| e_rstd/rstd),
then SiLU as in elementwise_bound (slope SILU_SLOPE, approximation (|z| + 6) u |r|).  LayerNorm is two-pass: no
amplification; the mean error enters the variance only as e_mean^2.

Backward dx = rstd (gamma dz - m1 - xhat m2) (+ dx_add): the accumulation errors of the two means scaled by rstd and
rstd |xhat|, the silu_grad approximation, 4 u of fp32 evaluation, one rounding for the fp32 addend.  dgamma, dbeta, column
sums: acc(path) sum|terms| + per-term errors + u |r|, with `accumulate` (u |old|) and `grad_scale`.

Measured on the MI355X (tests/test_norm_plans_gpu.py, cases off* / f32_off*: B=2, HW=4096, C=128), the relative error of
the kernel's rstd at |mean| / std = 0 / 8 / 64:
    fp32 input   5.9e-8 / 2.8e-6 / 1.6e-4       bf16 input   8.1e-8 / 7.4e-7 / 2.2e-5       fp16 input   6.9e-8 / 1.4e-6 / 1.1e-4
all between 0.001 and 0.03 of the allowance above (the CPU emulation of tests/test_norm_plans_cpu.py gives 5.9e-8 / 2.4e-6 /
2.0e-4 for fp32 input), so the single-pass variance stays as it is: at |mean| / std = 64 it costs 1.6e-4 of |xhat|, below the
1e-3 bar of the fp32-residual-stream mode and below the output rounding of either storage type.
"""
import math

import torch

import elementwise_bound as eb
from elementwise_bound import C_ACC, U, FLOOR, SILU_SLOPE, GELU_SLOPE, ERF_AS, F64

U32 = 2.0 ** -24
TRANS = 4 * U32


def check(y, r, e, out_dtype, where=None, label=""):
    return eb.check(y, r, e, out_dtype, where=where, label=label)


def acc(path):
    return C_ACC * U32 * math.sqrt(float(sum(path)))


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------- launch geometry (host code)

def gn_geometry(B, HW, C, want_wg=2048):
    """norm.hip gn_geometry -> (chunks, ppc, threads, slots)."""
    tpp = C // 8
    slots = max(1, 256 // tpp)
    ppc = max(cdiv(HW, max(1, want_wg // B)), slots * 4)
    return cdiv(HW, ppc), ppc, tpp * slots, slots


def gnb_geometry(B, HW, C):
    """backward.hip gnb_geometry."""
    return gn_geometry(B, HW, C, 1024)


def lnb_blocks(rows):
    return min(256, max(1, cdiv(rows, 4)))


def colsum_plan(rps):
    chunks = max(1, min(1024, cdiv(rps, 64)))
    rpc = (cdiv(rps, chunks) + 7) & ~7
    return cdiv(rps, rpc), rpc


def grid_for(items, cap=4096):
    return int(min(cap, max(1, cdiv(items, 256))))


def ln_maxc(C):
    return 1 if C <= 512 else (2 if C <= 1024 else 4)


# ---------------------------------------------------------------------------------------- failure positions

class Where:
    """Flat index -> text.  kind 'gn': [B, HW, C] (image, group, channel, pixel chunk of ppc pixels); 'stats': [B, G, 2];
    'rows': [rows, C] (row, channel, 16-channel column group); 'cols': [segs, N] (segment, column / channel)."""

    def __init__(self, kind, **kw):
        self.kind, self.kw = kind, kw

    def __call__(self, flat):
        k, flat = self.kw, int(flat)
        if self.kind == "gn":
            b, rem = divmod(flat, k["HW"] * k["C"])
            p, c = divmod(rem, k["C"])
            return f"image {b}, group {c // (k['C'] // k['groups'])}, channel {c}, pixel {p} (pixel chunk {p // k['ppc']})"
        if self.kind == "stats":
            bg, w = divmod(flat, 2)
            return f"image {bg // k['groups']}, group {bg % k['groups']}, {'rstd' if w else 'mean'}"
        if self.kind == "rows":
            r, c = divmod(flat, k["C"])
            return f"row {r}, channel {c} (column group {c // 16})"
        s, c = divmod(flat, k["N"])
        return f"segment {s}, channel {c} (column group {c // 16})"


# ---------------------------------------------------------------------------------------- GroupNorm forward

def _per_channel(t, cpg):
    """[B, G] -> [B, 1, C]."""
    return t.repeat_interleave(cpg, 1)[:, None, :]


def gn_stats_ref(x, groups, eps, pre_chunks=0):
    """x [B, HW, C] -> fp64 (mr [B, G, 2], e_mr [B, G, 2]): (mean, rstd) and their allowances (the fp32 store adds u |r|
    in check()).  pre_chunks > 0: the chunk sums come from the producing conv (HW cpg / pre_chunks terms each)."""
    B, HW, C = x.shape
    cpg = C // groups
    n = HW * cpg
    v = x.to(F64).reshape(B, HW, groups, cpg)
    S, A, Q = v.sum((1, 3)), v.abs().sum((1, 3)), (v * v).sum((1, 3))
    if pre_chunks:
        nc = n / pre_chunks
        fS, fQ = nc * U32, (nc + 1) * U32
    else:
        chunks, ppc, threads, slots = gn_geometry(B, HW, C)
        fS = fQ = acc([cdiv(ppc, slots), slots * cpg])
    mean = S / n
    var = (Q / n - mean * mean).clamp_min(0.0)
    rstd = (var + eps).rsqrt()
    e_mean = fS * A / n
    # var = E[x^2] - mean^2 from fp32 sums: the error of E[x^2] is relative to mean^2 + var, not to var
    amplification = (mean * mean + var) / (var + eps)
    e_var_rel = fQ * amplification + 2 * mean.abs() * e_mean / (var + eps)
    e_rstd = rstd * 0.5 * e_var_rel
    return torch.stack([mean, rstd], -1), torch.stack([e_mean, e_rstd], -1)


def _silu_fwd(pre, e_pre):
    r = pre * torch.sigmoid(pre)
    return r, SILU_SLOPE * e_pre + (pre.abs() + 6.0) * U32 * r.abs()


def gn_fwd_ref(x, gamma, beta, groups, eps, silu, pre_chunks=0):
    """-> (r, e) [B, HW, C] of GroupNorm (+SiLU), and (mr, e_mr) of the statistics."""
    B, HW, C = x.shape
    cpg = C // groups
    mr, e_mr = gn_stats_ref(x, groups, eps, pre_chunks)
    mean, rstd = _per_channel(mr[..., 0], cpg), _per_channel(mr[..., 1], cpg)
    # the kernel reads the statistics back as fp32: their store rounding propagates too
    e_mean = _per_channel(e_mr[..., 0] + U32 * mr[..., 0].abs(), cpg)
    e_rstd_rel = _per_channel(e_mr[..., 1] / mr[..., 1] + U32, cpg)
    ga = gamma.to(x.device, F64)[None, None, :] if gamma is not None else torch.ones(1, 1, C, dtype=F64, device=x.device)
    be = beta.to(x.device, F64)[None, None, :] if beta is not None else torch.zeros(1, 1, C, dtype=F64, device=x.device)
    x64 = x.to(F64)
    rs = rstd * ga
    xhat_g = (x64 - mean) * rs
    pre = xhat_g + be
    e_pre = 3 * U32 * ((x64 * rs).abs() + (mean * rs).abs() + be.abs()) + ga.abs() * rstd * e_mean + xhat_g.abs() * e_rstd_rel
    if silu:
        r, e = _silu_fwd(pre, e_pre)
    else:
        r, e = pre, e_pre
    return r, e, mr, e_mr


# ---------------------------------------------------------------------------------------- GroupNorm backward

def _silu_grad(z, e_z):
    """silu'(z) = sg (1 + z (1 - sg)) as backward.hip evaluates it, and its allowance: sg = rcp(1 + exp(-z)) is off by
    eps_s = (|z| + 6) u relative (exp2 of a rounded product, 1 + e, rcp: elementwise_bound's accounting), which reaches
    the result through sg and through z (1 - sg); four fp32 operations; |silu''| <= 0.5 propagates e_z."""
    sg = torch.sigmoid(z)
    g = sg * (1.0 + z * (1.0 - sg))
    eps_s = (z.abs() + 6.0) * U32
    return g, eps_s * (g.abs() + z.abs() * sg * sg) + 4 * U32 * (g.abs() + z.abs() * sg) + 0.5 * e_z


def gn_bwd_ref(x, dy, mr, gamma, beta, groups, silu, dx_add=None, dgamma0=None, dbeta0=None, grad_scale=1.0):
    """x, dy [B, HW, C]; mr [B, G, 2] fp32: the forward's own buffer (an input here).  dgamma0 / dbeta0: the previous
    contents when accumulating.  -> {'dx': (r, e), 'dgamma': (r, e), 'dbeta': (r, e)}."""
    B, HW, C = x.shape
    cpg = C // groups
    n = HW * cpg
    dev = x.device
    mr = mr.to(dev, F64)
    mean, rstd = _per_channel(mr[..., 0], cpg), _per_channel(mr[..., 1], cpg)
    ga = gamma.to(dev, F64)[None, None, :] if gamma is not None else torch.ones(1, 1, C, dtype=F64, device=dev)
    be = beta.to(dev, F64)[None, None, :] if beta is not None else torch.zeros(1, 1, C, dtype=F64, device=dev)
    xh = (x.to(F64) - mean) * rstd
    e_xh = 2 * U32 * xh.abs()
    d = dy.to(F64)
    if silu:
        z = ga * xh + be
        g, e_g = _silu_grad(z, 3 * U32 * ((ga * xh).abs() + be.abs()))
        dz = d * g
        e_dz = d.abs() * e_g + U32 * dz.abs()
    else:
        dz, e_dz = d, torch.zeros_like(d)
    t2 = dz * xh
    e_t2 = dz.abs() * e_xh + xh.abs() * e_dz + U32 * t2.abs()
    chunks, ppc, threads, slots = gnb_geometry(B, HW, C)
    path_c = [cdiv(ppc, slots), slots, cdiv(chunks, 4), 2]      # thread, slots, gn_bwd_fold lane, its 4-way tree
    s1, a1, e1 = dz.sum(1), dz.abs().sum(1), e_dz.sum(1)                                   # [B, C]
    s2, a2, e2 = t2.sum(1), t2.abs().sum(1), e_t2.sum(1)
    e_s1, e_s2 = acc(path_c) * a1 + e1, acc(path_c) * a2 + e2
    out = {}
    gs = float(grad_scale)
    for name, s, a, e_terms, old in (("dbeta", s1, a1, e1, dbeta0), ("dgamma", s2, a2, e2, dgamma0)):
        tot = gs * s.sum(0)
        e = abs(gs) * (acc(path_c + [B]) * a.sum(0) + e_terms.sum(0)) + 2 * U32 * tot.abs()
        if old is not None:
            o = old.to(dev, F64)
            tot, e = tot + o, e + U32 * o.abs()
        out[name] = (tot, e)
    path_g = [cdiv(cpg, 64), 6]                                  # gn_bwd_group_param_kernel: lane stride, butterfly
    g2 = ga[0]                                                   # [1, C]

    def group_mean(s, e_s):
        w = (g2 * s).reshape(B, groups, cpg)
        m = w.sum(-1) / n
        e = ((g2.abs() * e_s).reshape(B, groups, cpg).sum(-1) + (acc(path_g) + U32) * w.abs().sum(-1)) / n + 2 * U32 * m.abs()
        return _per_channel(m, cpg), _per_channel(e, cpg)

    m1, e_m1 = group_mean(s1, e_s1)
    m2, e_m2 = group_mean(s2, e_s2)
    r = rstd * (ga * dz - m1 - xh * m2)
    e = rstd * (ga.abs() * e_dz + e_m1 + xh.abs() * e_m2 + m2.abs() * e_xh) \
        + 4 * U32 * rstd * ((ga * dz).abs() + m1.abs() + (xh * m2).abs())
    if dx_add is not None:
        r = r + dx_add.to(F64)
        e = e + U32 * r.abs()
    out["dx"] = (r, e)
    return out


# ---------------------------------------------------------------------------------------- LayerNorm

def ln_stats_ref(x, eps):
    """x [rows, C] -> fp64 mean, rstd [rows, 1], e_mean, e_rstd_rel of ln_kernel / ln_bwd_kernel's two-pass statistics: a
    lane adds 8 MAXC values, six butterfly levels; the mean's error enters the variance only as e_mean^2."""
    C = x.shape[1]
    x64 = x.to(F64)
    a = acc([8 * ln_maxc(C), 6])
    mean = x64.mean(1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(1, keepdim=True)
    e_mean = a * x64.abs().mean(1, keepdim=True) + U32 * mean.abs()
    e_rstd_rel = 0.5 * (a + 4 * U32 + e_mean * e_mean / (var + eps)) + TRANS
    return mean, (var + eps).rsqrt(), e_mean, e_rstd_rel


def ln_fwd_ref(x, gamma, beta, eps):
    mean, rstd, e_mean, e_rr = ln_stats_ref(x, eps)
    ga, be = gamma.to(x.device, F64)[None, :], beta.to(x.device, F64)[None, :]
    xg = (x.to(F64) - mean) * rstd * ga
    r = xg + be
    return r, ga.abs() * rstd * e_mean + xg.abs() * (e_rr + 3 * U32) + U32 * r.abs()


def ln_bwd_ref(x, dy, gamma, eps, dx_add=None, dgamma0=None, dbeta0=None, grad_scale=1.0):
    """-> {'dx', 'dgamma', 'dbeta'}: (r, e).  ln_bwd_kernel recomputes the statistics (two-pass fp32) itself."""
    rows, C = x.shape
    dev = x.device
    mean, rstd, e_mean, e_rr = ln_stats_ref(x, eps)
    ga = gamma.to(dev, F64)[None, :]
    xh = (x.to(F64) - mean) * rstd
    e_xh = rstd * e_mean + xh.abs() * (e_rr + 2 * U32)
    d = dy.to(F64)
    gd = ga * d
    a = acc([8 * ln_maxc(C), 6])
    m1 = gd.mean(1, keepdim=True)
    e_m1 = (a + U32) * gd.abs().mean(1, keepdim=True) + 2 * U32 * m1.abs()
    t = gd * xh
    m2 = t.mean(1, keepdim=True)
    e_m2 = (a + 2 * U32) * t.abs().mean(1, keepdim=True) + (gd.abs() * e_xh).mean(1, keepdim=True) + 2 * U32 * m2.abs()
    core = rstd * (gd - m1 - xh * m2)
    e = rstd * (e_m1 + xh.abs() * e_m2 + m2.abs() * e_xh) + core.abs() * e_rr \
        + 4 * U32 * rstd * (gd.abs() + m1.abs() + (xh * m2).abs())
    r = core
    if dx_add is not None:
        r = core + dx_add.to(F64)
        e = e + U32 * r.abs()
    out = {"dx": (r, e)}
    nb = lnb_blocks(rows)
    path = [cdiv(rows, nb * 4), 4, cdiv(nb, 16), 16]             # wave's rows, 4 waves, fold lane, 16 lanes
    gs = float(grad_scale)
    for name, terms, e_terms, old in (("dgamma", d * xh, d.abs() * e_xh + U32 * (d * xh).abs(), dgamma0),
                                      ("dbeta", d, None, dbeta0)):
        tot = gs * terms.sum(0)
        ee = abs(gs) * (acc(path) * terms.abs().sum(0) + (e_terms.sum(0) if e_terms is not None else 0.0)) + 2 * U32 * tot.abs()
        if old is not None:
            o = old.to(dev, F64)
            tot, ee = tot + o, ee + U32 * o.abs()
        out[name] = (tot, ee)
    return out


# ---------------------------------------------------------------------------------------- column sums

def colsum_ref(x, segs, scale=1.0, old=None):
    """x [rows, N] (any row stride) -> (r, e) [segs, N]: out = (old) + scale * column sums per segment.  Path: a thread's
    rpc / 8 rows, 8 row lanes, a fold lane's chunks / 16 partials, the 16-lane tree."""
    rows, N = x.shape
    rps = rows // segs
    chunks, rpc = colsum_plan(rps)
    v = x.to(F64).reshape(segs, rps, N)
    s = float(scale) * v.sum(1)
    e = abs(float(scale)) * acc([rpc // 8, 8, cdiv(chunks, 16), 16]) * v.abs().sum(1) + 2 * U32 * s.abs()
    if old is not None:
        o = old.to(x.device, F64).reshape(segs, N)
        s, e = s + o, e + U32 * o.abs()
    return s, e


# ---------------------------------------------------------------------------------------- softmax

def softmax_rows_ref(x, scale, approx_exp=False, nonfinite=False):
    """x [rows, L] fp32 -> (r, e) of softmax(x * scale).  Each probability exp2((x - m) c), c = fl(scale log2 e): the
    difference, c and the product are rounded (3 u |(x - m) scale| on the exponent), TRANS for exp2; the row sum
    (L / 256 terms per thread -- 4 L / 1024 in the register kernel --, butterfly, 4 waves) carries the p-weighted mean of
    those plus acc(); the divide and the final product one u each.  approx_exp: __expf (softmax_groups), same budget.
    nonfinite (tests/nonfinite.py): a logit of -inf is a mask -- its probability is exactly 0 and carries no error, so
    its exponent term (inf) is left out of the row's allowance instead of turning it into 0 x inf."""
    rows, L = x.shape
    s = x.to(F64) * float(scale)
    m = s.max(1, keepdim=True).values
    p = torch.softmax(s, 1)
    eps_i = 3 * U32 * (s - m).abs() + TRANS
    if nonfinite:
        eps_i = torch.where(s == -math.inf, torch.zeros_like(eps_i), eps_i)
    path = [cdiv(L, 256), 6, 4] if not approx_exp else [L]
    rel = eps_i + (p * eps_i).sum(1, keepdim=True) + acc(path) + 3 * U32
    return p, p * rel


def softmax_groups_ref(x, groups, L, nonfinite=False):
    """x [rows, ld] fp32 -> (r, e) [rows, ld]: softmax over each group's L entries; columns >= groups * L are exactly 0."""
    rows, ld = x.shape
    r = torch.zeros(rows, ld, dtype=F64, device=x.device)
    e = torch.zeros_like(r)
    p, pe = softmax_rows_ref(x[:, :groups * L].reshape(rows * groups, L), 1.0, approx_exp=True, nonfinite=nonfinite)
    r[:, :groups * L], e[:, :groups * L] = p.reshape(rows, -1), pe.reshape(rows, -1)
    return r, e


# ---------------------------------------------------------------------------------------- pointwise

def _gelu(g):
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


def _gelu_err(g, gel):
    """|gelu_erf(g) - gelu(g)|: A-S erf + the rcp / exp2 inside it, the 0.5 x (1 + erf) products (elementwise_bound)."""
    return 0.5 * g.abs() * (ERF_AS + 4 * U32) + 3 * U32 * gel.abs()


def geglu_unpack(pre):
    """packed pre [rows, 2H] -> fp64 value, gate [rows, H] (64-column groups: 32 value columns, their 32 gate columns)."""
    rows, H2 = pre.shape
    v = pre.to(F64).view(rows, H2 // 64, 2, 32)
    return v[:, :, 0].reshape(rows, H2 // 2), v[:, :, 1].reshape(rows, H2 // 2)


def geglu_pack(a, g):
    rows, H = a.shape
    return torch.stack([a.view(rows, H // 32, 32), g.view(rows, H // 32, 32)], 2).reshape(rows, 2 * H)


def geglu_fwd_ref(pre):
    a, g = geglu_unpack(pre)
    gel = _gelu(g)
    r = a * gel
    return r, a.abs() * _gelu_err(g, gel) + U32 * r.abs()


def geglu_bwd_ref(pre, dout):
    """-> (r, e) [rows, 2H] packed: d value = d gelu(g); d gate = d a gelu'(g), gelu' = cdf + g pdf with the A-S cdf and
    pdf = 0.39894 __expf(-g^2 / 2) (exponent g^2 u, TRANS, three products)."""
    a, g = geglu_unpack(pre)
    d = dout.to(F64)
    gel = _gelu(g)
    da = d * gel
    e_da = d.abs() * _gelu_err(g, gel) + U32 * da.abs()
    cdf = 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0)))
    gp = g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    gg = cdf + gp
    e_gg = 0.5 * (ERF_AS + 4 * U32) + U32 * cdf + gp.abs() * (g * g * U32 + TRANS + 3 * U32) + U32 * gg.abs()
    dg = d * a * gg
    e_dg = (d * a).abs() * e_gg + 2 * U32 * dg.abs()
    return geglu_pack(da, dg), geglu_pack(e_da, e_dg)


def add_ref(a, b):
    r = a.to(F64) + b.to(F64)
    return r, U32 * r.abs()


def pool2x2_ref(a):
    """[B, 2H, 2W, C] -> [B, H, W, C] sums of the 2x2 blocks: three fp32 adds."""
    B, H2, W2, C = a.shape
    v = a.to(F64).view(B, H2 // 2, 2, W2 // 2, 2, C)
    return v.sum((2, 4)), 3 * U32 * v.abs().sum((2, 4))


def silu_ref(a, dy=None):
    """silu_kernel: sg by an IEEE divide; silu(a) = a sg, or dy sg (1 + a (1 - sg))."""
    z = a.to(F64)
    if dy is None:
        r = z * torch.sigmoid(z)
        return r, (z.abs() + 6.0) * U32 * r.abs()
    g, e_g = _silu_grad(z, torch.zeros_like(z))
    d = dy.to(F64)
    r = d * g
    return r, d.abs() * e_g + 2 * U32 * r.abs()


def mse_ref(pred, target, loss_scale, blocks=256):
    """-> loss (r, e) [1] and dpred (r, e) NCHW: loss = mean d^2 (a thread's total / (256 blocks) terms, butterfly, 4 waves,
    then 256 / 64 per lane and a butterfly); dpred = d * fl(fl(2 / total) loss_scale): four roundings."""
    d = pred.to(F64) - target.to(F64)
    total = d.numel()
    q = (d * d).sum().reshape(1)
    loss = q / total
    e_loss = (acc([cdiv(total, 256 * blocks), 6, 2, blocks // 64, 6]) + 2 * U32 + 2 * U32) * loss
    g = d * (2.0 / total * float(loss_scale))
    return (loss, e_loss), (g, 4 * U32 * g.abs())


def loss_grad_ref(g, scale):
    r = g.to(F64) * float(scale)
    return r, U32 * r.abs()


def sumsq_ref(x, blocks=1024):
    """sum x^2 of n fp32 values: four partial sums of n / (4 x 256 blocks) terms (fma), their tree, the scalar tail, butterfly,
    4 waves, 1024 / 64 partials per lane of the final fold and its butterfly."""
    v = x.to(F64)
    r = (v * v).sum().reshape(1)
    n = v.numel()
    return r, acc([cdiv(n, 4 * 256 * blocks), 2, 1, 6, 2, blocks // 64, 6]) * r


def adamw_ref(p, g, m, v, step, lr, beta1, beta2, eps, wd, sumsq=None, max_norm=0.0):
    """One AdamW step in fp64 from the operands adamw_kernel reads: fp32 p, g, m, v, the fp32 hyper-parameters (rounded
    here as the launch rounds them), the device's sum of squares and the fp64 clip factor from it.
    -> {'p', 'm', 'v'}: (r, e); the 16-bit shadow is checked against 'p' with the shadow's dtype as output type.
    bc = 1 - powf(beta, step) on the host: powf's ulp, 2 u beta^step, becomes 2 u beta^step / bc relative."""
    f = lambda t: float(torch.tensor(t, dtype=torch.float32))
    lr, beta1, beta2, eps, wd, max_norm = f(lr), f(beta1), f(beta2), f(eps), f(wd), f(max_norm)
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    clip, e_g_rel = 1.0, 0.0
    if sumsq is not None and max_norm > 0.0:
        clip = min(1.0, max_norm / (math.sqrt(float(sumsq)) + f(1e-6)))
        e_g_rel = 4 * U32                                   # sqrtf, the sum, the divide, g * clip
    g = g * clip
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    e_bc1, e_bc2 = 2 * U32 * beta1 ** step / bc1 + U32, 2 * U32 * beta2 ** step / bc2 + U32
    w1 = p * (1.0 - lr * wd)
    t_m = (1.0 - beta1) * g
    m1 = beta1 * m + t_m
    e_m = 2 * U32 * (beta1 * m).abs() + (3 * U32 + e_g_rel) * t_m.abs()
    t_v = (1.0 - beta2) * g * g
    v1 = beta2 * v + t_v
    e_v = 2 * U32 * (beta2 * v).abs() + (4 * U32 + 2 * e_g_rel) * t_v
    sq = v1.sqrt()
    e_sq = e_v / (2 * sq + 1e-300) + U32 * sq
    root = sq / math.sqrt(bc2)
    denom = root + eps
    e_denom = e_sq / math.sqrt(bc2) + root * (0.5 * e_bc2 + 2 * U32) + U32 * denom
    k = lr / bc1
    upd = k * (m1 / denom)
    e_upd = upd.abs() * (e_denom / denom + e_bc1 + 3 * U32) + k * e_m / denom
    w = w1 - upd
    e_w = 3 * U32 * w1.abs() + e_upd
    return {"p": (w, e_w), "m": (m1, e_m), "v": (v1, e_v)}
