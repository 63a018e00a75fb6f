"""Per-element error bound of the attention kernels (forward and backward) against an fp64 reference of the same operation.

Companion of tests/elementwise_bound.py (same check() / U / FLOOR / C_ACC conventions; an fp32 accumulation over n terms is
allowed C_ACC 2^-24 sqrt(n) of the sum of absolute values, as for the GEMMs).  The reference is computed in fp64, on the
device that holds the operands, from exactly the 16-bit q / k / v (/ out / dout) the kernel reads -- a pre-scaled q is used
as given -- per (image, head) and in query chunks, with the key order [own ; shot 0 ; shot 1 ; ...] (bank image
episode * nshot + shot) built here, independently of diffews_amd.ops.  Every bound is a sum of named terms, each from what
the kernel does; the constants were fixed from this derivation before any GPU run and are not fitted to measurements.

Notation (log2 units, the kernels' exp2 domain): s_ij = c q_i.k_j (c = 1 for a pre-scaled q, else scale log2 e),
m_i = max_j s_ij, lse_i = log2 sum_j 2^s_ij, P_ij = 2^(s_ij - lse_i), r_i = sum_j P_ij v_j; A_ij = c sum_d |q_id||k_jd|;
D the head dim, nk the keys of a row, nt its key tiles.

Forward (fsa_ring_kernel + fsa_combine_kernel, xattn_kernel, vattn_kernel):
  score   es_ij = C_ACC 2^-24 (sqrt(D) A_ij + |m_i| + 8) + (4 + nt) 2^-24 (|s_ij| + |m_i| + 8): the fp32 MFMA / FMA
          accumulation of exact 16-bit products with the running reference (at most 2^8 = kDefer below m_i, never above)
          as its initial value; the fp32 constant c, the multiply by c and the subtraction of m_ref c (PRE = false); one
          rounding of the reference per rescale (at most one per tile).
  exp2    v_exp_f32 is accurate to 1 ULP (AMD Instinct CDNA3 / CDNA4 ISA reference guides, V_EXP_F32; V_LOG_F32 and
          V_RCP_F32 likewise): relative E_EXP = 2^-23.  The fp32 probability has relative error ep_ij = ln2 es_ij + E_EXP;
          numerator and l share it: |d r_i| <= sum_j P_ij ep_ij (|v_j| + |r_i|).
  P -> T  P is rounded to T before P.V while l sums the unrounded fp32 P (attention.hip: the P^T pack after `psum`):
          u_T sum_j P_ij |v_j| -- a normalisation mismatch, not |v_j - r_i|.  vattn_kernel does the same; xattn_kernel
          keeps fp32 P (no term).
  subnormal P (fp16): P relative to the running reference is subnormal in T below 2^-14 and its rounding is absolute,
          2^-25 (derived for kept subnormals).  Only keys with s_ij < m_ref - 14 <= m_i - 14 can be subnormal (threshold
          m_i - 13 covers the score error); in units of the normalised P the error is 2^-25 2^(m_ref - lse_i), at most
          2^-25 2^(m_i - lse_i) since the deferred reference never exceeds m_i: sub_T 2^(m_i - lse_i) sum_mask |v_j|.
          bf16 has fp32's exponent range: sub_T = 2^-125 below 2^-125 (also covers v_exp_f32 flushing results < 2^-126).
  accumulation: O over nk keys by MFMA, l over nk keys in fp32, one rescale of both per tile at most:
          C_ACC 2^-24 (sqrt(nk) + nt) (sum_j P_ij |v_j| + |r_i|); xattn_kernel's sequential FMAs over L keys: 3 L 2^-24.
  key-split merge (fsa_combine_kernel): exp2 weights (E_EXP; the partial maxima in fp32: 2 ln2 2^-24 (|m_i| + 8)) and
          fp32 partial sums in split order (2 nsplit 2^-24), on sum_j P_ij |v_j| + |r_i|.
  output  v_rcp_f32 and the product: (E_RCP + 2^-24) |r_i|; then u_T |r| + floor_T in check().
  lse     (fp32; the unsplit path and the combine path): sum_j P_ij es_ij (score errors) + (E_EXP + C_ACC 2^-24
          (sqrt(nk) + nt) + split weights) / ln2 (relative error of l) + E_LOG (log2(nk) + 9) (v_log_f32, 1 ULP of
          log2 l <= log2(nk) + 8) + 2^-23 |lse_i| (m_ref + log2 l in fp32, m_ref c) + 2^-24 |lse| in check().

Backward (fsa_attention_bwd / attention_bwd: fsa_delta_kernel, fsa_bwd_dq_kernel (+ fsa_dq_combine_kernel),
fsa_bwd_dkv_kernel (+ fsa_dkv_fold_kernel)).  The reference takes the `out` and `lse` handed to the kernel as given (the
production chain hands it the forward's own outputs, which pass the forward checks first): P_ij = 2^(s_ij - lse_i),
dP_ij = dO_i.v_j, delta_i = sum_d dO_id O_id, dS_ij = P_ij (dP_ij - delta_i); dq = scale dS K (w.r.t. the unscaled
projection output: the FSA_QSCALE conversion), dk = ln2 dS^T Q (q pre-scaled), dv = P^T dO.
  P       recomputed as exp2(s - lse), s accumulated from -lse: es_ij = C_ACC 2^-24 (8 A_ij + |lse_i|),
          eP_ij = P_ij (ln2 es_ij + E_EXP).
  delta   fp32 from the 16-bit O: e_delta_i = C_ACC 2^-24 8 sum_d |dO_id||O_id|.
  dP      fp32 MFMA from -delta: e_dP_ij = C_ACC 2^-24 (8 (|dO| |V|^T)_ij + |delta_i|) + e_delta_i.
  dS      fp32 product, rounded to T before the dS.K and Q^T.dS MFMAs (attention_bwd.hip: the dQ pack, stage_b):
          E_dS = (1 + u_T) (eP |dP - delta| + P e_dP) + (u_T + 2^-24) |dS| + sub_T [|dS| below 2x T's smallest normal].
  P -> T  for dV (stage_b): E_P = (1 + u_T) eP + u_T P + sub_T [P below 2x T's smallest normal].
  each gradient: its E times the absolute other operand, e.g. scale E_dS |K|, + C_ACC 2^-24 (sqrt(n) + splits) times the
          absolute product (fp32 accumulation over the n keys / query rows, split partials summed in order), + 2 2^-24 |g|
          (the scale / ln2 multiply), + u_T |g| + floor_T in check().
cross_attention_bwd (xattn_bwd_kernel + xattn_bwd_fold_kernel, natural units, fp32 throughout): P = softmax(scale q k^T)
  from __expf (v_exp_f32 on x log2 e: E_EXP + 2^-24 |x|) normalised through l (sum_k P_ik ep_ik + L 2^-24 + E_RCP +
  2^-24), delta = sum_j P dP from the recomputed P, sequential sums (2 L 2^-24 for dq; (64 + chunks) 2^-24 for the
  64-row chunk partials and their fold).

Unlike a global relative L2, this flags an error that stays inside one key tile of one shot, one query block, one head,
one split or one support image's dK / dV: tests/test_attention_plans_cpu.py injects such faults, shows that the existing
`rel() < k TOL` checks accept them and that these bounds reject them, naming the image, head and tile.
"""
import math

import torch

from elementwise_bound import C_ACC, U, FLOOR, F64, check  # noqa: F401  (re-exported for the tests)

LN2 = math.log(2.0)
U24 = 2.0 ** -24
E_EXP = 2.0 ** -23          # v_exp_f32: 1 ULP
E_LOG = 2.0 ** -23          # v_log_f32: 1 ULP of its result
E_RCP = 2.0 ** -23          # v_rcp_f32: 1 ULP
KDEFER = 8.0                # deferred-rescale threshold (log2 units): the running reference is at most 2^8 below the maximum
SUB = {torch.bfloat16: 2.0 ** -125, torch.float16: 2.0 ** -25}     # absolute rounding of a P / dS value in T's subnormal range
NORM_EXP = {torch.bfloat16: 125, torch.float16: 14}                # 2^-NORM_EXP: smallest normal of T (bf16: + exp2 flush)
QCHUNK_ELEMS = 1 << 23      # query rows per reference chunk: rows * keys <= 8 M (64 MB per fp64 matrix)


def _chunks(n, nk):
    step = max(1, min(n, QCHUNK_ELEMS // max(nk, 1)))
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def key_segments(k, v, b, n_plain=0, nshot=0, k_bank=None, v_bank=None):
    """Key / value rows of batch entry b in the kernels' order [own ; shot 0 ; shot 1 ; ...] as a list of (image, K, V):
    own keys k[b] (image b), then for an entry b >= n_plain of a bank-reading launch bank image
    (b - n_plain) * nshot + shot of k_bank / v_bank."""
    segs = [(b, k[b], v[b])]
    if nshot and b >= n_plain:
        for s in range(nshot):
            img = (b - n_plain) * nshot + s
            segs.append((img, k_bank[img], v_bank[img]))
    return segs


# ------------------------------------------------------------------------------------------------ forward

def fwd_ref(q, K, V, dtype, c=1.0, round_p=True, tile=64, nsplit=1, xattn=False, nonfinite=False):
    """fp64 reference and error allowance of one (image, head) of a forward kernel.  q [n, D], K / V [nk, D] (16-bit
    values, any device; K / V in the kernel's key order).  c: factor to log2 units (1: q pre-scaled).
    Returns (r [n, D], e [n, D], lse [n], e_lse [n]): check(y, r, e, dtype) and check(lse_y, lse, e_lse, float32).
    nonfinite (tests/nonfinite.py): a score of -inf is a mask -- its probability is exactly 0 and carries no error, so its
    score allowance (inf) is left out instead of turning the row's allowance into 0 x inf."""
    q, K, V = q.to(F64), K.to(F64), V.to(F64)
    n, D = q.shape
    nk = K.shape[0]
    nt = -(-nk // tile)
    u, sub, nexp = U[dtype], SUB[dtype], NORM_EXP[dtype]
    Va = V.abs()
    r, e = torch.empty(n, D, dtype=F64, device=q.device), torch.empty(n, D, dtype=F64, device=q.device)
    lse, e_lse = torch.empty(n, dtype=F64, device=q.device), torch.empty(n, dtype=F64, device=q.device)
    acc = 3 * nk * U24 if xattn else C_ACC * U24 * (math.sqrt(nk) + nt)
    for i0, i1 in _chunks(n, nk):
        s = (q[i0:i1] @ K.t()) * c
        A = (q[i0:i1].abs() @ K.abs().t()) * abs(c)
        m = s.amax(1, keepdim=True)
        ls = m + torch.log2(torch.exp2(s - m).sum(1, keepdim=True))
        P = torch.exp2(s - ls)
        ri = P @ V
        PV = P @ Va
        es = C_ACC * U24 * (math.sqrt(D) * A + m.abs() + KDEFER) + (4 + nt) * U24 * (s.abs() + m.abs() + KDEFER)
        if nonfinite:
            es = torch.where(s == -math.inf, torch.zeros_like(es), es)
        Pe = P * (LN2 * es + E_EXP)
        ei = Pe @ Va + Pe.sum(1, keepdim=True) * ri.abs()                      # score + exp2
        if round_p:
            ei += u * PV                                                        # P rounded to T, l from the fp32 P
            mask = (s < m - (nexp - 1)).to(F64)
            ei += sub * torch.exp2(m - ls) * (mask @ Va)                        # subnormal P (fp16)
        ei += acc * (PV + ri.abs())                                             # O and l accumulation, rescales
        w_split = torch.zeros_like(m)
        if nsplit > 1:
            w_split = E_EXP + 2 * LN2 * U24 * (m.abs() + KDEFER) + 2 * nsplit * U24
            ei += w_split * (PV + ri.abs())                                     # merge of the key splits
        ei += (E_RCP + U24) * ri.abs()                                          # 1 / l and the product
        r[i0:i1], e[i0:i1] = ri, ei
        lse[i0:i1] = ls[:, 0]
        el = (P * es).sum(1) + (E_EXP + acc + w_split[:, 0]) / LN2
        e_lse[i0:i1] = el + E_LOG * (math.log2(nk) + 9) + 2.0 ** -23 * ls[:, 0].abs()
    return r, e, lse, e_lse


# ------------------------------------------------------------------------------------------------ backward

class BwdAcc:
    """dK / dV of one key image and head, summed over every query pass that reads it (a support image's dK / dV collects
    its own pass and its episode's query pass)."""

    def __init__(self, nk, D, device):
        z = lambda: torch.zeros(nk, D, dtype=F64, device=device)
        self.dk, self.dv, self.edk, self.edv, self.adk, self.adv = z(), z(), z(), z(), z(), z()
        self.rows = 0

    def finish(self, splits=1):
        """(dk, e_dk, dv, e_dv) with the accumulation over all query rows (splits: the dK/dV query split)."""
        acc = C_ACC * U24 * (math.sqrt(max(self.rows, 1)) + splits)
        return (LN2 * self.dk, LN2 * (self.edk + acc * self.adk) + 2 * U24 * LN2 * self.dk.abs(),
                self.dv, self.edv + acc * self.adv)


def bwd_ref(q, segs, o, do, lse, dtype, scale=64 ** -0.5, dq_splits=1):
    """fp64 reference of the flash backward (fsa_bwd_dq_kernel / fsa_bwd_dkv_kernel) for one (query image, head).
    q [n, 64] pre-scaled; segs: list of (K [nk, 64], V [nk, 64], BwdAcc) in key order; o / do [n, 64] (the 16-bit out
    handed to the kernel and its gradient); lse [n] fp32 as handed to the kernel.  Returns (dq, e_dq) and adds the
    dK / dV of each segment to its BwdAcc."""
    q, o, do, lse = q.to(F64), o.to(F64), do.to(F64), lse.to(F64)[:, None]
    n, D = q.shape
    u, sub = U[dtype], SUB[dtype]
    small = 2.0 ** -(NORM_EXP[dtype] - 1)
    K = torch.cat([s[0] for s in segs]).to(F64)
    V = torch.cat([s[1] for s in segs]).to(F64)
    nk = K.shape[0]
    bounds = [0]
    for s in segs:
        bounds.append(bounds[-1] + s[0].shape[0])
    delta = (do * o).sum(1, keepdim=True)
    e_delta = C_ACC * U24 * 8 * (do.abs() * o.abs()).sum(1, keepdim=True)
    Ka, Va, qa, doa = K.abs(), V.abs(), q.abs(), do.abs()
    dq = torch.zeros(n, D, dtype=F64, device=q.device)
    edq, adq = torch.zeros_like(dq), torch.zeros_like(dq)
    for i0, i1 in _chunks(n, nk):
        s = q[i0:i1] @ K.t()
        P = torch.exp2(s - lse[i0:i1])
        dd = do[i0:i1] @ V.t() - delta[i0:i1]
        dS = P * dd
        es = C_ACC * U24 * (8 * (qa[i0:i1] @ Ka.t()) + lse[i0:i1].abs())
        eP = P * (LN2 * es + E_EXP)
        e_dP = C_ACC * U24 * (8 * (doa[i0:i1] @ Va.t()) + delta[i0:i1].abs()) + e_delta[i0:i1]
        E_dS = (1 + u) * (eP * dd.abs() + P * e_dP) + (u + U24) * dS.abs() + sub * (dS.abs() < small).to(F64)
        E_P = (1 + u) * eP + u * P + sub * (P < small).to(F64)
        aS = dS.abs() + E_dS
        dq[i0:i1] = scale * (dS @ K)
        edq[i0:i1] = scale * (E_dS @ Ka)
        adq[i0:i1] = scale * (aS @ Ka)
        for (_, _, accum), j0, j1 in zip(segs, bounds[:-1], bounds[1:]):
            accum.dk += dS[:, j0:j1].t() @ q[i0:i1]
            accum.edk += E_dS[:, j0:j1].t() @ qa[i0:i1]
            accum.adk += aS[:, j0:j1].t() @ qa[i0:i1]
            accum.dv += P[:, j0:j1].t() @ do[i0:i1]
            accum.edv += E_P[:, j0:j1].t() @ doa[i0:i1]
            accum.adv += (P[:, j0:j1] + E_P[:, j0:j1]).t() @ doa[i0:i1]
    for accum in {id(s[2]): s[2] for s in segs}.values():
        accum.rows += n
    acc = C_ACC * U24 * (math.sqrt(nk) + dq_splits)
    return dq, edq + acc * adq + 2 * U24 * dq.abs()


def xattn_bwd_ref(q, k, v, do, scale=64 ** -0.5):
    """fp64 reference of xattn_bwd_kernel + xattn_bwd_fold_kernel for one (image, head): q / do [n, 64], k / v [L, 64]
    (16-bit, q NOT pre-scaled).  Returns (dq, e_dq, dk, e_dk, dv, e_dv)."""
    q, k, v, do = q.to(F64), k.to(F64), v.to(F64), do.to(F64)
    n, L = q.shape[0], k.shape[0]
    chunks = -(-n // 64)
    s = scale * (q @ k.t())
    m = s.amax(1, keepdim=True)
    P = torch.softmax(s, 1)
    dP = do @ v.t()
    dd = dP - (P * dP).sum(1, keepdim=True)
    ee = U24 * (C_ACC * 8 * scale * (q.abs() @ k.abs().t()) + 2 * s.abs()) + 2 * U24 * (s - m).abs() + E_EXP
    eP = P * (ee + (P * ee).sum(1, keepdim=True) + L * U24 + E_RCP + U24)     # normalisation through l, 1 / l, product
    e_dP = C_ACC * U24 * 8 * (do.abs() @ v.abs().t())
    e_delta = (eP * dP.abs() + P * e_dP).sum(1, keepdim=True) + L * U24 * (P * dP.abs()).sum(1, keepdim=True)
    dS = scale * P * dd
    E_dS = scale * (eP * dd.abs() + P * (e_dP + e_delta) + 3 * U24 * P * dd.abs())
    aS = dS.abs() + E_dS
    fold = (64 + chunks) * U24
    dq, e_dq = dS @ k, E_dS @ k.abs() + 2 * L * U24 * (aS @ k.abs())
    dk, e_dk = dS.t() @ q, E_dS.t() @ q.abs() + fold * (aS.t() @ q.abs())
    dv, e_dv = P.t() @ do, eP.t() @ do.abs() + fold * ((P + eP).t() @ do.abs())
    return dq, e_dq, dk, e_dk, dv, e_dv


# ------------------------------------------------------------------------------------------------ failure messages

class Where:
    """Flat index of a [batch, rows, heads * D] tensor (lse=True: [batch, heads, rows]) -> 'image, head, row (block),
    column' text.  block: rows per query block (a forward workgroup's rows) or per key tile (what='key')."""

    def __init__(self, rows, heads, block, what="query row", lse=False, D=64):
        self.rows, self.heads, self.block, self.what, self.lse, self.D = rows, heads, block, what, lse, D

    def __call__(self, flat):
        flat = int(flat)
        kind = "key tile" if self.what == "key" else "query block"
        if self.lse:
            bh, row = divmod(flat, self.rows)
            b, h = divmod(bh, self.heads)
            return f"image {b}, head {h}, {self.what} {row} ({kind} {row // self.block})"
        C = self.heads * self.D
        b, rem = divmod(flat, self.rows * C)
        row, col = divmod(rem, C)
        return f"image {b}, head {col // self.D}, {self.what} {row} ({kind} {row // self.block}), column {col % self.D}"
