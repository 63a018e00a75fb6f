"""Non-finite propagation: every kernel between the loss and the flat gradient must keep an inf or a NaN non-finite.

The step guard (adamw_kernel reads dfw_sumsq of the flat gradient and skips the update when it is not finite) is sound
only if no kernel on the way turns a non-finite value into a finite one.  This helper holds what the two test files share:

  plant(inputs, name, index, value)     a copy of a case's inputs with ONE element of ONE operand replaced;
  check_propagation(y, r, e, T, ...)    the rule: where the fp64 reference r of the same operation on the planted operands
                                        is non-finite, y must be non-finite (inf and NaN are not told apart: 0 x inf may
                                        turn one into the other; sign=True for the store-overflow cases, whose reference
                                        is +-inf with no NaN in play); where r is finite, the family's own bound applies
                                        unchanged, on those elements only (nothing leaks into rows, images or columns that
                                        do not depend on the plant);
  CASES                                 one object per case: make() the finite operands on any device, plants(), ref()
                                        (the fp64 references of elementwise_bound / norm_bound / attention_bound, reused),
                                        declared() (the non-finite set stated analytically, from the operation alone) and
                                        run() (the kernel; GPU only).

tests/test_nonfinite_cpu.py proves on the CPU that ref() and declared() agree for every case, plant and value;
tests/test_nonfinite_gpu.py runs the kernels.  A logit of -inf in a softmax is a mask, not an overflow: its probability is
exactly 0 and the row stays finite, in the reference and (checked) in the kernel; such plants declare an empty set.
Where a reference's allowance itself holds 0 x inf on the planted operands (+-inf in q, k or lse of the attention backward:
Case.bound_applies), the elements the reference keeps finite are required to be finite, without a bound.
"""
import math
from dataclasses import dataclass

import torch

import elementwise_bound as eb
import norm_bound as nb
import test_gemm_plans_gpu as tg

F64, F32 = torch.float64, torch.float32
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = (BF16, F16)
TNAME = {BF16: "bf16", F16: "f16", F32: "f32"}
VALUES = {"+inf": math.inf, "-inf": -math.inf, "nan": math.nan}
EPS = 1e-5
F16_MAX, F16_INF_FROM = 65504.0, 65520.0          # largest finite fp16; the smallest magnitude that rounds to inf


# ------------------------------------------------------------------------------------------------ plant and rule

def plant(inputs, name, index, value):
    """Copy of `inputs` (a dict of tensors and plain values) in which inputs[name][index] = value.  The planted operand
    is a fresh tensor with the original's shape and strides; every other entry, and the original, is left untouched."""
    t = inputs[name]
    c = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)
    c.copy_(t)
    c[tuple(index)] = value
    out = dict(inputs)
    out[name] = c
    return out


def describe(name, index, value):
    return f"{name}[{', '.join(str(int(i)) for i in index)}] = {value}"


@dataclass
class Ref:
    r: torch.Tensor          # fp64 reference
    e: torch.Tensor          # the family's error allowance (without u_T |r| and the floor, which check() adds)
    dtype: torch.dtype       # output type
    where: object = None     # flat index -> text
    check: object = None     # the family's checker (default elementwise_bound.check)


def check_propagation(y, r, e, out_dtype, where=None, label="", planted="", check=None, sign=False, bound=True):
    """The rule, on every element of one output.  Returns (non-finite elements of r, NaN among the matching y, inf among
    them, worst err / bound ratio of the finite part).  bound=False (Case.bound_applies): where r is finite y must be
    finite; no bound is applied."""
    check = check or eb.check
    y64 = y.reshape(r.shape).to(r.device, F64).flatten()
    rf, ef = r.flatten(), e.flatten()
    nf = ~torch.isfinite(rf)
    lost = nf & torch.isfinite(y64)
    what = "finite where the reference is non-finite"
    if sign:
        lost = nf & (y64 != rf)
        what = "not the reference's infinity"
    pos = (lambda i: where(i)) if where is not None else (lambda i: f"element {i}")
    if bool(lost.any()):
        idx = torch.nonzero(lost).flatten()
        i = int(idx[0])
        raise AssertionError(f"{label}: plant {planted}: {idx.numel()} of {int(nf.sum())} output elements {what}; "
                             f"first at {pos(i)}: y={float(y64[i]):.6g} ref={float(rf[i])}")
    keep = torch.nonzero(~nf).flatten()
    worst = 0.0
    if keep.numel() and not bound:
        leaked = keep[~torch.isfinite(y64[keep])]
        if leaked.numel():
            raise AssertionError(f"{label}: plant {planted}: {leaked.numel()} output elements non-finite where the reference "
                                 f"is finite; first at {pos(int(leaked[0]))}")
    elif keep.numel():
        worst = check(y64[keep], rf[keep], ef[keep], out_dtype, where=lambda i: pos(int(keep[int(i)])),
                      label=f"{label}: plant {planted}: element that does not depend on the plant")
    yn = y64[nf]
    return int(nf.sum()), int(torch.isnan(yn).sum()), int(torch.isinf(yn).sum()), worst


def conv_readers(H, W, stride, pad, ups, y, x):
    """Output pixels (oy, ox) and taps t = ky * 3 + kx of ops.conv3x3's geometry that read input pixel (y, x)."""
    Ho, Wo = tg._conv_out_hw(H, W, stride, pad, ups)
    src = [(uy, ux) for uy in (2 * y, 2 * y + 1) for ux in (2 * x, 2 * x + 1)] if ups else [(y, x)]
    out = set()
    for uy, ux in src:
        for ky in range(3):
            for kx in range(3):
                ny, nx = uy + pad - ky, ux + pad - kx
                if ny % stride == 0 and nx % stride == 0 and 0 <= ny // stride < Ho and 0 <= nx // stride < Wo:
                    out.add((ny // stride, nx // stride, ky * 3 + kx))
    return Ho, Wo, sorted(out)


def _rnd(g, shape, dtype, device, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype).to(device)


class Case:
    family = ""
    dtypes = DTYPES
    full = ()                # outputs that are full reductions (no finite element is required there)
    overflow = False         # a store-overflow case: finite operands, the reference exceeds the fp16 range
    value_dependent = False  # the declared set depends on which value is planted (signs, masks)

    def masked(self, name, index, value):
        """True where the plant is a mask by definition (a -inf logit): the declared set is empty."""
        return False

    def values(self, name, index):
        """Names (keys of VALUES) planted at this position: all three unless the case says why not."""
        return tuple(VALUES)

    def bound_applies(self, name, index, value):
        """False where the family's allowance is not defined on the planted operands (0 x inf inside it): the elements the
        reference keeps finite must then be finite, without a bound."""
        return True

    def post(self, env, inp, dtype, outs, planted):
        """Further GPU-side assertions on what run() returned."""


# ------------------------------------------------------------------------------------------------ GEMM / conv forward

class GemmFwd(Case):
    """One Fwd case of tests/test_gemm_plans_gpu.py: its operands, its planned kernel (asserted), its fp64 epilogue."""
    family = "gemm_fwd"

    def __init__(self, source, cid, plants):
        self.c = next(c for c in tg.FWD_CASES if c.id == cid)
        self.source, self.id, self._plants = source, f"{source}/{cid}", plants

    def make(self, dtype, device):
        return tg.make_fwd_inputs(self.c, dtype, device, seed=sum(map(ord, self.c.id)))

    def plants(self):
        return self._plants

    def dims(self):
        return tg.fwd_dims(self.c)

    def ref(self, inp, dtype):
        c = self.c
        M, N, K, rpi, Ho, Wo, imgs = self.dims()
        if c.op == "linear":
            S, A = eb.gemm_ref(inp["x"], inp["w"])
        else:
            S, A = eb.conv_ref(inp["x"], inp["w"], *c.shape[5:])
        r, e = eb.epilogue_ref(S, A, K, bias=inp.get("bias"), rowbias=inp.get("rowbias"), rows_per_img=rpi,
                               residual=inp.get("res"), out_scale=c.scale, colscale=c.colscale, act=c.act,
                               geglu=c.geglu, splits=c.splitk or 1)
        bm, bn = tg.tile_of(c.expect)
        where = eb.Where(r.shape[1], rows_per_img=rpi, Wo=Wo, tile=(bm, bn),
                         patch=c.op == "conv" and Wo % 16 == 0 and Ho % (bm // 16) == 0)
        return {"y": Ref(r, e, dtype if c.out == "T" else F32, where)}

    def _col(self, n):
        return (n // 64) * 32 + n % 32 if self.c.geglu else n

    def declared(self, inp, name, index, value):
        c = self.c
        M, N, K, rpi, Ho, Wo, imgs = self.dims()
        m = torch.zeros(M, N // 2 if c.geglu else N, dtype=torch.bool)
        if name == "x" and c.op == "linear":
            m[index[0], :] = True                                   # A[i, k]: row i
        elif name == "x":
            b, y, x, _ = index                                      # one input pixel: the pixels whose taps read it
            for oy, ox, _t in conv_readers(*c.shape[1:3], *c.shape[5:], y, x)[2]:
                m[b * Ho * Wo + oy * Wo + ox, :] = True
        elif name in ("w", "bias"):
            m[:, self._col(index[0])] = True                        # W[n, k], bias[n]: column n
        elif name == "rowbias":
            m[index[0] * rpi:(index[0] + 1) * rpi, self._col(index[1])] = True
        elif name == "res":
            i = int(torch.arange(M * N).reshape(inp["res"].shape)[tuple(index)])
            m[i // N, i % N] = True
        else:
            raise KeyError(name)
        return {"y": m}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        want = tg.expected(self.c, dtype)
        names = []
        with tg.configured(L, self.c.cfg):
            ops.gemm_hook = lambda name, *a: names.append(name)
            try:
                y = tg.run_fwd(ops, self.c, inp)
            finally:
                ops.gemm_hook = None
        assert names == [want], names
        self._y = y
        return {"y": y.permute(0, 2, 3, 1) if self.c.out == "NCHW" else y}

    def post(self, env, inp, dtype, outs, planted):
        """Fused GroupNorm statistics: a chunk slot over non-finite stored values must be non-finite, and the GroupNorm
        that consumes the sums must give a non-finite group (and stay inside its bound everywhere else)."""
        c = self.c
        if not c.gn:
            return
        ops, ob, L = env
        M, N, K, rpi, Ho, Wo, imgs = self.dims()
        y = self._y
        st = getattr(y, "_gn_stats", None)
        assert st is not None, f"{self.id}: no fused GroupNorm sums"
        bm, bn = tg.tile_of(c.expect)
        label = f"{self.id} plant {planted}"
        eb.gn_chunk_check(y.reshape(imgs, Ho, Wo, N), st[0], c.gn, bm, bn, label=label, nonfinite=True)
        g = torch.Generator().manual_seed(1)
        gamma, beta = _rnd(g, (N,), F32, y.device, 0.2, 1.0), _rnd(g, (N,), F32, y.device, 0.2)
        odt = dtype if y.dtype == F32 else None
        out, mr = ops.groupnorm(y, gamma, beta, c.gn, 1e-6, silu=True, return_stats=True, out_dtype=odt)
        r, e, mr_ref, e_mr = nb.gn_fwd_ref(y.reshape(imgs, Ho * Wo, N), gamma, beta, c.gn, 1e-6, True, pre_chunks=st[1])
        ppc = nb.gn_geometry(imgs, Ho * Wo, N)[1]
        n1 = check_propagation(mr, mr_ref, e_mr, F32, nb.Where("stats", groups=c.gn), label + " fused (mean, rstd)", planted)
        n2 = check_propagation(out, r, e, dtype, nb.Where("gn", HW=Ho * Wo, C=N, groups=c.gn, ppc=ppc),
                               label + " groupnorm from fused sums", planted)
        assert n1[0] > 0 and n2[0] > 0, f"{label}: the consuming GroupNorm's reference has no non-finite group"


_LIN = [("x", (-1, -1)), ("x", (0, 0)), ("w", (-1, 3)), ("w", (0, -1)), ("bias", (-1,)), ("res", (-1, -1)), ("rowbias", (-1, 1))]
_CONV = [("x", (-1, -1, -1, -1)), ("x", (0, 1, 1, 0)), ("w", (-1, 3)), ("bias", (-1,)), ("res", (-1, -1, -1, -1)),
         ("rowbias", (-1, 1))]


def _abs_index(shape, index):
    return tuple(int(i) % int(n) for i, n in zip(index, shape))


def _gemm_case(source, cid):
    case = GemmFwd(source, cid, None)
    probe = tg.make_fwd_inputs(case.c, F16, "cpu", fill=False)
    case._plants = [(n, _abs_index(probe[n].shape, i)) for n, i in (_LIN if case.c.op == "linear" else _CONV) if n in probe]
    return case


GEMM_FWD = [
    _gemm_case("gemm", "gk_splitk_silu"),            # split-K 5 (x[-1, -1]: last K-chunk of the last split), SiLU, row bias
    _gemm_case("gemm", "gk128x128_geglu"),           # GEGLU epilogue, M = 260: last tile of 4 rows
    _gemm_case("gemm", "gk64x64_lin_rf32_f32"),      # fp32 residual stream, out_f32, M = 257
    _gemm_case("gemm", "gk_conv_splitk"),            # conv, split-K 3
    _gemm_case("gemm8", "g8_256x256_geglu"),         # M = 1000: last tile of 232 rows
    _gemm_case("gemm8", "g8_256x256_conv_ups_gn"),   # conv + nearest-2x, fused GroupNorm sums
    _gemm_case("gemm_big", "big256x128x32_lin"),     # M = 513: last tile of 1 row
    _gemm_case("gemm_big", "big256x256_conv_f32o_gn"),   # fp32 output, fused sums of the fp32 values
    _gemm_case("conv_patch8", "cp8_256x128_ragged_gn"),  # N = 192: ragged last n-tile, fused sums
    _gemm_case("conv_patch", "cp512x128_f32o_gn"),       # the smallest conv_patch case: fp32 stream in and out, fused sums
]


# ------------------------------------------------------------------------------------------------ boundary convs, folded up2x

import test_boundary_plans_gpu as tb       # noqa: E402
import test_up2x_fold_gpu as tu            # noqa: E402


class ConvSmall(Case):
    """One single-source Cs case of tests/test_boundary_plans_gpu.py (ops.conv_small: NCHW fp32 x, fp32 w [Cout, taps, Cin])."""
    family = "conv_small"

    def __init__(self, cid):
        self.c = tb.BY_ID[cid]
        self.id = f"conv_small/{cid}"
        assert not isinstance(self.c.B, tuple) and not self.c.misalign

    def make(self, dtype, device):
        c = self.c
        g = torch.Generator().manual_seed(len(c.id) + c.Cout)
        K = c.taps * c.Cin
        return {"x": _rnd(g, (c.B, c.Cin, c.H, c.W), F32, device), "w": _rnd(g, (c.Cout, c.taps, c.Cin), F32, device, K ** -0.5),
                **({"bias": _rnd(g, (c.Cout,), F32, device)} if c.bias else {})}

    def plants(self):
        c = self.c
        p = [("x", (c.B - 1, c.Cin - 1, c.H - 1, c.W - 1)), ("x", (0, 0, 0, 0)),
             ("w", (c.Cout - 1, c.taps // 2, c.Cin - 1))]        # the centre tap: inside the map at every pixel
        return p + ([("bias", (0,))] if c.bias else [])

    def ref(self, inp, dtype):
        c = self.c
        parts = [eb.conv_small_ref(inp["x"][b:b + 1], inp["w"], inp.get("bias"), c.taps, c.in_scale, c.out_scale) for b in range(c.B)]
        r, e = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        return {"y": Ref(r, e, dtype if c.mode == "T" else F32, eb.Where(c.Cout, c.H * c.W, c.W))}

    def declared(self, inp, name, index, value):
        c = self.c
        m = torch.zeros(c.B, c.H, c.W, c.Cout, dtype=torch.bool)
        if name == "x":
            b, _, y, x = index
            reach = (-1, 0, 1) if c.taps == 9 else (0,)
            for dy in reach:
                for dx in reach:
                    if 0 <= y + dy < c.H and 0 <= x + dx < c.W:
                        m[b, y + dy, x + dx] = True
        else:
            m[..., index[0]] = True
        return {"y": m.reshape(-1, c.Cout)}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        c = self.c
        self._iters, self._chunks = tb.planned(c, dtype, L)[1], tb.planned(c, dtype, L)[3]
        y, _, _ = tb.run(ops, c, dtype, [inp["x"]], inp["w"], inp.get("bias"), self._chunks)
        self._y = y
        return {"y": y.permute(0, 2, 3, 1) if c.mode == "NCHW" else y}

    def post(self, env, inp, dtype, outs, planted):
        if self.c.gn and self._chunks:
            st = getattr(self._y, "_gn_stats", None)
            assert st is not None, f"{self.id}: no fused sums"
            eb.cs_chunk_check(self._y, st[0], self.c.gn, self._iters, label=f"{self.id} plant {planted}", nonfinite=True)


class Up2x(Case):
    """ops.conv3x3_up2x: the nearest-2x upsample conv as four folded 2 x 2 parity convs (gemm8_kernel<.., up2x>)."""
    family = "up2x"

    def __init__(self, shape):
        self.shape, self.id = shape, "up2x/" + "x".join(map(str, shape))
        self.GROUPS = 24 if shape[-1] == 192 else 32

    def make(self, dtype, device):
        from diffews_amd import packing
        B, Hi, Wi, Cin, Cout = self.shape
        g = torch.Generator().manual_seed(Hi * Wi + Cin + Cout)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to(dtype)
        return {"x": _rnd(g, (B, Hi, Wi, Cin), dtype, device), "wf": packing.fold_up2x(packing.pack_conv3x3(w)).to(device),
                "bias": _rnd(g, (Cout,), F32, device)}

    def plants(self):
        B, Hi, Wi, Cin, Cout = self.shape
        # wf [Cout][py][px][ty][tx][Cin]: parity (0, 0), tap (1, 1) reads source pixel (y, x) itself: inside the map everywhere
        return [("x", (B - 1, Hi - 1, Wi - 1, Cin - 1)), ("x", (0, 1, 1, 0)), ("wf", (Cout - 1, 3 * Cin + 3)), ("bias", (0,))]

    def ref(self, inp, dtype):
        B, Hi, Wi, Cin, Cout = self.shape
        S, A = tu.folded_ref(inp["x"], inp["wf"])
        r, e = eb.epilogue_ref(S, A, 4 * Cin, bias=inp["bias"])
        return {"y": Ref(r, e, dtype, eb.Where(Cout, 4 * Hi * Wi, 2 * Wi))}

    def declared(self, inp, name, index, value):
        B, Hi, Wi, Cin, Cout = self.shape
        m = torch.zeros(B, 2 * Hi, 2 * Wi, Cout, dtype=torch.bool)
        if name == "x":          # source (sy, sx) is tap (ty, tx) of low-resolution position (sy - ty + 1 - py, ..) of parity (py, px)
            b, sy, sx, _ = index
            for py in range(2):
                for px in range(2):
                    for ty in range(2):
                        for tx in range(2):
                            yl, xl = sy - ty + 1 - py, sx - tx + 1 - px
                            if 0 <= yl < Hi and 0 <= xl < Wi:
                                m[b, 2 * yl + py, 2 * xl + px] = True
        elif name == "wf":
            py, px = index[1] // (8 * Cin), index[1] // (4 * Cin) % 2
            m[:, py::2, px::2, index[0]] = True
        else:
            m[..., index[0]] = True
        return {"y": m.reshape(-1, Cout)}

    def run(self, env, inp, dtype):
        ops = env[0]
        Cout = self.shape[-1]
        y = ops.conv3x3_up2x(inp["x"], inp["wf"], Cout, bias=inp["bias"], gn_groups=self.GROUPS)
        assert y is not None
        self._y = y
        return {"y": y}

    def post(self, env, inp, dtype, outs, planted):
        ops = env[0]
        B, Hi, Wi, Cin, Cout = self.shape
        y, label = self._y, f"{self.id} plant {planted}"
        st = getattr(y, "_gn_stats", None)
        assert st is not None, f"{self.id}: no fused sums"
        s, q, a, n = tu._chunk_sums(y, self.GROUPS, 256 if Cout % 256 == 0 else 128)
        got = st[0].to(F64)
        ratio = torch.maximum((got[..., 0] - s).abs() / (n * 2.0 ** -24 * a + 1e-30),
                              (got[..., 1] - q).abs() / ((n + 1) * 2.0 ** -24 * q + 1e-30))
        ratio = torch.where(torch.isfinite(got).all(-1), ratio, torch.full_like(ratio, math.inf))
        ratio = eb._nonfinite_slots(ratio, s, q, got, label)
        assert float(ratio.max()) <= 1.0, f"{label}: chunk sums off, worst ratio {float(ratio.max()):.3g}"
        g = torch.Generator().manual_seed(5)
        gamma, beta = _rnd(g, (Cout,), F32, y.device, 0.5, 1.0), _rnd(g, (Cout,), F32, y.device)
        fed, mr = ops.groupnorm(y, gamma, beta, self.GROUPS, 1e-6, silu=True, return_stats=True)
        r, e, mr_ref, e_mr = nb.gn_fwd_ref(y.view(B, 4 * Hi * Wi, Cout), gamma, beta, self.GROUPS, 1e-6, True, pre_chunks=st[1])
        n = check_propagation(fed, r, e, dtype, nb.Where("gn", HW=4 * Hi * Wi, C=Cout, groups=self.GROUPS, ppc=1),
                              label + " groupnorm from fused sums", planted)
        assert n[0] > 0
        check_propagation(mr, mr_ref, e_mr, F32, nb.Where("stats", groups=self.GROUPS), label + " fused (mean, rstd)", planted)


BOUNDARY = [ConvSmall("w8_c128"), ConvSmall("dec_in"), ConvSmall("t1_T"), ConvSmall("w4_w12_t9"), ConvSmall("w4_w4_f32"),
            ConvSmall("sc_w10_t9"), ConvSmall("sc_nchw_t1_c4"), Up2x((1, 16, 16, 64, 128)), Up2x((1, 32, 16, 64, 192))]


# ------------------------------------------------------------------------------------------------ dfw_gemm_tn

class GemmTn(Case):
    """One Tn case of tests/test_gemm_plans_gpu.py: out[n][tap][k] (+)= scale sum_m dy[m][n] x[row(m, tap)][k]."""
    family = "gemm_tn"

    def __init__(self, cid):
        self.c = next(c for c in tg.TN_CASES if c.id == cid)
        self.id = cid

    def make(self, dtype, device):
        return tg.make_tn_inputs(self.c, dtype, device, seed=sum(map(ord, self.c.id)))

    def _geo(self):
        c = self.c
        if c.op == "lin":
            M, N, Kc = c.shape
            return M, N, Kc, 1, None
        B, H, W, Kc, N, stride, pad, ups = c.shape
        Ho, Wo = tg._conv_out_hw(H, W, stride, pad, ups)
        return B * Ho * Wo, N, Kc, 9, (B, H, W, Ho, Wo, stride, pad, ups)

    def plants(self):
        """The last M chunk of the last split: an interior pixel of the last image's second-to-last row (all nine taps of
        it are inside the map, so no product is 0 x inf with a padding zero), in dy and in x."""
        M, N, Kc, taps, geo = self._geo()
        if taps == 1:
            return [("dy", (M - 1, N - 1)), ("dy", (0, 0)), ("x", (M - 1, Kc - 1))]
        B, H, W, Ho, Wo = geo[:5]
        out = [("x", (B - 1, H - 2, W - 2, Kc - 1))]
        if Ho >= 3 and Wo >= 3:                       # a 2 x 2 map has no interior pixel
            out.append(("dy", (M - Wo - 2, N - 1)))
        if self.c.accumulate:
            out.append(("out", (0, N - 1, 4, 0)))
        return out

    def ref(self, inp, dtype):
        c = self.c
        dy = inp["dy"].to(F64)
        cols = [inp["x"].reshape(-1, inp["x"].shape[-1]).to(F64)] if c.op == "lin" else eb.conv_taps(inp["x"], *inp["geom"][4:])[2]
        S = torch.stack([dy.t() @ col for col in cols], 1)
        A = torch.stack([dy.abs().t() @ col.abs() for col in cols], 1)
        splits = getattr(self, "_splits", 1)                           # of the launch run() made (the CPU proof: no bound used)
        r = c.scale * S
        e = eb.C_ACC * 2.0 ** -24 * math.sqrt(dy.shape[0]) * abs(c.scale) * A * math.sqrt(splits)
        if c.accumulate:
            pre = inp["out"][0].to(F64)
            r, e = r + pre, e + eb.C_ACC * 2.0 ** -24 * pre.abs() * math.sqrt(splits)
        taps, Kc = r.shape[1], r.shape[2]

        def where(flat):
            n, rem = divmod(int(flat), taps * Kc)
            t, k = divmod(rem, Kc)
            return f"out channel {n}, tap {t}, in channel {k}, tile ({n // 128}, {k // 128})"

        return {"out": Ref(r, e, F32, where)}

    def declared(self, inp, name, index, value):
        M, N, Kc, taps, geo = self._geo()
        m = torch.zeros(N, taps, Kc, dtype=torch.bool)
        if name == "dy":
            m[index[1]] = True                                   # dy[m, n]: every tap and input channel of out channel n
        elif name == "out":
            m[index[1], index[2], index[3]] = True
        elif taps == 1:
            m[:, 0, index[1]] = True                             # x[m, k]: input channel k of every out channel
        else:
            b, y, x, k = index
            for _oy, _ox, t in conv_readers(*geo[1:3], *geo[5:], y, x)[2]:
                m[:, t, k] = True
        return {"out": m}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        with tg.tn_names(L) as names:
            out = tg.run_tn(ob, self.c, inp)
        assert len(names) == 1 and tg.name_matches(names[0], tg.expected(self.c, dtype)), names
        self._splits = int(names[0].split("+split")[1]) if "+split" in names[0] else 1
        return {"out": out[0]}


GEMM_TN = [GemmTn("tn_lin_1x1"), GemmTn("tn_conv_1x1"), GemmTn("tn_reg_tiny"), GemmTn("tn_reg_pad0_acc"), GemmTn("tn_reg_s2"),
           GemmTn("tn_reg_split")]


# ------------------------------------------------------------------------------------------------ column sums

class Colsum(Case):
    family = "colsum"

    def __init__(self, rps, segs, N, scale, accumulate):
        self.rps, self.segs, self.N, self.scale, self.acc = rps, segs, N, scale, accumulate
        self.id = f"colsum_{rps}x{segs}x{N}" + ("_acc" if accumulate else "")

    def make(self, dtype, device):
        g = torch.Generator().manual_seed(self.rps + self.N)
        return {"x": _rnd(g, (self.segs * self.rps, self.N), dtype, device, 1.0, 0.25), "out0": _rnd(g, (self.segs, self.N), F32, device)}

    def plants(self):
        p = [("x", (self.segs * self.rps - 1, self.N - 1)), ("x", (0, 0))]       # the last row of the last chunk; the first
        return p + ([("out0", (self.segs - 1, 1))] if self.acc else [])

    def ref(self, inp, dtype):
        r, e = nb.colsum_ref(inp["x"], self.segs, self.scale, inp["out0"] if self.acc else None)
        return {"out": Ref(r, e, F32, nb.Where("cols", N=self.N), nb.check)}

    def declared(self, inp, name, index, value):
        m = torch.zeros(self.segs, self.N, dtype=torch.bool)
        if name == "x":
            m[index[0] // self.rps, index[1]] = True            # the column of that segment
        else:
            m[index[0], index[1]] = True
        return {"out": m}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        o1, o2 = inp["out0"].clone(), inp["out0"].clone()
        ob.colsum(inp["x"], segs=self.segs, out=o1, accumulate=self.acc, scale=self.scale)
        q = ob.ColsumQueue()
        q.add(inp["x"], o2, segs=self.segs, accumulate=self.acc, scale=self.scale)
        q.flush()
        return {"out": o1, "out/queue": o2}


COLSUM = [Colsum(1000, 3, 640, 0.25, True), Colsum(3000, 1, 640, 1.0, False), Colsum(64, 2, 264, 1.0, False)]


# ------------------------------------------------------------------------------------------------ GroupNorm

class GnFwd(Case):
    family = "groupnorm_fwd"

    def __init__(self, cid, B, HW, C, groups=32, silu=True, xf32=False):
        self.id, self.B, self.HW, self.C, self.groups, self.silu, self.xf32 = f"gn_fwd_{cid}", B, HW, C, groups, silu, xf32

    def make(self, dtype, device):
        g = torch.Generator().manual_seed(self.C + self.HW)
        x = _rnd(g, (self.B, self.HW, self.C), F32 if self.xf32 else dtype, device, 2.0, 0.5)
        return {"x": x, "gamma": _rnd(g, (self.C,), F32, device, 0.2, 1.0), "beta": _rnd(g, (self.C,), F32, device, 0.2)}

    def plants(self):
        return [("x", (self.B - 1, self.HW - 1, self.C - 1)), ("x", (0, 0, 0)), ("gamma", (self.C - 1,)), ("beta", (0,))]

    def ref(self, inp, dtype):
        r, e, mr, e_mr = nb.gn_fwd_ref(inp["x"], inp["gamma"], inp["beta"], self.groups, EPS, self.silu)
        ppc = nb.gn_geometry(self.B, self.HW, self.C)[1]
        return {"y": Ref(r, e, dtype, nb.Where("gn", HW=self.HW, C=self.C, groups=self.groups, ppc=ppc), nb.check),
                "mean_rstd": Ref(mr, e_mr, F32, nb.Where("stats", groups=self.groups), nb.check)}

    def declared(self, inp, name, index, value):
        cpg = self.C // self.groups
        y = torch.zeros(self.B, self.HW, self.C, dtype=torch.bool)
        mr = torch.zeros(self.B, self.groups, 2, dtype=torch.bool)
        if name == "x":
            b, _, c = index
            grp = c // cpg
            y[b, :, grp * cpg:(grp + 1) * cpg] = True           # the (image, group): every pixel, every channel of it
            mr[b, grp] = True
        else:
            y[:, :, index[0]] = True                            # gamma[c], beta[c]: channel c of every image
        return {"y": y, "mean_rstd": mr}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        y, mr = ops.groupnorm(inp["x"], inp["gamma"], inp["beta"], self.groups, EPS, silu=self.silu, return_stats=True,
                              out_dtype=dtype if self.xf32 else None)
        return {"y": y, "mean_rstd": mr}


class GnBwd(Case):
    """dfw_groupnorm_bwd from a given (mean, rstd) buffer (the fp64 statistics of the finite x rounded to fp32: an
    operand here, as in tests/norm_bound.gn_bwd_ref)."""
    family = "groupnorm_bwd"

    def __init__(self, cid, B, HW, C, groups=32, silu=True):
        self.id, self.B, self.HW, self.C, self.groups, self.silu = f"gn_bwd_{cid}", B, HW, C, groups, silu

    def make(self, dtype, device):
        g = torch.Generator().manual_seed(self.C + self.HW + 1)
        sh = (self.B, self.HW, self.C)
        x = _rnd(g, sh, dtype, device, 2.0, 0.5)
        mr = nb.gn_stats_ref(x, self.groups, EPS)[0].to(F32)
        return {"x": x, "dy": _rnd(g, sh, dtype, device), "mean_rstd": mr, "gamma": _rnd(g, (self.C,), F32, device, 0.2, 1.0),
                "beta": _rnd(g, (self.C,), F32, device, 0.2), "dx_add": _rnd(g, sh, dtype, device),
                "dgamma0": _rnd(g, (self.C,), F32, device), "dbeta0": _rnd(g, (self.C,), F32, device)}

    def plants(self):
        last = (self.B - 1, self.HW - 1, self.C - 1)
        return [("x", last), ("dy", last), ("dy", (0, 0, 0)), ("gamma", (self.C - 1,)), ("dx_add", last),
                ("mean_rstd", (self.B - 1, self.groups - 1, 0)), ("mean_rstd", (0, 0, 1)), ("dgamma0", (1,))]

    def ref(self, inp, dtype):
        out = nb.gn_bwd_ref(inp["x"], inp["dy"], inp["mean_rstd"], inp["gamma"], inp["beta"], self.groups, self.silu,
                            inp["dx_add"], inp["dgamma0"], inp["dbeta0"], 0.5)
        ppc = nb.gnb_geometry(self.B, self.HW, self.C)[1]
        whc = nb.Where("cols", N=self.C)
        return {"dx": Ref(*out["dx"], dtype, nb.Where("gn", HW=self.HW, C=self.C, groups=self.groups, ppc=ppc), nb.check),
                "dgamma": Ref(*out["dgamma"], F32, whc, nb.check), "dbeta": Ref(*out["dbeta"], F32, whc, nb.check)}

    def declared(self, inp, name, index, value):
        """xhat = (x - mean) rstd, dz = dy silu'(gamma xhat + beta) (dz = dy without SiLU); dbeta[c] = sum dz,
        dgamma[c] = sum dz xhat; dx = rstd (gamma dz - m1 - xhat m2) with m1, m2 the (image, group) means of gamma dz and
        gamma dz xhat."""
        cpg = self.C // self.groups
        dx = torch.zeros(self.B, self.HW, self.C, dtype=torch.bool)
        dg, db = torch.zeros(self.C, dtype=torch.bool), torch.zeros(self.C, dtype=torch.bool)

        def group(b, grp):
            dx[b, :, grp * cpg:(grp + 1) * cpg] = True

        if name == "x":                   # xhat at one element: dgamma[c]; through silu' also dz, so dbeta[c]; m2 of the group
            b, _, c = index
            group(b, c // cpg)
            dg[c] = True
            db[c] = self.silu
        elif name == "dy":                # dz at one element: both sums of channel c, both means of the group
            b, _, c = index
            group(b, c // cpg)
            dg[c] = db[c] = True
        elif name == "gamma":             # gamma[c] enters m1 / m2 of its group in every image; dgamma / dbeta only via silu'
            c = index[0]
            for b in range(self.B):
                group(b, c // cpg)
            dg[c] = db[c] = self.silu
        elif name == "dx_add":
            dx[tuple(index)] = True
        elif name == "mean_rstd":         # xhat of the whole (image, group)
            b, grp, _ = index
            group(b, grp)
            dg[grp * cpg:(grp + 1) * cpg] = True
            db[grp * cpg:(grp + 1) * cpg] = self.silu
        elif name == "dgamma0":
            dg[index[0]] = True
        return {"dx": dx, "dgamma": dg, "dbeta": db}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        dg, db = inp["dgamma0"].clone(), inp["dbeta0"].clone()
        dx = ob.groupnorm_bwd(inp["x"], inp["dy"], inp["mean_rstd"], inp["gamma"], inp["beta"], self.groups, self.silu, dg, db,
                              accumulate=True, grad_scale=0.5, dx_add=inp["dx_add"])
        return {"dx": dx, "dgamma": dg, "dbeta": db}


GROUPNORM = [GnFwd("one_chunk_ragged", 2, 100, 64), GnFwd("cpg2_nosilu", 2, 256, 64, silu=False),
             GnFwd("u320_64", 3, 64, 320), GnFwd("f32_one_chunk", 2, 100, 64, xf32=True),
             GnFwd("f32_u320_64_nosilu", 3, 64, 320, silu=False, xf32=True),
             GnBwd("one_chunk_ragged", 2, 100, 64), GnBwd("u320_64_nosilu", 3, 64, 320, silu=False)]


# ------------------------------------------------------------------------------------------------ LayerNorm

class LnFwd(Case):
    family = "layernorm_fwd"

    def __init__(self, rows, C, xf32=False):
        self.rows, self.C, self.xf32 = rows, C, xf32
        self.id = f"ln_fwd_{rows}x{C}" + ("_f32" if xf32 else "")

    def make(self, dtype, device):
        g = torch.Generator().manual_seed(self.rows * 7 + self.C)
        return {"x": _rnd(g, (self.rows, self.C), F32 if self.xf32 else dtype, device, 3.0, 1.0),
                "gamma": _rnd(g, (self.C,), F32, device, 0.5, 1.0), "beta": _rnd(g, (self.C,), F32, device, 0.2)}

    def plants(self):
        return [("x", (self.rows - 1, self.C - 1)), ("x", (0, 0)), ("gamma", (self.C - 1,)), ("beta", (0,))]

    def ref(self, inp, dtype):
        r, e = nb.ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"], EPS)
        return {"y": Ref(r, e, dtype, nb.Where("rows", C=self.C), nb.check)}

    def declared(self, inp, name, index, value):
        m = torch.zeros(self.rows, self.C, dtype=torch.bool)
        if name == "x":
            m[index[0]] = True
        else:
            m[:, index[0]] = True
        return {"y": m}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        return {"y": ops.layernorm(inp["x"], inp["gamma"], inp["beta"], EPS, out_dtype=dtype if self.xf32 else None)}


class LnBwd(Case):
    family = "layernorm_bwd"

    def __init__(self, rows, C):
        self.rows, self.C, self.id = rows, C, f"ln_bwd_{rows}x{C}"

    def make(self, dtype, device):
        g = torch.Generator().manual_seed(self.rows * 7 + self.C + 1)
        sh = (self.rows, self.C)
        return {"x": _rnd(g, sh, dtype, device, 3.0, 1.0), "dy": _rnd(g, sh, dtype, device),
                "gamma": _rnd(g, (self.C,), F32, device, 0.5, 1.0), "dx_add": _rnd(g, sh, dtype, device),
                "dgamma0": _rnd(g, (self.C,), F32, device), "dbeta0": _rnd(g, (self.C,), F32, device)}

    def plants(self):
        last = (self.rows - 1, self.C - 1)
        return [("x", last), ("dy", last), ("dy", (0, 0)), ("gamma", (self.C - 1,)), ("dx_add", last), ("dbeta0", (0,))]

    full_by_plant = {"gamma": ("dx",), "x": ("dgamma",)}

    def ref(self, inp, dtype):
        out = nb.ln_bwd_ref(inp["x"], inp["dy"], inp["gamma"], EPS, inp["dx_add"], inp["dgamma0"], inp["dbeta0"], 0.5)
        whc = nb.Where("cols", N=self.C)
        return {"dx": Ref(*out["dx"], dtype, nb.Where("rows", C=self.C), nb.check),
                "dgamma": Ref(*out["dgamma"], F32, whc, nb.check), "dbeta": Ref(*out["dbeta"], F32, whc, nb.check)}

    def declared(self, inp, name, index, value):
        """The statistics are recomputed from x: a planted x makes the whole row's xhat non-finite, so dgamma = sum dy xhat
        is non-finite in EVERY column (dbeta = sum dy in none); gamma[c] enters the row mean of gamma dy of every row, so
        all of dx (dgamma, dbeta do not read gamma)."""
        dx = torch.zeros(self.rows, self.C, dtype=torch.bool)
        dg, db = torch.zeros(self.C, dtype=torch.bool), torch.zeros(self.C, dtype=torch.bool)
        if name == "x":
            dx[index[0]] = True
            dg[:] = True
        elif name == "dy":
            dx[index[0]] = True
            dg[index[1]] = db[index[1]] = True
        elif name == "gamma":
            dx[:] = True
        elif name == "dx_add":
            dx[tuple(index)] = True
        elif name == "dbeta0":
            db[index[0]] = True
        return {"dx": dx, "dgamma": dg, "dbeta": db}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        dg, db = inp["dgamma0"].clone(), inp["dbeta0"].clone()
        dx = ob.layernorm_bwd(inp["x"], inp["dy"], inp["gamma"], dg, db, EPS, accumulate=True, grad_scale=0.5, dx_add=inp["dx_add"])
        return {"dx": dx, "dgamma": dg, "dbeta": db}


LAYERNORM = [LnFwd(3, 320), LnFwd(5, 1024), LnFwd(3, 2048), LnFwd(257, 64, xf32=True),
             LnBwd(3, 320), LnBwd(5, 1024), LnBwd(3, 2048)]


# ------------------------------------------------------------------------------------------------ pointwise and softmax

class Geglu(Case):
    family = "geglu"

    def __init__(self, rows, H, bwd):
        self.rows, self.H, self.bwd = rows, H, bwd
        self.id = f"geglu_{'bwd' if bwd else 'fwd'}_{rows}x{H}"

    def make(self, dtype, device):
        g = torch.Generator().manual_seed(self.rows + self.H)
        return {"pre": _rnd(g, (self.rows, 2 * self.H), dtype, device, 1.5), "dout": _rnd(g, (self.rows, self.H), dtype, device)}

    def plants(self):
        r, W = self.rows - 1, 2 * self.H
        p = [("pre", (r, 0)), ("pre", (r, W - 1)), ("pre", (0, 32))]       # a value column, the last gate column, a gate column
        return p + ([("dout", (r, 0)), ("dout", (r, self.H - 1))] if self.bwd else [])

    def ref(self, inp, dtype):
        if self.bwd:
            return {"dpre": Ref(*nb.geglu_bwd_ref(inp["pre"], inp["dout"]), dtype, nb.Where("rows", C=2 * self.H), nb.check)}
        return {"out": Ref(*nb.geglu_fwd_ref(inp["pre"]), dtype, nb.Where("rows", C=self.H), nb.check)}

    def declared(self, inp, name, index, value):
        """out = a gelu(g); d a = d gelu(g) (does not read a), d g = d a gelu'(g)."""
        r, j = index
        if name == "pre":
            grp, gate, o = j // 64, (j % 64) // 32, j % 32
            h = grp * 32 + o
        else:
            h = j
            grp, o = h // 32, h % 32
        va, ga = grp * 64 + o, grp * 64 + 32 + o
        if not self.bwd:
            m = torch.zeros(self.rows, self.H, dtype=torch.bool)
            m[r, h] = True
            return {"out": m}
        m = torch.zeros(self.rows, 2 * self.H, dtype=torch.bool)
        m[r, ga] = True
        if name == "dout" or gate:
            m[r, va] = True
        return {"dpre": m}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        return {"dpre": ob.geglu_bwd(inp["pre"], inp["dout"])} if self.bwd else {"out": ob.geglu_fwd(inp["pre"])}


class Elementwise(Case):
    """The four dfw_elementwise modes (add, slice_channels, zero_stuff2x, pool2x2_sum) and silu_kernel (forward, backward)."""
    SLICE = (64, 128)            # slice_channels(a, c0, C)

    def __init__(self, mode):
        self.mode, self.id = mode, f"ew_{mode}"
        self.family = "silu" if mode.startswith("silu") else "elementwise"
        self.shape = (2, 6, 6, 320) if mode in ("pool2x2", "zero_stuff2x") else (3, 100, 320)

    def make(self, dtype, device):
        g = torch.Generator().manual_seed(len(self.mode))
        return {"a": _rnd(g, self.shape, dtype, device, 3.0), "b": _rnd(g, self.shape, dtype, device)}

    def plants(self):
        last = tuple(n - 1 for n in self.shape)
        first = tuple(0 for _ in self.shape)
        if self.mode == "slice_channels":          # the first and the last element inside the slice
            c0, Cc = self.SLICE
            return [("a", first[:-1] + (c0,)), ("a", last[:-1] + (c0 + Cc - 1,))]
        return [("a", first), ("a", last)] + ([("b", last)] if self.mode in ("add", "silu_grad") else [])

    def _copy_ref(self, a):
        """slice_channels and zero_stuff2x move 16-bit values unchanged: the reference is the value itself, allowance 0."""
        if self.mode == "slice_channels":
            r = a[..., self.SLICE[0]:self.SLICE[0] + self.SLICE[1]].to(F64)
        else:
            B, H, W, C = a.shape
            r = torch.zeros(B, 2 * H, 2 * W, C, dtype=F64, device=a.device)
            r[:, ::2, ::2] = a.to(F64)
        return r, torch.zeros_like(r)

    def ref(self, inp, dtype):
        a, b = inp["a"], inp["b"]
        r, e = {"add": lambda: nb.add_ref(a, b), "pool2x2": lambda: nb.pool2x2_ref(a), "silu": lambda: nb.silu_ref(a),
                "silu_grad": lambda: nb.silu_ref(a, b), "slice_channels": lambda: self._copy_ref(a),
                "zero_stuff2x": lambda: self._copy_ref(a)}[self.mode]()
        return {"y": Ref(r, e, dtype, nb.Where("rows", C=r.shape[-1]), nb.check)}

    def declared(self, inp, name, index, value):
        if self.mode == "pool2x2":
            B, H2, W2, C = self.shape
            m = torch.zeros(B, H2 // 2, W2 // 2, C, dtype=torch.bool)
            m[index[0], index[1] // 2, index[2] // 2, index[3]] = True
        elif self.mode == "slice_channels":
            m = torch.zeros(*self.shape[:-1], self.SLICE[1], dtype=torch.bool)
            m[tuple(index[:-1]) + (index[-1] - self.SLICE[0],)] = True
        elif self.mode == "zero_stuff2x":
            B, H, W, C = self.shape
            m = torch.zeros(B, 2 * H, 2 * W, C, dtype=torch.bool)
            m[index[0], 2 * index[1], 2 * index[2], index[3]] = True
        else:
            m = torch.zeros(self.shape, dtype=torch.bool)
            m[tuple(index)] = True
        return {"y": m}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        a, b = inp["a"], inp["b"]
        return {"y": {"add": lambda: ob.add(a, b), "pool2x2": lambda: ob.pool2x2_sum(a), "silu": lambda: ob.silu(a),
                      "silu_grad": lambda: ob.silu(a, b), "slice_channels": lambda: ob.slice_channels(a, *self.SLICE),
                      "zero_stuff2x": lambda: ob.zero_stuff2x(a)}[self.mode]()}


class SoftmaxRows(Case):
    family = "softmax"
    value_dependent = True
    SCALE = 0.3

    def __init__(self, Lr):
        self.L, self.id = Lr, f"softmax_rows_L{Lr}"

    def make(self, dtype, device):
        g = torch.Generator().manual_seed(self.L)
        return {"x": _rnd(g, (5, self.L), F32, device, 4.0)}

    def plants(self):
        return [("x", (4, 0)), ("x", (4, self.L - 1)), ("x", (0, self.L // 2))]

    def masked(self, name, index, value):
        return value == -math.inf

    def ref(self, inp, dtype):
        return {"y": Ref(*nb.softmax_rows_ref(inp["x"], self.SCALE, nonfinite=True), dtype, nb.Where("rows", C=self.L), nb.check)}

    def declared(self, inp, name, index, value):
        m = torch.zeros(5, self.L, dtype=torch.bool)
        if not self.masked(name, index, value):
            m[index[0]] = True                                  # the row
        return {"y": m}

    def run(self, env, inp, dtype):
        return {"y": env[0].softmax_rows(inp["x"], dtype, scale=self.SCALE)}


class SoftmaxGroups(Case):
    family = "softmax"
    value_dependent = True

    def __init__(self, rows, ld, groups, Lg):
        self.rows, self.ld, self.groups, self.Lg = rows, ld, groups, Lg
        self.id = f"softmax_groups_{rows}x{ld}_{groups}x{Lg}"

    def make(self, dtype, device):
        return {"x": _rnd(torch.Generator().manual_seed(self.rows), (self.rows, self.ld), F32, device, 3.0)}

    def plants(self):
        last = self.groups * self.Lg - 1
        return [("x", (self.rows - 1, last)), ("x", (self.rows - 1, last - self.Lg + 1)), ("x", (0, 0))]   # the last group: its ends

    def masked(self, name, index, value):
        return value == -math.inf

    def ref(self, inp, dtype):
        return {"y": Ref(*nb.softmax_groups_ref(inp["x"], self.groups, self.Lg, nonfinite=True), dtype,
                         nb.Where("rows", C=self.ld), nb.check)}

    def declared(self, inp, name, index, value):
        m = torch.zeros(self.rows, self.ld, dtype=torch.bool)
        if not self.masked(name, index, value):
            grp = index[1] // self.Lg
            m[index[0], grp * self.Lg:(grp + 1) * self.Lg] = True
        return {"y": m}

    def run(self, env, inp, dtype):
        return {"y": env[0].softmax_groups(inp["x"], self.groups, self.Lg, dtype)}


POINTWISE = [Geglu(3, 32, False), Geglu(500, 256, False), Geglu(3, 32, True), Geglu(500, 256, True),
             Elementwise("add"), Elementwise("slice_channels"), Elementwise("zero_stuff2x"), Elementwise("pool2x2"), Elementwise("silu"), Elementwise("silu_grad"),
             SoftmaxRows(4), SoftmaxRows(1020), SoftmaxRows(4098), SoftmaxRows(264),
             SoftmaxGroups(33, 128, 3, 8), SoftmaxGroups(7, 64, 1, 64), SoftmaxGroups(300, 64, 10, 4)]


# ------------------------------------------------------------------------------------------------ loss and sumsq

class Mse(Case):
    family = "loss"
    SHAPE = (1, 3, 7, 5)

    def __init__(self, grad_only=False):
        self.grad_only, self.id = grad_only, "loss_grad" if grad_only else "mse_loss"
        self.full = () if grad_only else ("loss",)

    def make(self, dtype, device):
        g = torch.Generator().manual_seed(16)
        return {"pred": _rnd(g, self.SHAPE, F32, device), "target": _rnd(g, self.SHAPE, F32, device)}

    def plants(self):
        last = tuple(n - 1 for n in self.SHAPE)
        return [("pred", last), ("pred", (0, 0, 0, 0))] + ([] if self.grad_only else [("target", last)])

    def ref(self, inp, dtype):
        if self.grad_only:
            return {"dpred": Ref(*nb.loss_grad_ref(inp["pred"], 0.37), dtype)}
        (lr, le), (gr, ge) = nb.mse_ref(inp["pred"], inp["target"], 8.0)
        return {"loss": Ref(lr, le, F32), "dpred": Ref(gr, ge, dtype)}

    def declared(self, inp, name, index, value):
        m = torch.zeros(self.SHAPE, dtype=torch.bool)
        m[tuple(index)] = True
        return {"dpred": m} if self.grad_only else {"loss": torch.ones(1, dtype=torch.bool), "dpred": m}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        Cc = self.SHAPE[1]
        nchw = torch.empty(self.SHAPE, device=inp["pred"].device)
        if self.grad_only:
            dp = ob.loss_grad(inp["pred"], dtype, scale=0.37, dpred_nchw_out=nchw)
            return {"dpred": dp[..., :Cc].permute(0, 3, 1, 2), "dpred/nchw": nchw}
        loss, dp = ob.mse_loss(inp["pred"], inp["target"], dtype, loss_scale=8.0, dpred_nchw_out=nchw)
        return {"loss": loss, "dpred": dp[..., :Cc].permute(0, 3, 1, 2), "dpred/nchw": nchw}


class Sumsq(Case):
    """dfw_sumsq: 1024 blocks x 256 threads x 4 floats = 1 048 576 elements per grid-stride trip."""
    family = "sumsq"
    dtypes = (F32,)
    full = ("out",)
    TRIP = 1024 * 256 * 4

    def __init__(self, n):
        self.n, self.id = n, f"sumsq_n{n}"

    def make(self, dtype, device):
        return {"x": _rnd(torch.Generator().manual_seed(self.n), (self.n,), F32, device, 3.0)}

    def plants(self):
        n = self.n
        p = [("x", (0,)), ("x", (n // 4 * 4 - 1,)), ("x", (n - 1,))]        # first; last of the 4-wide body; the scalar tail
        return p + ([("x", (self.TRIP + 5,))] if n > self.TRIP else [])     # the second grid-stride trip

    def ref(self, inp, dtype):
        return {"out": Ref(*nb.sumsq_ref(inp["x"]), F32)}

    def declared(self, inp, name, index, value):
        return {"out": torch.ones(1, dtype=torch.bool)}

    def run(self, env, inp, dtype):
        return {"out": env[1].sumsq(inp["x"])}


LOSS = [Mse(), Mse(grad_only=True), Sumsq(100_003), Sumsq(Sumsq.TRIP + 1027)]


# ------------------------------------------------------------------------------------------------ store overflow (fp16)

def _search_scale(row_of, lo=1.0, hi=6.0e4, steps=80):
    """Smallest f of a geometric grid for which row_of(f) (the fp64 results that depend on f) has an element above the
    fp16 range and none in the forbidden band [65504 / 2, 65520 (1 + 2^-8)]: a result is either well inside the range or
    rounds to inf whatever the kernel's fp32 rounding."""
    for i in range(steps + 1):
        f = lo * (hi / lo) ** (i / steps)
        a = row_of(f).abs()
        over = a > F16_INF_FROM * (1 + 2.0 ** -8)
        if bool(over.any()) and not bool(((a >= F16_MAX / 2) & ~over).any()):
            return f
    raise AssertionError("no scale puts the row outside the forbidden band")


class OverflowCase(Case):
    """Finite fp16 operands whose exact result exceeds 65520 at chosen output elements: the store must give inf of the
    right sign there (IEEE round-to-nearest-even), and every other element -- below 65504 / 2 -- stays inside its bound."""
    dtypes = (F16,)
    overflow = True
    okey = "y"               # the output whose elements leave the fp16 range

    def plants(self):
        return [(None, (), None)]


class GemmOverflow(OverflowCase, GemmFwd):
    """Row `row` of A (a linear's input row; a conv's nine input pixels under one output pixel) is replaced by
    f sign(W[n0]): output (row, n0) is f sum |W[n0]|, the rest of the row f times a random-sign sum."""
    family = "store_overflow"

    def __init__(self, source, cid):
        GemmFwd.__init__(self, source, cid, None)
        self.id = f"overflow/{self.id}"

    def make(self, dtype, device):
        c = self.c
        inp = GemmFwd.make(self, dtype, device)
        M, N, K, rpi, Ho, Wo, imgs = self.dims()
        x, w = inp["x"].clone(), inp["w"]
        n0 = 5
        sgn = torch.sign(w[n0].float())
        if c.op == "linear":
            row = M - 1
            unit = sgn.clone()
            put = lambda f: x.__setitem__(row, (f * unit).to(dtype))
            rows = [row]
        else:
            B, H, W, Cin = c.shape[:4]
            assert c.shape[5:] == (1, 1, False)
            oy, ox = Ho - 2, Wo - 2                                            # interior: all nine taps inside the map
            unit = sgn.reshape(3, 3, Cin)
            put = lambda f: x[B - 1].__setitem__((slice(oy - 1, oy + 2), slice(ox - 1, ox + 2)), (f * unit).to(dtype))
            rows = [(B - 1) * Ho * Wo + (oy + dy) * Wo + ox + dx for dy in (-2, -1, 0, 1, 2) for dx in (-2, -1, 0, 1, 2)
                    if oy + dy < Ho and ox + dx < Wo]
        keep = torch.tensor(rows, device=x.device)

        # S is linear in f on the dependent rows: two references (f = 0, f = 1), then only those rows' epilogue per trial
        def sums(f):
            put(f)
            S, A = eb.gemm_ref(x, w) if c.op == "linear" else eb.conv_ref(x, w, *c.shape[5:])
            return S[keep], A[keep]

        (S0, A0), (S1, A1) = sums(0.0), sums(1.0)
        add = torch.zeros_like(S0)
        if "res" in inp:
            add = add + inp["res"].reshape(M, N)[keep].to(F64)
        if "rowbias" in inp:
            add = add + inp["rowbias"].to(F64)[keep // rpi]

        def row_of(f):
            fr = float(torch.tensor(f).to(dtype))
            return eb.epilogue_ref(S0 + fr * (S1 - S0), A0 + fr * (A1 - A0), K, bias=inp.get("bias"), residual=add,
                                   out_scale=c.scale, colscale=c.colscale, act=c.act, geglu=c.geglu)[0]

        put(_search_scale(row_of))
        inp["x"] = x
        return inp

    def declared(self, inp, name, index, value):
        return None


GEMM_OVERFLOW = [GemmOverflow("gemm", "gk_splitk_silu"), GemmOverflow("gemm", "gk_conv_splitk"),
                 GemmOverflow("gemm8", "g8_256x256_geglu"), GemmOverflow("gemm_big", "big256x128x32_lin"),
                 GemmOverflow("conv_patch8", "cp8_256x128_ragged_gn"), GemmOverflow("conv_patch", "cp512x128_wblk")]


class NormOverflow(OverflowCase):
    """GroupNorm / LayerNorm with gamma[c0] scaled: xhat gamma exceeds the fp16 range where |xhat| is large in channel c0."""
    family = "store_overflow"

    def __init__(self, base):
        self.base, self.id = base, f"overflow/{base.id}"

    def make(self, dtype, device):
        inp = self.base.make(dtype, device)
        c0 = 3
        gamma = inp["gamma"].clone()

        def row_of(f):
            gamma[c0] = f
            return self.base.ref(dict(inp, gamma=gamma), dtype)["y"].r[..., c0]

        gamma[c0] = _search_scale(row_of, 1e3, 1e8)
        inp["gamma"] = gamma
        return inp

    def ref(self, inp, dtype):
        return {"y": self.base.ref(inp, dtype)["y"]}

    def run(self, env, inp, dtype):
        return {"y": self.base.run(env, inp, dtype)["y"]}


class NormBwdOverflow(OverflowCase):
    """LayerNorm / GroupNorm backward with gamma[c0] scaled: dx = rstd (gamma dz - m1 - xhat m2) exceeds the fp16 range in
    channel c0 (gamma dz itself), while the means m1, m2 carry the scaled term divided by the row's (group's) size."""
    family = "store_overflow"
    okey = "dx"

    def __init__(self, base):
        self.base, self.id = base, f"overflow/{base.id}"

    def make(self, dtype, device):
        inp = self.base.make(dtype, device)
        gamma = inp["gamma"].clone()

        def row_of(f):
            gamma[3] = f
            return self.base.ref(dict(inp, gamma=gamma), dtype)["dx"].r

        gamma[3] = _search_scale(row_of, 1e3, 1e8)
        inp["gamma"] = gamma
        return inp

    def ref(self, inp, dtype):
        return self.base.ref(inp, dtype)

    def run(self, env, inp, dtype):
        return self.base.run(env, inp, dtype)


NORM_OVERFLOW = [NormOverflow(GnFwd("one_chunk_ragged", 2, 100, 64, silu=False)), NormOverflow(LnFwd(3, 320)),
                 NormBwdOverflow(LnBwd(3, 320)), NormBwdOverflow(GnBwd("one_chunk_ragged", 2, 100, 64))]


# ------------------------------------------------------------------------------------------------ attention forward

import attention_bound as ab               # noqa: E402
import test_attention_plans_gpu as ta      # noqa: E402

LOG2E = math.log2(math.e)


def _sign_up(qcol, value):
    """Rows whose score against a key planted with `value` (inf or NaN) in one column is +inf or NaN: the planted product
    q_ic k_jc is +inf where the signs agree, NaN where q_ic == 0 (and always for a NaN); -inf otherwise: a masked key."""
    if value != value:
        return torch.ones(qcol.shape, dtype=torch.bool)
    return (qcol.double() * (1.0 if value > 0 else -1.0) >= 0).cpu()


class AttnFwd(Case):
    """kind 'fsa': one Fsa case of tests/test_attention_plans_gpu.py (its planned launch asserted); 'xattn': ops.cross_attention;
    'vattn': ops.vae_attention.  Outputs: y [B, n, heads * D] and, for fsa, lse [B, heads, n]."""
    family = "attention_fwd"
    value_dependent = True

    def __init__(self, kind, cid, far_below=False):
        self.kind, self.far = kind, far_below
        table = {"fsa": ta.FSA_CASES, "xattn": ta.XA_CASES, "vattn": ta.VA_CASES}[kind]
        self.c = next(c for c in table if c.id == cid)
        self.id = f"{kind}_{cid}"
        c = self.c
        self.H, self.D = (1, 512) if kind == "vattn" else (c.heads, 64)
        self.n_q = c.N if kind == "vattn" else c.n_q
        self.n_kv = c.N if kind == "vattn" else (c.L if kind == "xattn" else c.n_kv)
        self.nshot, self.n_plain, self.n_bank = (c.nshot, c.n_plain, c.n_bank) if kind == "fsa" else (0, 0, 0)
        # one image, one head: a NaN key reaches every row there is (an infinite one still leaves the masked rows finite)
        self.full_by_plant = {"k": ("y", "lse")} if c.B == 1 and self.H == 1 else {}

    def make(self, dtype, device):
        seed = sum(map(ord, self.c.id))
        if self.kind == "fsa":
            inp = ta.make_fsa_inputs(self.c, dtype, device, seed=seed)
            del inp["lse"]
            if self.nshot and not self.n_bank:
                del inp["kb"], inp["vb"]                    # lock-step: the bank IS k[:n_plain] / v[:n_plain] (see _full)
            return inp
        if self.kind == "xattn":
            q, k, v, _ = ta.make_xa_inputs(self.c, dtype, device, seed=seed)
        else:
            q, k, v = ta.make_va_inputs(self.c, dtype, device, seed=seed)
        return {"q": q, "k": k, "v": v}

    def _full(self, inp):
        if self.nshot and not self.n_bank:
            return dict(inp, kb=inp["k"][:self.n_plain], vb=inp["v"][:self.n_plain])
        return inp

    def plants(self):
        B, C, nq, nk = self.c.B, self.H * self.D, self.n_q, self.n_kv
        if self.far:          # keys of the first tile: ~180 log2 units below the row maximum of the rising ramp
            return [("k", (0, 3, 5)), ("v", (0, 3, 5))]
        p = [("q", (B - 1, nq - 1, C - 1)), ("k", (B - 1, 0, 0)), ("k", (B - 1, nk - 1, C - 1)), ("v", (B - 1, nk - 1, C - 1)),
             ("v", (0, 0, 1))]
        if self.nshot and self.n_bank:
            nbank = (B - self.n_plain) * self.nshot
            p += [("kb", (nbank - 1, self.n_bank - 1, C - 1)), ("vb", (0, 0, 0))]
        elif self.nshot:
            p += [("k", (0, nk - 1, 1)), ("v", (self.n_plain - 1, 0, C - 1))]      # support images: bank keys of the queries
        return p

    def _c(self):
        if self.kind == "xattn":
            return 64 ** -0.5 * LOG2E
        return 1.0 if self.kind == "vattn" or self.c.pre else 64 ** -0.5 * LOG2E

    def ref(self, inp, dtype):
        inp = self._full(inp)
        c, H, D, n = self.c, self.H, self.D, self.n_q
        q = inp["q"]
        dev = q.device
        r = torch.empty(c.B, n, H * D, dtype=F64, device=dev)
        e = torch.empty_like(r)
        lr = torch.empty(c.B, H, n, dtype=F64, device=dev)
        le = torch.empty_like(lr)
        nsplit = getattr(self, "_nsplit", 1)
        kw = dict(round_p=False, tile=1, xattn=True) if self.kind == "xattn" else (dict(tile=32) if self.kind == "vattn" else {})
        for b in range(c.B):
            segs = ab.key_segments(inp["k"], inp["v"], b, self.n_plain, self.nshot, inp.get("kb"), inp.get("vb"))
            ns = nsplit if (self.nshot and b >= self.n_plain) else 1
            for h in range(H):
                sl = slice(h * D, (h + 1) * D)
                K = torch.cat([s[1][:, sl] for s in segs])
                V = torch.cat([s[2][:, sl] for s in segs])
                r[b, :, sl], e[b, :, sl], lr[b, h], le[b, h] = ab.fwd_ref(q[b][:, sl], K, V, dtype, c=self._c(), nsplit=ns,
                                                                          nonfinite=True, **kw)
        rows = 256 if (self.kind == "fsa" and ",8,1," in c.expect) else 128
        out = {"y": Ref(r, e, dtype, ab.Where(n, H, rows, D=D), ab.check)}
        if self.kind == "fsa":
            out["lse"] = Ref(lr, le, F32, ab.Where(n, H, rows, lse=True), ab.check)
        return out

    def _readers(self, name, img):
        """Batch entries whose key order holds image `img` of operand `name` (k / v: own keys; the bank's: its queries)."""
        if name in ("kb", "vb"):
            return [self.n_plain + img // self.nshot]
        out = [img]
        if self.nshot and not self.n_bank and img < self.n_plain:
            out.append(self.n_plain + img // self.nshot)
        return out

    def declared(self, inp, name, index, value):
        """s_ij = c q_i.k_j, P = softmax, y_i = sum_j P_ij v_j.  q[b, i, c]: row i of that image and head (its scores are
        +-inf by the sign of k_jc, the maximum is +inf, every s - m is NaN or -inf: the row is NaN).  A key: every query row
        of every image that reads it -- for +-inf only the rows whose q_ic makes the score +inf (or NaN); where it is -inf
        the key is masked and the row stays finite.  A value: column c of those rows (lse does not read v)."""
        c, H, D, n = self.c, self.H, self.D, self.n_q
        y = torch.zeros(c.B, n, H * D, dtype=torch.bool)
        lse = torch.zeros(c.B, H, n, dtype=torch.bool)
        b, i, col = index
        h = col // D
        sl = slice(h * D, (h + 1) * D)
        if name == "q":
            y[b, i, sl] = True
            lse[b, h, i] = True
        else:
            for rb in self._readers(name, b):
                if name in ("k", "kb"):
                    up = _sign_up(inp["q"][rb, :, col], value)
                    y[rb, :, sl] = up[:, None]
                    lse[rb, h] = up
                else:
                    y[rb, :, col] = True
        return {"y": y, "lse": lse} if self.kind == "fsa" else {"y": y}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        inp = self._full(inp)
        c = self.c
        if self.kind == "xattn":
            return {"y": ops.cross_attention(inp["q"], inp["k"], inp["v"], c.heads)}
        if self.kind == "vattn":
            return {"y": ops.vae_attention(inp["q"], inp["k"], inp["v"])}
        lse = torch.empty(c.B, c.heads, c.n_q, dtype=F32, device=inp["q"].device)
        want = ta.expected(c, dtype)
        with ta.configured(L, c.cfg), ta.fsa_names(ops, L) as names:
            y = ta.run_fsa(ops, c, dict(inp, lse=lse))
        assert names == [want], names
        self._nsplit = int(want.split("+split")[1]) if "+split" in want else 1
        return {"y": y, "lse": lse}


ATTN_FWD = [AttnFwd("fsa", "nq129_nkv65_scale"),               # NW 4, scale, last key tile of 1 key
            AttnFwd("fsa", "nq17_nkv127_heads10"),             # NW 4, pre, last key tile of 63 keys
            AttnFwd("fsa", "nshot0_nq1025_nw8"),               # NW 8, pre
            AttnFwd("fsa", "nq1151_nkv1087_nw8_scale"),        # NW 8, scale
            AttnFwd("fsa", "lockstep_shot1_scale"),            # lock-step bank
            AttnFwd("fsa", "twopass_shot2_nbank321"),          # two-pass bank, n_bank != n_kv
            AttnFwd("fsa", "twopass_shot2_split3"),            # key split on (two-pass)
            AttnFwd("fsa", "lockstep_shot7_forced3"),          # key split on (lock-step)
            AttnFwd("fsa", "ramp+12_pre", far_below=True),     # the planted key ~180 log2 units below the row maximum
            AttnFwd("xattn", "L77"), AttnFwd("vattn", "B9_N100")]


# ------------------------------------------------------------------------------------------------ attention backward

class AttnBwdBase(Case):
    """Flash backward from given out / lse (the fp64 forward of the finite operands, rounded: operands here, as in
    attention_bound.bwd_ref).  P_ij = 2^(s_ij - lse_i), dP_ij = dO_i.v_j, delta_i = dO_i.O_i, dS = P (dP - delta);
    dq_i = scale sum_j dS_ij k_j, dk_j = ln2 sum_i dS_ij q_i, dv_j = sum_i P_ij dO_i.

    An infinite q or k gives P = 2^(+-inf) = inf or 0 by the sign of each single product q_ic k_jc: where it is inf ("up")
    dS and everything it feeds is non-finite; where it is 0 dS = 0 exactly and only 0 x inf remains, in the plant's own
    column.  +inf in the stored lse is a mask: P = 0, every gradient finite.  The references' allowances hold 0 x inf on
    these operands, so for +-inf in q, k and +inf in lse the finite elements are only required to be finite
    (bound_applies); dout, v, NaN and lse = -inf keep the full bound."""
    family = "attention_bwd"
    value_dependent = True

    def _sub(self, name, index):
        return getattr(self, "_what", lambda n, i: n)(name, index)

    def masked(self, name, index, value):
        return self._sub(name, index) == "lse" and value == math.inf

    def bound_applies(self, name, index, value):
        return not (self._sub(name, index) in ("q", "k", "lse") and abs(value) == math.inf)

    def _fwd(self, q, segs_of, B, H, n, dtype):
        out = torch.empty(B, n, H * 64, dtype=dtype, device=q.device)
        lse = torch.empty(B, H, n, dtype=F32, device=q.device)
        for b in range(B):
            segs = segs_of(b)
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                K = torch.cat([s[1][:, sl] for s in segs])
                V = torch.cat([s[2][:, sl] for s in segs])
                r, _, lr, _ = ab.fwd_ref(q[b][:, sl], K, V, dtype)
                out[b, :, sl], lse[b, h] = r.to(dtype), lr.to(F32)
        return out, lse


class FsaBwd(AttnBwdBase):
    """dfw_fsa_attention_bwd on a fused qkv [Bt, N, 3C] (lock-step [support ; query] batch)."""

    def __init__(self, cid):
        self.c = next(c for c in ta.FSA_BWD_CASES if c.id == cid)
        self.id = f"fsa_bwd_{cid}"
        c = self.c
        self.n_plain = c.b * c.nshot
        self.Bt, self.C = self.n_plain + c.b, c.heads * 64

    def _segs(self, qkv, b):
        C = self.C
        k, v = qkv[..., C:2 * C], qkv[..., 2 * C:]
        return ab.key_segments(k, v, b, self.n_plain, self.c.nshot, k, v)

    def make(self, dtype, device):
        c, C = self.c, self.C
        g = torch.Generator().manual_seed(sum(map(ord, c.id)))
        qkv = torch.randn(self.Bt, c.N, 3 * C, generator=g)
        qkv[..., :C] *= ta.QSCALE * 2
        qkv = qkv.to(dtype).to(device)
        dout = torch.randn(self.Bt, c.N, C, generator=g).to(dtype).to(device)
        out, lse = self._fwd(qkv[..., :C], lambda b: self._segs(qkv, b), self.Bt, c.heads, c.N, dtype)
        return {"qkv": qkv, "out": out, "dout": dout, "lse": lse}

    def _what(self, name, index):
        return ("q", "k", "v")[index[2] // self.C] if name == "qkv" else name

    def plants(self):
        c, C, B = self.c, self.C, self.Bt
        last = (B - 1, c.N - 1)
        p = [("dout", last + (C - 1,)), ("qkv", last + (3 * C - 1,)), ("qkv", (0, 0, 2 * C)), ("lse", (B - 1, c.heads - 1, c.N - 1)),
             ("qkv", last + (C - 1,)), ("qkv", last + (2 * C - 1,)), ("qkv", (0, c.N - 1, C))]
        return p

    def ref(self, inp, dtype):
        c, C, Bt, N, H = self.c, self.C, self.Bt, self.c.N, self.c.heads
        qkv = inp["qkv"]
        q = qkv[..., :C]
        dev = qkv.device
        accs = [[ab.BwdAcc(N, 64, dev) for _ in range(H)] for _ in range(Bt)]
        dq = torch.empty(Bt, N, C, dtype=F64, device=dev)
        edq = torch.empty_like(dq)
        splits = getattr(self, "_splits", 1)
        for b in range(Bt):
            segs = self._segs(qkv, b)
            ns = splits if (c.nshot and b >= self.n_plain) else 1
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                dq[b, :, sl], edq[b, :, sl] = ab.bwd_ref(q[b][:, sl], [(K[:, sl], V[:, sl], accs[img][h]) for img, K, V in segs],
                                                         inp["out"][b][:, sl], inp["dout"][b][:, sl], inp["lse"][b, h], dtype,
                                                         dq_splits=ns)
        dk, edk, dv, edv = (torch.empty_like(dq) for _ in range(4))
        for b in range(Bt):
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                dk[b, :, sl], edk[b, :, sl], dv[b, :, sl], edv[b, :, sl] = accs[b][h].finish()
        return {"dq": Ref(dq, edq, dtype, ab.Where(N, H, 128), ab.check),
                "dk": Ref(dk, edk, dtype, ab.Where(N, H, 64, what="key"), ab.check),
                "dv": Ref(dv, edv, dtype, ab.Where(N, H, 64, what="key"), ab.check)}

    def _keys_of(self, b):
        """Key images batch entry b reads."""
        out = [b]
        if self.c.nshot and b >= self.n_plain:
            out += [(b - self.n_plain) * self.c.nshot + s for s in range(self.c.nshot)]
        return out

    def _readers(self, img):
        out = [img]
        if self.c.nshot and img < self.n_plain:
            out.append(self.n_plain + img // self.c.nshot)
        return out

    def declared(self, inp, name, index, value):
        C, Bt, N = self.C, self.Bt, self.c.N
        dq, dk, dv = (torch.zeros(Bt, N, C, dtype=torch.bool) for _ in range(3))
        what = self._what(name, index)
        if what == "lse":
            b, h, i = index
            col = h * 64
        else:
            b, i, col = index
            col %= C
        sl = slice(col // 64 * 64, col // 64 * 64 + 64)
        inf = abs(value) == math.inf
        qkv = inp["qkv"]
        if what == "lse" and value == math.inf:
            pass
        elif what == "q" and inf:
            anyup = False
            for img in self._keys_of(b):
                up = _sign_up(qkv[img, :, C + col], value)
                dk[img, :, sl], dv[img, :, sl] = up[:, None], up[:, None]
                dk[img, :, col] = True
                anyup = anyup or bool(up.any())
            dq[b, i, sl] = anyup
        elif what == "k" and inf:
            anyup = False
            for rb in self._readers(b):
                up = _sign_up(qkv[rb, :, col], value)
                dq[rb, :, sl] = up[:, None]
                dq[rb, :, col] = True
                anyup = anyup or bool(up.any())
            dk[b, i, sl] = dv[b, i, sl] = anyup
        elif what in ("dout", "lse", "q"):     # row i: dS_i: (dout: through dP and delta), so dq_i and dk of every key it reads
            dq[b, i, sl] = True
            for img in self._keys_of(b):
                dk[img, :, sl] = True
                if what == "dout":
                    dv[img, :, col] = True      # dv_j = sum_i P_ij dO_i: column c
                else:
                    dv[img, :, sl] = True       # P_i: itself
        else:                                   # key j: dS_:j of every row that reads it, so their dq and dk_j (k: dv_j too)
            for rb in self._readers(b):
                dq[rb, :, sl] = True
            dk[b, i, sl] = True
            if what == "k":
                dv[b, i, sl] = True
        return {"dq": dq, "dk": dk, "dv": dv}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        c, C = self.c, self.C
        with ta.configured(L, c.cfg):
            self._splits = ta.fsa_bwd_splits(L, c, L.BF16 if dtype == BF16 else L.F16)
            assert self._splits == c.splits
            d = ob.fsa_attention_bwd(inp["qkv"], inp["out"], inp["dout"], inp["lse"], c.heads, nshot=c.nshot,
                                     n_plain=self.n_plain, key_split=c.key_split)
        return {"dq": d[..., :C], "dk": d[..., C:2 * C], "dv": d[..., 2 * C:]}


class AttnBwd(AttnBwdBase):
    """dfw_attention_bwd: q in its own tensor, k / v column slices of one kv buffer [B, L, 2C + 64]."""

    def __init__(self, cid):
        self.c = next(c for c in ta.ATTN_BWD_CASES if c.id == cid)
        self.id, self.C = f"attn_bwd_{cid}", self.c.heads * 64

    def make(self, dtype, device):
        c, C = self.c, self.C
        g = torch.Generator().manual_seed(sum(map(ord, c.id)))
        q = (torch.randn(c.B, c.n_q, C, generator=g) * ta.QSCALE * 2).to(dtype).to(device)
        kv = torch.randn(c.B, c.n_kv, 2 * C + 64, generator=g).to(dtype).to(device)
        dout = torch.randn(c.B, c.n_q, C, generator=g).to(dtype).to(device)
        out, lse = self._fwd(q, lambda b: [(b, kv[b][:, :C], kv[b][:, C:2 * C])], c.B, c.heads, c.n_q, dtype)
        return {"q": q, "kv": kv, "out": out, "dout": dout, "lse": lse}

    def _what(self, name, index):
        return ("k", "v")[index[2] // self.C] if name == "kv" else name

    def plants(self):
        c, C = self.c, self.C
        last = (c.B - 1, c.n_q - 1)
        return [("dout", last + (C - 1,)), ("kv", (c.B - 1, c.n_kv - 1, 2 * C - 1)), ("kv", (0, 0, C)),
                ("lse", (c.B - 1, c.heads - 1, c.n_q - 1)), ("q", last + (C - 1,)), ("kv", (c.B - 1, c.n_kv - 1, C - 1))]

    def ref(self, inp, dtype):
        c, C, H = self.c, self.C, self.c.heads
        dev = inp["q"].device
        k, v = inp["kv"][..., :C], inp["kv"][..., C:2 * C]
        rq = torch.empty(c.B, c.n_q, C, dtype=F64, device=dev)
        eq = torch.empty_like(rq)
        rk, ek, rv, ev = (torch.empty(c.B, c.n_kv, C, dtype=F64, device=dev) for _ in range(4))
        for b in range(c.B):
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                acc = ab.BwdAcc(c.n_kv, 64, dev)
                rq[b, :, sl], eq[b, :, sl] = ab.bwd_ref(inp["q"][b][:, sl], [(k[b][:, sl], v[b][:, sl], acc)], inp["out"][b][:, sl],
                                                        inp["dout"][b][:, sl], inp["lse"][b, h], dtype)
                rk[b, :, sl], ek[b, :, sl], rv[b, :, sl], ev[b, :, sl] = acc.finish(c.qsplit)
        return {"dq": Ref(rq, eq, dtype, ab.Where(c.n_q, H, 128), ab.check),
                "dk": Ref(rk, ek, dtype, ab.Where(c.n_kv, H, 64, what="key"), ab.check),
                "dv": Ref(rv, ev, dtype, ab.Where(c.n_kv, H, 64, what="key"), ab.check)}

    def declared(self, inp, name, index, value):
        c, C = self.c, self.C
        dq = torch.zeros(c.B, c.n_q, C, dtype=torch.bool)
        dk, dv = (torch.zeros(c.B, c.n_kv, C, dtype=torch.bool) for _ in range(2))
        what = self._what(name, index)
        if what == "lse":
            b, h, i = index
            col = h * 64
        else:
            b, i, col = index
            col %= C
        sl = slice(col // 64 * 64, col // 64 * 64 + 64)
        inf = abs(value) == math.inf
        if what == "lse" and value == math.inf:
            pass
        elif what == "q" and inf:
            up = _sign_up(inp["kv"][b, :, col], value)
            dk[b, :, sl], dv[b, :, sl] = up[:, None], up[:, None]
            dk[b, :, col] = True
            dq[b, i, sl] = bool(up.any())
        elif what == "k" and inf:
            up = _sign_up(inp["q"][b, :, col], value)
            dq[b, :, sl] = up[:, None]
            dq[b, :, col] = True
            dk[b, i, sl] = dv[b, i, sl] = bool(up.any())
        elif what in ("dout", "lse", "q"):
            dq[b, i, sl] = True
            dk[b, :, sl] = True
            if what == "dout":
                dv[b, :, col] = True
            else:
                dv[b, :, sl] = True
        else:
            dq[b, :, sl] = True
            dk[b, i, sl] = True
            if what == "k":
                dv[b, i, sl] = True
        return {"dq": dq, "dk": dk, "dv": dv}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        c, C = self.c, self.C
        assert ta.attn_bwd_qsplit(L, c, L.BF16 if dtype == BF16 else L.F16) == c.qsplit
        kv = inp["kv"]
        dkv = torch.full_like(kv, 3.0)
        dq = ob.attention_bwd(inp["q"], kv[..., :C], kv[..., C:2 * C], inp["out"], inp["dout"], inp["lse"], c.heads,
                              dkv[..., :C], dkv[..., C:2 * C], q_split=c.q_split)
        assert bool((dkv[..., 2 * C:] == 3.0).all()), "dK/dV stores outside their column slices"
        return {"dq": dq, "dk": dkv[..., :C], "dv": dkv[..., C:2 * C]}


class XattnBwd(AttnBwdBase):
    """dfw_cross_attention_bwd: P = softmax(scale q k^T) recomputed (no lse), delta_i = sum_j P_ij dP_ij."""

    def __init__(self, cid):
        self.c = next(c for c in ta.XB_CASES if c.id == cid)
        self.id, self.C = f"xattn_bwd_{cid}", self.c.heads * 64

    def make(self, dtype, device):
        q, k, v, do = ta.make_xa_inputs(self.c, dtype, device, seed=sum(map(ord, self.c.id)))
        return {"q": q, "k": k, "v": v, "dout": do}

    def plants(self):
        c, C = self.c, self.C
        last = (c.B - 1, c.n_q - 1, C - 1)
        return [("dout", last), ("v", (c.B - 1, c.L - 1, C - 1)), ("v", (0, 0, 0)), ("q", last), ("k", (c.B - 1, c.L - 1, C - 1))]

    def ref(self, inp, dtype):
        c, C = self.c, self.C
        dev = inp["q"].device
        rq = torch.empty(c.B, c.n_q, C, dtype=F64, device=dev)
        eq = torch.empty_like(rq)
        rk, ek, rv, ev = (torch.empty(c.B, c.L, C, dtype=F64, device=dev) for _ in range(4))
        for b in range(c.B):
            for h in range(c.heads):
                sl = slice(h * 64, (h + 1) * 64)
                rq[b, :, sl], eq[b, :, sl], rk[b, :, sl], ek[b, :, sl], rv[b, :, sl], ev[b, :, sl] = ab.xattn_bwd_ref(
                    inp["q"][b][:, sl], inp["k"][b][:, sl], inp["v"][b][:, sl], inp["dout"][b][:, sl])
        return {"dq": Ref(rq, eq, dtype, ab.Where(c.n_q, c.heads, 64), ab.check),
                "dk": Ref(rk, ek, dtype, ab.Where(c.L, c.heads, 16, what="key"), ab.check),
                "dv": Ref(rv, ev, dtype, ab.Where(c.L, c.heads, 16, what="key"), ab.check)}

    def declared(self, inp, name, index, value):
        """delta_i = sum_j P_ij dP_ij couples the keys of a row: a planted v_j makes delta of EVERY row non-finite, so all of
        dq and dk of that image and head (dv does not read v); a NaN k_j makes every row's softmax NaN: the whole head."""
        c, C = self.c, self.C
        dq = torch.zeros(c.B, c.n_q, C, dtype=torch.bool)
        dk, dv = (torch.zeros(c.B, c.L, C, dtype=torch.bool) for _ in range(2))
        b, i, col = index
        sl = slice(col // 64 * 64, col // 64 * 64 + 64)
        if name == "k" and abs(value) == math.inf:      # up rows: softmax NaN, the whole head through them; others: 0 x inf
            up = _sign_up(inp["q"][b, :, col], value)
            dq[b, :, sl] = up[:, None]
            dq[b, :, col] = True
            dk[b, :, sl] = dv[b, :, sl] = bool(up.any())
        elif name in ("dout", "q"):
            dq[b, i, sl] = True
            dk[b, :, sl] = True
            if name == "dout":
                dv[b, :, col] = True
            else:
                dv[b, :, sl] = True
        else:
            dq[b, :, sl] = True
            dk[b, :, sl] = True
            if name == "k":
                dv[b, :, sl] = True
        return {"dq": dq, "dk": dk, "dv": dv}

    def run(self, env, inp, dtype):
        ops, ob, L = env
        c, C = self.c, self.C
        dkv = torch.full((c.B, c.L, 2 * C + 64), 3.0, dtype=dtype, device=inp["q"].device)
        dq = ob.cross_attention_bwd(inp["q"], inp["k"], inp["v"], inp["dout"], c.heads, dkv[..., :C], dkv[..., C:2 * C])
        assert bool((dkv[..., 2 * C:] == 3.0).all()), "dK/dV stores outside their column slices"
        return {"dq": dq, "dk": dkv[..., :C], "dv": dkv[..., C:2 * C]}


ATTN_BWD = [FsaBwd("nshot0"), FsaBwd("shot2"), FsaBwd("shot7_forced3"),          # dQ split off, off (bank), on
            AttnBwd("nkv77_qsplit"), AttnBwd("nkv77_noqsplit"), XattnBwd("L77")]


class BiasOverflow(OverflowCase):
    """A boundary conv (fp32 operands) or the folded up2x with the fp32 bias[n0] scaled: column n0 of every pixel leaves
    the fp16 range in the epilogue's 16-bit store.  (Scaling source pixels of the up2x instead moves the other parities of
    the same position, whose folded weights share terms with the chosen one, through the band below the threshold.)"""
    family = "store_overflow"

    def __init__(self, base):
        self.base, self.id = base, f"overflow/{base.id}"

    def make(self, dtype, device):
        inp = self.base.make(dtype, device)
        bias = inp["bias"].clone()

        def row_of(f):
            bias[5] = f
            return self.base.ref(dict(inp, bias=bias), dtype)["y"].r[:, 5]

        bias[5] = _search_scale(row_of, 1e3, 1e6)
        inp["bias"] = bias
        return inp

    def ref(self, inp, dtype):
        return self.base.ref(inp, dtype)

    def run(self, env, inp, dtype):
        return self.base.run(env, inp, dtype)

    def post(self, env, inp, dtype, outs, planted):
        self.base.post(env, inp, dtype, outs, planted)


class AttnBwdOverflow(OverflowCase):
    """dq of the flash backward above the fp16 range, from finite operands of AttnBwd `nkv2_noqsplit` (two keys):
    dq_i = scale dS_i0 (k_0 - k_1) up to the rounding of the stored out / lse.  k_1 = k_0 except column D0, where it is 16
    lower; dout row I0 = f sign(v_0 - v_1), so dS_I0,0 = P_0 P_1 f sum |v_0 - v_1| and dq[I0, D0] = 2 dS; q row I0 is
    scaled by 0.01 (P = 1/2, and the row adds little to dk).  dS itself stays inside the fp16 range (the kernel rounds it
    to the storage type before its MFMAs); every other dq, dk, dv element stays far inside it."""
    family = "store_overflow"
    okey = "dq"
    I0, D0 = 500, 7

    def __init__(self):
        self.base = AttnBwd("nkv2_noqsplit")
        self.id = f"overflow/{self.base.id}"

    def make(self, dtype, device):
        b, C = self.base, self.base.C
        c = b.c
        inp = b.make(dtype, device)
        q, kv, dout = inp["q"].clone(), inp["kv"].clone(), inp["dout"].clone()
        kv[0, 1, :C] = kv[0, 0, :C]
        kv[0, 1, self.D0] = kv[0, 0, self.D0] - 16.0
        q[0, self.I0] = (q[0, self.I0].float() * 0.01).to(dtype)
        out, lse = b._fwd(q, lambda i: [(i, kv[i][:, :C], kv[i][:, C:2 * C])], c.B, c.heads, c.n_q, dtype)
        unit = torch.sign(kv[0, 0, C:2 * C].float() - kv[0, 1, C:2 * C].float())
        inp = {"q": q, "kv": kv, "out": out, "dout": dout, "lse": lse}

        def row_of(f):
            dout[0, self.I0] = (f * unit).to(dtype)
            refs = b.ref(inp, dtype)
            return torch.cat([refs[k].r.flatten() for k in ("dq", "dk", "dv")])

        row_of(_search_scale(row_of, 1e2, 6e4))
        return inp

    def ref(self, inp, dtype):
        return self.base.ref(inp, dtype)

    def run(self, env, inp, dtype):
        return self.base.run(env, inp, dtype)


BOUNDARY_OVERFLOW = [BiasOverflow(ConvSmall("w8_c128")), BiasOverflow(ConvSmall("w4_w12_t9")), BiasOverflow(ConvSmall("sc_w10_t9")),
                     BiasOverflow(Up2x((1, 16, 16, 64, 128))), AttnBwdOverflow()]


def threshold_operands(device):
    """The two neighbours of the fp16 overflow threshold through one GEMM: x [4, 64], w [64, 64] (fp16) whose column 0 is
    exactly 65504, 65520, -65504, -65520 -- eight products of exactly representable operands (64 is the smallest K the
    GEMM accepts; the other 56 products are 0 x 0.25), so the fp32 accumulation is exact in any order.  65504 is the
    largest finite fp16; 65520 is the tie between it and 2^16 and rounds to even: inf.  -> (x, w, column 0 in fp64)."""
    x = torch.zeros(4, 64)
    x[:, :8] = torch.tensor([512.0, 256.0, 128.0, 64.0, 32.0, 16.0, 8.0, 7.5])
    x[1, 7] = 7.75
    x[2:] = -x[:2]
    w = torch.full((64, 64), 0.25)
    w[0, :8], w[0, 8:] = 64.0, 0.0
    return x.to(F16).to(device), w.to(F16).to(device), [65504.0, 65520.0, -65504.0, -65520.0]


CASES = GEMM_FWD + BOUNDARY + GEMM_TN + COLSUM + GROUPNORM + LAYERNORM + POINTWISE + ATTN_FWD + ATTN_BWD + LOSS
OVERFLOW_CASES = GEMM_OVERFLOW + NORM_OVERFLOW + BOUNDARY_OVERFLOW


def params(cases):
    """[(case, dtype, plant, value name)] and their ids for pytest.mark.parametrize (store-overflow cases: no value)."""
    out, ids = [], []
    for c in cases:
        for dt in c.dtypes:
            for p in c.plants():
                if c.overflow:
                    out.append((c, dt, p))
                    ids.append(f"{c.id}-{TNAME[dt]}-scaled")
                    continue
                for v in c.values(*p):
                    out.append((c, dt, p, v))
                    ids.append(f"{c.id}-{TNAME[dt]}-{p[0]}{list(p[1])}{v}".replace(" ", ""))
    return out, ids
