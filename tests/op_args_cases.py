"""The refusal table of ops.py and ops_bwd.py (diffews_amd.ops._Args): per function that takes an address, the smallest
valid call on host tensors and, per tensor argument, one defect the wrapper has to refuse by name.  Shared by
tests/test_op_args_cpu.py (every row, twice: as imported and with `assert` stripped) and tests/test_op_args_gpu.py (a dozen
rows on device tensors).  Nothing here launches anything."""
import re
import types

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U8, I32, I64 = torch.uint8, torch.int32, torch.int64


def t(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype)


def bf(*shape):
    return t(BF, *shape)


def f32(*shape):
    return t(F32, *shape)


# ---- defects: tensor -> a tensor the wrapper must refuse

def wrong_dtype(x):
    """A dtype no wrapper takes for any argument that also takes x's."""
    return x.to(F64 if x.dtype.is_floating_point else torch.int16)


def wrong_shape(x):
    """One column short: another shape, and too few elements for the extent."""
    return x[..., :-1].contiguous()


def wrong_stride(x):
    """x's shape and dtype over a last stride of 2 (the last dimension has to be longer than 1)."""
    assert x.shape[-1] > 1
    return torch.zeros(*x.shape[:-1], 2 * x.shape[-1], dtype=x.dtype, device=x.device)[..., ::2]


DEFECTS = {"dtype": wrong_dtype, "shape": wrong_shape, "stride": wrong_stride}


class Row:
    """One refusal: `name` as the message spells it, the defect (a key of DEFECTS applied to kwargs[name], or a function
    that edits the kwargs), the exception and the pattern (default: "<wrapper>: <name>")."""

    def __init__(self, name, defect, exc=ValueError, match=None):
        self.name, self.defect, self.exc, self.match = name, defect, exc, match

    @property
    def param(self):
        return self.name.split(".")[0].split("[")[0].split(" ")[0]

    def spoil(self, kw):
        if callable(self.defect):
            self.defect(kw)
        else:
            kw[self.name] = DEFECTS[self.defect](kw[self.name])


class Case:
    """`fn`: "ops.linear", "ops_bwd.ColsumQueue.add"; `valid()` -> kwargs of a valid call; `rows`; `wrapper`: the name
    the messages carry when it is not fn's (a wrapper behind a public name)."""

    def __init__(self, fn, valid, rows, wrapper=None, outputs=(), scalars=()):
        self.fn, self.valid, self.wrapper, self.outputs = fn, valid, wrapper or fn.split(".", 1)[1], outputs
        self.scalars = set(scalars)         # names that are scalars here and tensors elsewhere
        self.rows = [r if isinstance(r, Row) else Row(*r) for r in rows]

    def call(self, mods, kw):
        mod, _, name = self.fn.partition(".")
        obj = mods[mod]
        for part in name.split("."):
            obj = getattr(obj() if isinstance(obj, type) else obj, part)
        return obj(**kw)

    def pattern(self, row):
        return row.match or re.escape(f"{self.wrapper}: {row.name}") + r"(?!\w)"


def _targets(n):
    """What the native wrappers read of an input_pipeline.NativeTargets: one 2 x 2 query from a 4 x 4 source."""
    from diffews_amd import _lib as L
    items = (L.NativeItem * 1)()
    items[0].h = items[0].w = 2
    return types.SimpleNamespace(dev=t(U8, 64), b=1, src_hw=(4, 4), u8_bytes=16, tmp_bytes=16, pred_bytes=16, items=items,
                                 sizes=[(2, 2)], gt_base=(t(U8, 64), 64))


def _spoil_targets(field, how):
    def spoil(kw):
        tg = kw["targets"]
        if field == "dev":
            tg.dev = DEFECTS[how](tg.dev)
        else:
            tg.gt_base = (DEFECTS[how](tg.gt_base[0]), tg.gt_base[1])
    return spoil


def _plan():
    """A _lib.TilePlan record: an 8 x 8 image cut into 2 x 2 windows of 4 x 4."""
    from diffews_amd import _lib as L
    p = L.TilePlan()
    p.img_h = p.img_w = 8
    p.tile_h = p.tile_w = 4
    p.ny = p.nx = 2
    return p


def _cand_tab():
    """seg_labels_cand's table for one query that owns both of E_cap = 2 entries."""
    return torch.tensor([0, 2, 1, 2], dtype=I32)


def _kv(n):
    """k and v (or dk and dv) as column slices of one [1, 3, 256] buffer, v behind k."""
    kv = bf(1, 3, 256)
    return kv[..., :128], kv[..., 128:]


def _attn_bwd():
    (k, v), (dk, dv) = _kv(0), _kv(1)
    return dict(q=bf(1, 4, 128), k=k, v=v, out=bf(1, 4, 128), dout=bf(1, 4, 128), lse=f32(1, 2, 4), heads=2, dk_out=dk, dv_out=dv)


def _xattn_bwd():
    kw = _attn_bwd()
    del kw["out"], kw["lse"]
    return kw


def _entry(which, how):
    def spoil(kw):
        kind, w, y = kw["entries"][0]
        kw["entries"] = [(kind, DEFECTS[how](w), y) if which == "w" else (kind, w, DEFECTS[how](y))]
    return spoil


def _table(how):
    def spoil(kw):
        tab, n, blocks = kw["table"]
        kw["table"] = (DEFECTS[how](tab), n, blocks)
    return spoil


def _first_x(kw):
    kw["x"] = [wrong_dtype(kw["x"][0]), kw["x"][1]]


_SEG = dict(labels=lambda: t(U8, 1, 4, 4), ids=lambda: t(I32, 1, 4, 4), ws=lambda: t(U8, 16))
BIAS_T = ("dtype", TypeError, "must be a contiguous float32 tensor")         # _f32 keeps its TypeError


def _fsa(**more):
    q = bf(3, 128, 128)
    return dict(q=q, k=bf(3, 128, 128), v=bf(3, 128, 128), heads=2, k_bank=bf(3, 128, 128), v_bank=bf(3, 128, 128),
                out=bf(3, 128, 128), **more)


_FSA_ROWS = [("q", "stride"), ("k", "dtype"), ("v", "shape"), ("k_bank", "shape"), ("v_bank", "dtype"), ("out", "shape")]

CASES = [
    Case("ops.linear", lambda: dict(x=bf(4, 8), w=bf(16, 8), bias=f32(16), residual=bf(4, 16), rowbias=f32(1, 16), rows_per_img=4,
                                    out=bf(4, 16)),
         [("x", "stride"), ("w", "shape"), ("bias", "shape"), ("bias", *BIAS_T), ("residual", "dtype"), ("rowbias", "shape"),
          ("rowbias", "dtype", TypeError, "rowbias must be float32"), ("out", "shape"), ("out", "dtype"), ("out", "stride")],
         outputs=("out",)),
    Case("ops.bmm_nt", lambda: dict(x=bf(2, 4, 8), w=bf(2, 16, 8)), [("x", "stride"), ("w", "dtype"), ("w", "shape")]),
    Case("ops.conv3x3", lambda: dict(x=bf(1, 4, 4, 32), w=bf(64, 288), cout=64, bias=f32(64), rowbias=f32(1, 64),
                                     residual=bf(1, 4, 4, 64), w_blk=bf(64 * 288)),
         [("x", "stride"), ("w", "shape"), ("bias", "shape"), ("rowbias", "shape"), ("residual", "shape"), ("w_blk", "dtype")]),
    Case("ops.fsa_attention", lambda: _fsa(nshot=1, lse=f32(3, 2, 128)), _FSA_ROWS + [("lse", "dtype")], outputs=("out", "lse")),
    Case("ops.fsa_attention_routed", lambda: _fsa(table=t(I32, 3, 2), table_host=t(I32, 3, 2), max_shots=1, min_shots=1),
         _FSA_ROWS + [("table", "shape"), ("table_host", "dtype")]),
    Case("ops.split_storage", lambda: dict(x=f32(8), dtype=BF), [("x", "dtype")]),
    Case("ops.conv3x3_up2x", lambda: dict(x=bf(1, 16, 16, 64), w_folded=bf(64, 1024), cout=64, bias=f32(64)),
         [("x", "stride"), ("w_folded", "shape"), ("bias", "shape")]),
    Case("ops.vae_attention", lambda: dict(q=bf(1, 4, 512), k=bf(1, 4, 512), v=bf(1, 4, 512), out=bf(1, 4, 512)),
         [("q", "stride"), ("k", "shape"), ("v", "dtype"), ("out", "shape")], outputs=("out",)),
    Case("ops.cross_attention", lambda: dict(q=bf(1, 4, 128), k=bf(1, 3, 128), v=bf(1, 3, 128), heads=2),
         [("q", "stride"), ("k", "shape"), ("v", "dtype")]),
    Case("ops.groupnorm", lambda: dict(x=bf(1, 2, 2, 32), gamma=f32(32), beta=f32(32), groups=32, eps=1e-5),
         [("x", "stride"), ("gamma", "shape"), ("beta", *BIAS_T)]),
    Case("ops.layernorm", lambda: dict(x=bf(4, 32), gamma=f32(32), beta=f32(32)), [("x", "stride"), ("gamma", *BIAS_T), ("beta", "shape")]),
    Case("ops.conv_small", lambda: dict(x=[f32(1, 4, 4, 4), f32(1, 4, 4, 4)], w=f32(8, 9, 4), bias=f32(8), cout=8, taps=9, dtype=BF,
                                        gn_groups=4, out=bf(2, 4, 4, 8), gn_part=f32(2, 1, 4, 2)),
         [Row("x[0]", _first_x), ("w", "shape"), ("bias", "shape"), ("out", "dtype"), ("out", "shape"), ("gn_part", "dtype")],
         outputs=("out", "gn_part")),
    Case("ops.conv_small", lambda: dict(x=f32(1, 4, 4, 4), w=f32(8, 9, 4), bias=f32(8), cout=8, taps=9, dtype=BF, nchw_f32_out=True,
                                        out=f32(1, 8, 4, 4)), [("out", "stride"), ("out", "dtype")]),
    Case("ops.meter_update", lambda: dict(counts=t(I64, 2, 4), class_id=t(I64, 2), inter_buf=t(I64, 2, 5), union_buf=t(I64, 2, 5)),
         [("counts", "shape"), ("class_id", "dtype"), ("inter_buf", "stride"), ("union_buf", "shape")]),
    Case("ops.softmax_rows", lambda: dict(x=f32(2, 8), dtype=BF), [("x", "dtype")]),
    Case("ops.softmax_groups", lambda: dict(x=f32(2, 8), groups=1, L_=8, dtype=BF), [("x", "stride")]),
    Case("ops.transpose", lambda: dict(x=bf(1, 2, 4)), [("x", "stride")]),
    Case("ops.concat_channels", lambda: dict(a=bf(2, 4), b=bf(2, 4)), [("a", "stride"), ("b", "dtype")]),
    Case("ops.to_storage", lambda: dict(x=f32(8), dtype=BF), [("x", "stride")]),
    Case("ops.timestep_embedding", lambda: dict(timesteps=f32(2), dim=8, dtype=BF), [("timesteps", "dtype")]),
    Case("ops.seg_postprocess", lambda: dict(x=f32(1, 3, 4, 4), gt=t(U8, 1, 4, 4), u8_out=t(U8, 1, 3, 4, 4), counts_out=t(I64, 1, 4),
                                             scratch=t(I32, 2)),
         [("x", "dtype"), ("gt", "shape"), ("u8_out", "shape"), ("counts_out", "dtype"), ("scratch", "dtype")]),
    Case("ops.seg_labels", lambda: dict(seg_u8=t(U8, 2, 1, 3, 4, 4), mx=t(I32, 2, 1), gt=t(U8, 1, 4, 4), labels_out=t(U8, 1, 4, 4),
                                        counts_out=t(I64, 1, 2, 3)),
         [("seg_u8", "dtype"), ("mx", "shape"), ("gt", "stride"), ("labels_out", "shape"), ("counts_out", "shape")]),
    Case("ops.seg_labels_cand", lambda: dict(seg_u8=t(U8, 2, 3, 4, 4), mx=t(I32, 2), tab=_cand_tab(), tab_host=_cand_tab(), nlabels=2,
                                             gt=t(U8, 1, 4, 4), labels_out=t(U8, 1, 4, 4), counts_out=t(I64, 1, 2, 3)),
         [("seg_u8", "stride"), ("mx", "dtype"), ("tab", "dtype"), ("tab_host", "shape"), ("gt", "shape"), ("labels_out", "dtype"),
          ("counts_out", "shape")]),
    Case("ops.seg_native", lambda: dict(seg_u8=t(U8, 1, 3, 4, 4), targets=_targets(1), u8_out=t(U8, 16), pred_out=t(U8, 16), tmp=t(U8, 16)),
         [("seg_u8", "dtype"), Row("targets.dev", _spoil_targets("dev", "dtype")), Row("targets.gt_base", _spoil_targets("gt", "shape")),
          ("u8_out", "shape"), ("pred_out", "dtype"), ("tmp", "shape")]),
    Case("ops.seg_labels_native", lambda: dict(seg_u8=t(U8, 2, 1, 3, 4, 4), targets=_targets(2), want_u8=True, labels_out=t(U8, 16),
                                               u8_out=t(U8, 32), tmp=t(U8, 32)),
         [("seg_u8", "stride"), Row("targets.dev", _spoil_targets("dev", "stride")), ("labels_out", "shape"), ("u8_out", "dtype"),
          ("tmp", "shape")]),
    Case("ops.seg_labels_cand_native", lambda: dict(seg_u8=t(U8, 2, 3, 4, 4), targets=_targets(2), tab=_cand_tab(), tab_host=_cand_tab(),
                                                    nlabels=2, want_u8=True, labels_out=t(U8, 16), u8_out=t(U8, 32), tmp=t(U8, 32)),
         [("seg_u8", "dtype"), Row("targets.dev", _spoil_targets("dev", "dtype")), ("tab", "stride"), ("tab_host", "dtype"),
          ("labels_out", "dtype"), ("u8_out", "shape"), ("tmp", "stride")]),
    Case("ops.tiles_cut", lambda: dict(plan=_plan(), img_u8=t(U8, 8, 8, 3), lut=f32(256), out=f32(4, 3, 4, 4)),
         [("img_u8", "shape"), ("lut", "dtype"), ("out", "shape"), ("out", "dtype")], outputs=("out",)),
    Case("ops.tiles_merge", lambda: dict(plan=_plan(), win=t(U8, 1, 4, 3, 4, 4), out=t(U8, 1, 3, 8, 8), mx=t(I32, 2)[:1]),
         [("win", "shape"), ("out", "dtype"), ("mx", "dtype")]),
    Case("ops.tiles_labels_cand", lambda: dict(plan=_plan(), ent=t(U8, 2, 3, 4, 4), tab=t(I32, 7), tab_host=t(I32, 7), N=1, gt=t(U8, 8, 8),
                                               labels_out=t(U8, 8, 8), counts_out=t(I64, 2, 2), mx_out=t(I32, 2)[:1], area_out=t(I64, 1, 2)),
         [("ent", "shape"), ("tab", "dtype"), ("tab_host", "shape"), ("gt", "dtype"), ("labels_out", "shape"), ("counts_out", "shape"),
          ("mx_out", "dtype"), ("area_out", "shape")]),
    Case("ops.seg_components", lambda: dict(labels=_SEG["labels"](), ids=_SEG["ids"](), n=t(I32, 1, 2), ws=_SEG["ws"](),
                                            filtered=t(U8, 1, 4, 4), stats=t(I32, 1, 2, 8), gt=t(U8, 1, 4, 4), counts=t(I64, 1, 2, 3), nlabels=2),
         [("labels", "dtype"), ("ids", "shape"), ("n", "shape"), ("ws", "dtype"), ("filtered", "stride"), ("stats", "shape"), ("gt", "shape"),
          ("counts", "dtype")], outputs=("ids",)),
    Case("ops.seg_holes", lambda: dict(labels=_SEG["labels"](), ids=_SEG["ids"](), ids_out=_SEG["ids"](), labels_out=_SEG["labels"](),
                                       holes=t(I32, 1, 2), ws=_SEG["ws"](), stats=t(I32, 1, 2, 8), stats_out=t(I32, 1, 2, 8), gt=t(U8, 1, 4, 4),
                                       counts=t(I64, 1, 2, 3), nlabels=2),
         [("labels", "stride"), ("ids", "dtype"), ("ids_out", "shape"), ("labels_out", "dtype"), ("holes", "shape"), ("ws", "dtype"),
          ("stats", "dtype"), ("stats_out", "shape"), ("gt", "dtype"), ("counts", "shape")]),
    Case("ops.seg_rle", lambda: dict(ids=_SEG["ids"](), runs=t(I32, 1, 4, 2), run_off=t(I32, 1, 3), nruns=t(I32, 1, 2), ws=_SEG["ws"](), cap=2),
         [("ids", "dtype"), ("runs", "shape"), ("run_off", "shape"), ("nruns", "dtype"), ("ws", "stride")]),
    Case("ops.seg_contours", lambda: dict(ids=_SEG["ids"](), verts=t(I32, 1, 8, 2), rings=t(I32, 1, 2, 4), ring_off=t(I32, 1, 3), n=t(I32, 1, 4),
                                          ws=_SEG["ws"](), cap=2, simp_verts=t(I32, 1, 8, 2), simp_rings=t(I32, 1, 2, 4), simp_n=t(I32, 1, 4)),
         [("ids", "stride"), ("verts", "dtype"), ("rings", "shape"), ("ring_off", "shape"), ("n", "dtype"), ("ws", "dtype"),
          ("simp_verts", "shape"), ("simp_rings", "dtype"), ("simp_n", "shape")]),
    Case("ops.seg_match", lambda: dict(pids=_SEG["ids"](), gids=_SEG["ids"](), pairs=t(I32, 1, 4, 3), pair_off=t(I32, 1, 4), area=t(I32, 1, 6),
                                       match=t(I32, 1, 2, 3), gmatch=t(I32, 1, 2), pq=t(I64, 1, 3, 4), n=t(I32, 1, 4), ws=_SEG["ws"](),
                                       max_records=4, pstats=t(I32, 1, 2, 8), gstats=t(I32, 1, 2, 8), skip=t(U8, 1, 4, 4)),
         [("pids", "dtype"), ("gids", "shape"), ("pairs", "shape"), ("pair_off", "shape"), ("area", "dtype"), ("match", "dtype"),
          ("gmatch", "stride"), ("pq", "dtype"), ("n", "shape"), ("ws", "dtype"), ("pstats", "shape"), ("gstats", "dtype"), ("skip", "dtype")]),
    Case("ops.seg_scores", lambda: dict(ids=_SEG["ids"](), labels=_SEG["labels"](), seg_u8=t(U8, 1, 3, 4, 4), planes=t(I32, 1, 3),
                                        planes_host=t(I32, 1, 3), scores=t(I64, 1, 2, 4), ws=_SEG["ws"]()),
         [("ids", "dtype"), ("labels", "shape"), ("seg_u8", "dtype"), ("planes", "dtype"), ("planes_host", "stride"), ("scores", "dtype"),
          ("ws", "dtype")]),
    Case("ops.seg_boundary", lambda: dict(map=_SEG["labels"](), dist=t(U8, 1, 4, 4), ws=_SEG["ws"](), dmax=2, band=t(U8, 1, 4, 4), d=1),
         [("map", "dtype"), ("dist", "shape"), ("ws", "dtype"), ("band", "dtype")], outputs=("dist",)),
    Case("ops.seg_boundary", lambda: dict(map=_SEG["ids"](), dist=t(torch.uint16, 1, 4, 4), ws=_SEG["ws"](), dmax=2, metric="euclidean",
                                          peaks=t(I64, 1, 2)), [("dist", "dtype"), ("peaks", "dtype"), ("peaks", "stride")]),
    Case("ops.seg_boundary_counts", lambda: dict(pred=_SEG["labels"](), pdist=t(U8, 1, 4, 4), gt=t(U8, 1, 4, 4), gdist=t(U8, 1, 4, 4),
                                                 counts=t(I64, 1, 2, 3), d=1),
         [("pred", "dtype"), ("pdist", "shape"), ("gt", "dtype"), ("gdist", "dtype"), ("counts", "dtype")]),
    # ---- ops_bwd
    Case("ops_bwd.gemm_tn", lambda: dict(dy=bf(4, 16), x=bf(4, 8), out=f32(1, 16, 1, 8)),
         [("dy", "stride"), ("x", "dtype"), ("out", "shape"), ("out", "dtype")], outputs=("out",), scalars=("n",)),
    Case("ops_bwd.colsum", lambda: dict(x=bf(4, 8), out=f32(1, 8)), [("x", "stride"), ("out", "shape"), ("out", "dtype")]),
    Case("ops_bwd.ColsumQueue.add", lambda: dict(x=bf(8, 8), out=f32(1, 8)), [("x", "stride"), ("out", "shape"), ("out", "dtype")]),
    Case("ops_bwd.groupnorm_bwd", lambda: dict(x=bf(1, 2, 2, 32), dy=bf(1, 2, 2, 32), mean_rstd=f32(1, 32, 2), gamma=f32(32), beta=f32(32),
                                               groups=32, silu=False, dgamma=f32(32), dbeta=f32(32), dx_add=bf(1, 2, 2, 32)),
         [("x", "stride"), ("dy", "shape"), ("mean_rstd", "shape"), ("gamma", "shape"), ("beta", *BIAS_T), ("dgamma", "shape"),
          ("dbeta", *BIAS_T), ("dx_add", "dtype")], outputs=("dgamma",)),
    Case("ops_bwd.layernorm_bwd", lambda: dict(x=bf(4, 32), dy=bf(4, 32), gamma=f32(32), dgamma=f32(32), dbeta=f32(32), dx_add=bf(4, 32)),
         [("x", "stride"), ("dy", "dtype"), ("gamma", "shape"), ("dgamma", *BIAS_T), ("dbeta", "shape"), ("dx_add", "shape")]),
    Case("ops_bwd.geglu_fwd", lambda: dict(pre=bf(2, 8)), [("pre", "stride")]),
    Case("ops_bwd.geglu_bwd", lambda: dict(pre=bf(2, 8), dout=bf(2, 4)), [("pre", "stride"), ("dout", "shape")]),
    Case("ops_bwd.add", lambda: dict(a=bf(2, 8), b=bf(2, 8)), [("a", "stride"), ("b", "dtype")]),
    Case("ops_bwd.slice_channels", lambda: dict(a=bf(2, 8), c0=0, Cc=4), [("a", "stride")]),
    Case("ops_bwd.zero_stuff2x", lambda: dict(a=bf(1, 2, 2, 8)), [("a", "stride")]),
    Case("ops_bwd.pool2x2_sum", lambda: dict(a=bf(1, 2, 2, 8)), [("a", "stride")]),
    Case("ops_bwd.nchw_to_nhwc", lambda: dict(x=f32(1, 4, 2, 2), dtype=BF), [("x", "dtype")]),
    Case("ops_bwd.mse_loss", lambda: dict(pred=f32(1, 4, 2, 2), target=f32(1, 4, 2, 2), dtype=BF, dpred_out=bf(1, 2, 2, 8),
                                          dpred_nchw_out=f32(1, 4, 2, 2)),
         [("pred", "dtype"), ("target", "shape"), ("dpred_out", "shape"), ("dpred_nchw_out", "dtype")]),
    Case("ops_bwd.fsa_attention_bwd", lambda: dict(qkv=bf(1, 4, 384), out=bf(1, 4, 128), dout=bf(1, 4, 128), lse=f32(1, 2, 4), heads=2),
         [("qkv", "stride"), ("out", "shape"), ("dout", "dtype"), ("lse", "dtype")]),
    Case("ops_bwd.attention_bwd", _attn_bwd,
         [("q", "stride"), ("k", "dtype"), ("v", "shape"), ("out", "shape"), ("dout", "stride"), ("lse", "shape"), ("dk_out", "dtype"),
          ("dv_out", "shape")], outputs=("dk_out",)),
    Case("ops_bwd.cross_attention_bwd", _xattn_bwd,
         [("q", "stride"), ("k", "dtype"), ("v", "shape"), ("dout", "shape"), ("dk_out", "shape"), ("dv_out", "dtype")]),
    Case("ops_bwd.silu", lambda: dict(a=bf(8), dy=bf(8)), [("a", "stride"), ("dy", "shape")]),
    Case("ops_bwd.sumsq", lambda: dict(x=f32(8)), [("x", "dtype")]),
    Case("ops_bwd.linear_wt", lambda: dict(w=bf(8, 8)), [("w", "stride")]),
    Case("ops_bwd.conv3x3_wd", lambda: dict(w=bf(8, 72), cout=8), [("w", "stride")]),
    Case("ops_bwd.relayout_table", lambda: dict(entries=[("T", bf(8, 8), bf(8, 8))], device="cpu"),
         [Row("entries[0] w", _entry("w", "stride")), Row("entries[0] y", _entry("y", "dtype"))]),
    Case("ops_bwd.weight_relayout_batch", lambda: dict(table=(t(I64, 1, 12), 1, 1)), [Row("table", _table("dtype")), Row("table", _table("shape"))]),
    Case("ops_bwd.loss_grad", lambda: dict(g=f32(1, 4, 2, 2), dtype=BF, dpred_out=bf(1, 2, 2, 8), dpred_nchw_out=f32(1, 4, 2, 2)),
         [("g", "stride"), ("dpred_out", "dtype"), ("dpred_nchw_out", "shape")]),
    Case("ops_bwd.to_f32", lambda: dict(x=bf(8), out=f32(8)), [("x", "stride"), ("out", "dtype"), ("out", "shape")], outputs=("out",)),
    Case("ops_bwd.adamw", lambda: dict(param=f32(8), grad=f32(8), exp_avg=f32(8), exp_avg_sq=f32(8), step=1, lr=1e-3, grad_sumsq=f32(1),
                                       shadow=bf(8), found_inf=t(I32, 1)),
         [("param", "dtype"), ("grad", "shape"), ("exp_avg", "stride"), ("exp_avg_sq", "dtype"), ("grad_sumsq", *BIAS_T), ("shadow", "shape"),
          ("found_inf", "dtype")], outputs=("param",)),
]

# Parameters that are not tensors whose address is passed: scalars, flags, dtypes, plans, and id lists the wrapper copies.
SCALARS = set("""self rows_per_img act geglu out_f32 out_scale splitk colscale cout stride pad ups out_nchw_f32 gn_groups gn_in heads nshot
    scale n_plain q_prescaled key_split bank_shared _group _shots max_shots min_shots dtype groups eps silu return_stats out_dtype taps
    nchw_f32_out in_scale L_ dim flip_sin_to_cos freq_shift r_threshold threshold batch_max nlabels want_area want_u8 want_pred
    class_ids entry_ids plan first count N connectivity min_area max_area cap order tol4 max_records iou dmax d metric kc geom
    accumulate batch batch2 strides M lda ldb out_strides segs grad_scale c0 Cc cp loss_scale q_split step lr betas weight_decay
    max_grad_norm device""".split())

# Functions the walk finds that have no rows of their own, each with its reason.
EXEMPT = {
    "ops._p": "the null-safe address of a tensor its caller has checked",
    "ops._Args.__call__": "the checker itself",
    "ops._gemm_launch": "no tensor parameter: the address is the workspace it allocates",
    "ops._fsa_launch": "q only names the device of the workspace it allocates; checked by fsa_attention and fsa_attention_routed",
    "ops._fsa_args": "runs under its caller's checker: rows q, k, v, out of fsa_attention and fsa_attention_routed",
    "ops._fsa_bank": "runs under its caller's checker: rows k_bank, v_bank of fsa_attention and fsa_attention_routed",
    "ops._native_setup": "runs under its caller's checker: rows targets.dev, targets.gt_base, u8_out, tmp of the three native wrappers",
    "ops.zeros": "no tensor parameter: fills the buffer it allocates",
    "ops_bwd._ew": "runs under its caller's checker: rows a, b of add, slice_channels, zero_stuff2x, pool2x2_sum",
    "ops_bwd.ColsumQueue.flush": "no tensor parameter: the addresses are those add() checked and a table it allocates",
}
