"""The refusal table of diffews_amd/ops_split.py, under the discipline of tests/op_args_cases.py (whose Case, Row and
defects it reuses): per function that takes an address, the smallest valid call on host tensors and, per tensor argument,
one defect the wrapper has to refuse by name.  Used by tests/test_split_args_cpu.py.  Nothing here launches anything."""
import torch

from op_args_cases import I32, I64, U8, Case, Row, t  # noqa: F401

U16 = torch.uint16

SCALARS = {"reach", "passes", "connectivity", "min_area", "nlabels", "B", "H", "W"}


def _nearest():
    return dict(map=t(I32, 1, 3, 4), seeds=t(I32, 1, 3, 4), nearest=t(I32, 1, 3, 4), dist=t(U16, 1, 3, 4), ws=t(U8, 128), reach=2)


def _keyed():
    return dict(labels=t(U8, 1, 3, 4), keys=t(I32, 1, 3, 4), ids=t(I32, 1, 3, 4), n=t(I32, 1, 2), ws=t(U8, 256),
                filtered=t(U8, 1, 3, 4), stats=t(I32, 1, 5, 8), gt=t(U8, 1, 3, 4), counts=t(I64, 1, 2, 4), nlabels=3)


def _drop(*names):
    def edit(kw):
        for n in names:
            kw[n] = None
    return edit


def _stats2d(kw):
    kw["stats"] = t(I32, 5, 8)


CASES = [
    Case("ops_split.seg_nearest", _nearest,
         [("map", "dtype"), ("map", lambda kw: kw.update(map=t(I32, 3, 4))), ("map", "stride"),
          ("seeds", "dtype"), ("seeds", "shape"), ("seeds", "stride"),
          ("nearest", "dtype"), ("nearest", "shape"), ("nearest", "stride"),
          ("dist", lambda kw: kw.update(dist=t(U8, 1, 3, 4))), ("dist", "shape"), ("dist", "stride"),
          ("ws", "dtype"), ("ws", "stride")]),
    Case("ops_split.seg_components_keyed", _keyed,
         [("labels", "dtype"), ("labels", lambda kw: kw.update(labels=t(U8, 3, 4))), ("labels", "stride"),
          ("keys", "dtype"), ("keys", "shape"), ("keys", "stride"),
          ("ids", "dtype"), ("ids", "shape"), ("ids", "stride"),
          ("n", "dtype"), ("n", "shape"), ("n", "stride"),
          ("ws", "dtype"), ("ws", "stride"),
          ("filtered", "dtype"), ("filtered", "shape"), ("filtered", "stride"),
          ("stats", "dtype"), ("stats", "shape"), ("stats", "stride"), ("stats", _stats2d),
          ("gt", "dtype"), ("gt", "shape"), ("gt", "stride"),
          ("counts", "dtype"), ("counts", "shape"), ("counts", "stride"),
          Row("counts need a ground truth", _drop("gt")),
          Row("a ground truth needs nlabels", _drop("nlabels"))]),
]
