"""CPU tests (no GPU) of candidate classes per query at native size: the C entry point through the header, the ctypes
table and the compiler, dfw_seg_labels_cand_native's host-side validation (every code comes back before any launch, on
host memory), the CPU reference (tests/cand_native_ref.py, which tests/test_candidates_native_gpu.py holds the kernels
to) tied to nway_native_ref on full lists and pinned on the input the GPU tests rely on, and the host logic above the op:
workspace sizing with K, candidate_tables' new entries, the argument errors of segment_candidates_native / segment_stream."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cand_native_ref as cn
import nway_native_ref as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE, ERANGE, EWORKSPACE = -1, -2, -3, -4


# ---------------------------------------------------------------------------------------------- ABI
def test_header_ctypes_symbol_and_version(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int dfw_seg_labels_cand_native(const dfw_seg_labels_cand_native_args* a, dfw_stream_t stream);" in flat
    cname, cls = "dfw_seg_labels_cand_native_args", L.SegLabelsCandNativeArgs
    body = re.search(r"typedef struct \{([^{}]*)\}\s*" + cname + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.strip().replace("*", " ").replace(",", " ").split()
        names += [p for p in parts if p not in ("const", "void", "float", "int32_t", "int64_t", "size_t", "uint8_t", "uint32_t")]
    assert names == [f[0] for f in cls._fields_]
    for need in ("tab", "tab_host", "E_cap", "nlabels", "items", "items_host", "weights", "gt", "tmp_cls_stride",
                 "u8_cls_stride", "labels", "mx", "counts", "area", "out_u8", "class_ids", "entry_ids"):
        assert need in names, need
    assert "batch_max" not in names
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "diffews_hip.h"\nint main(){printf("%zu", sizeof(' + cname + '));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(cls)
    assert L.SYMBOLS["dfw_seg_labels_cand_native"] == (C.c_int32, [C.POINTER(cls), C.c_void_p])
    assert hip_lib.dfw_seg_labels_cand_native is not None
    assert hip_lib.dfw_version() >= 112


def test_public_signatures():
    from diffews_amd import evaluate, ops
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise as P
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(ops.seg_labels_cand_native)[:11] == ["seg_u8", "targets", "tab", "tab_host", "nlabels", "r_threshold",
                                                      "threshold", "class_ids", "entry_ids", "want_area", "want_u8"]
    sig = inspect.signature(ops.seg_labels_cand_native).parameters
    assert sig["class_ids"].default is None and sig["entry_ids"].default is None
    assert sig["want_area"].default is False and sig["want_u8"].default is False
    assert names(P.segment_candidates_native) == ["self", "bankset", "query_img", "candidates", "native", "class_ids",
                                                  "query_labels", "r_threshold", "threshold", "entry_batch", "labels",
                                                  "captured"]
    sig = inspect.signature(P.segment_candidates_native).parameters
    assert sig["class_ids"].default is None and sig["native"].default is inspect.Parameter.empty and "batch_max" not in sig
    assert "native" not in inspect.signature(P.segment_candidates).parameters      # the plain call is what it was
    sig = inspect.signature(P.segment_stream).parameters
    assert sig["native"].default is False
    sig = inspect.signature(evaluate.evaluate_candidates).parameters
    assert sig["use_original_imgsize"].default is False and sig["class_ids"].default is None


# ---------------------------------------------------------------------------------------------- host validation
GOOD_TAB = [0, 2, 2, 5] + [3, 1, 2, 1, 3] + [0, 0, 0]              # B = 3, E = 5, E_cap = 8, nlabels = 3, K = 3


def _valid_args(L, tab=GOOD_TAB, E_cap=8, nlabels=3, sizes=((37, 83), (64, 64), (20, 28)), src=(64, 64), with_gt=True,
                with_u8=True, K=None):
    """A fully valid dfw_seg_labels_cand_native call on host memory (never launched: every test below breaks one thing)."""
    from diffews_amd.input_pipeline import NativeTargets
    gts = [np.zeros(s, np.uint8) for s in sizes] if with_gt else None
    t = NativeTargets(src, sizes, gt=gts, device=None)
    B = len(sizes)
    if K is None:
        K = max(max(b - a for a, b in zip(tab[:B], tab[1:B + 1])), 1)
    tmp_n = K * t.tmp_bytes + (0 if with_u8 else K * t.u8_bytes)
    keep = dict(t=t, seg=np.zeros((E_cap, 3) + tuple(src), np.uint8), tmp=np.zeros(tmp_n, np.uint8),
                u8=np.zeros(K * t.u8_bytes, np.uint8), labels=np.zeros(t.pred_bytes, np.uint8),
                mx=np.zeros(E_cap, np.uint32), counts=np.zeros((B, 2, nlabels + 1), np.int64),
                area=np.zeros((E_cap, 2), np.int64), ids=np.arange(max(nlabels, E_cap), dtype=np.int32),
                tab=np.asarray(tab, np.int32))
    a = L.SegLabelsCandNativeArgs()
    a.seg_u8, a.B, a.E_cap, a.nlabels, a.Hs, a.Ws = keep["seg"].ctypes.data, B, E_cap, nlabels, src[0], src[1]
    a.tab = a.tab_host = keep["tab"].ctypes.data
    a.items = a.items_host = C.addressof(t.items)
    a.weights, a.weights_bytes = t.host.ctypes.data, t.host.nbytes
    a.gt, a.gt_bytes = (t.host.ctypes.data, t.host.nbytes) if with_gt else (None, 0)
    a.tmp, a.tmp_bytes, a.tmp_res_off = keep["tmp"].ctypes.data, tmp_n, K * t.tmp_bytes
    a.tmp_cls_stride, a.u8_cls_stride = t.tmp_bytes, t.u8_bytes
    if with_u8:
        a.out_u8, a.out_u8_bytes = keep["u8"].ctypes.data, K * t.u8_bytes
    a.labels, a.labels_bytes = keep["labels"].ctypes.data, t.pred_bytes
    a.mx, a.counts, a.area = keep["mx"].ctypes.data, keep["counts"].ctypes.data if with_gt else None, keep["area"].ctypes.data
    a.class_ids = keep["ids"].ctypes.data
    a.r_threshold, a.threshold = 0.25, 0.0
    return a, keep


def test_validates_on_the_host_before_any_launch(hip_lib):
    """Every return code of the header's contract, on host memory with no GPU: a call that got past the validation would
    launch and fail differently (or crash), so each assertion also shows that nothing was launched.  The union of
    dfw_seg_labels_native's and dfw_seg_labels_cand's checks, plus E > 65535 and the K-strided workspace."""
    from diffews_amd import _lib as L
    lib = hip_lib
    call = lambda a: lib.dfw_seg_labels_cand_native(C.byref(a), None)
    assert lib.dfw_seg_labels_cand_native(None, None) == EINVAL
    # ---- dfw_seg_labels_native's and dfw_seg_labels_cand's null pointers and sizes
    for field in ("seg_u8", "tab", "tab_host", "items", "items_host", "weights", "tmp", "labels"):
        a, keep = _valid_args(L)
        setattr(a, field, None)
        assert call(a) == EINVAL, field
    for field in ("B", "E_cap", "Hs", "Ws"):
        for bad in (0, -2):
            a, keep = _valid_args(L)
            setattr(a, field, bad)
            assert call(a) == EINVAL, (field, bad)
    for bad in (0, -1, 255):
        a, keep = _valid_args(L)
        a.nlabels = bad
        assert call(a) == EINVAL, bad
    a, keep = _valid_args(L)
    a.gt = None                                         # counts without a ground truth
    assert call(a) == EINVAL
    a, keep = _valid_args(L)
    a.mx = None                                         # dynamic threshold without the maxima
    assert call(a) == EINVAL
    a, keep = _valid_args(L)
    a.r_threshold = 0.0                                 # neither thresholding flag
    assert call(a) == EINVAL
    a, keep = _valid_args(L)
    a.r_threshold, a.threshold = -1.0, -0.5
    assert call(a) == EINVAL
    a, keep = _valid_args(L)
    a.entry_ids = keep["ids"].ctypes.data               # both id tables
    assert call(a) == EINVAL
    a, keep = _valid_args(L)
    a.class_ids, a.entry_ids = None, keep["ids"].ctypes.data
    a.tmp_bytes -= 16                                   # (valid with entry_ids alone: the next failure is the workspace's)
    assert call(a) == EWORKSPACE
    # ---- the table, as dfw_seg_labels_cand validates it
    many = [0, 255, 255, 255] + [1] * 255 + [0]
    for what, tab, kw in [
            ("offsets start above 0", [1, 2, 2, 5] + GOOD_TAB[4:], {}),
            ("offsets start below 0", [-1, 2, 2, 5] + GOOD_TAB[4:], {}),
            ("offsets decrease", [0, 3, 2, 5] + GOOD_TAB[4:], {}),
            ("offsets end above E_cap", [0, 2, 2, 9] + GOOD_TAB[4:], {}),
            ("offsets pass E_cap in the middle", [0, 9, 9, 9] + GOOD_TAB[4:], {}),
            ("255 entries in a query", many, dict(E_cap=256, K=1)),
            ("label 0 below E", GOOD_TAB[:4] + [3, 0, 2, 1, 3, 0, 0, 0], {}),
            ("label above nlabels", GOOD_TAB[:4] + [3, 1, 4, 1, 3, 0, 0, 0], {}),
            ("label < 0", GOOD_TAB[:4] + [3, 1, 2, 1, -3, 0, 0, 0], {}),
            ("last real label bad", GOOD_TAB[:4] + [3, 1, 2, 1, 9, 0, 0, 0], {})]:
        a, keep = _valid_args(L, tab=tab, **({"K": 3} | kw))
        assert call(a) == EINVAL, what
    # ---- the items, as dfw_seg_labels_native validates them
    for field in ("h", "w"):
        for bad in (0, -3):
            a, keep = _valid_args(L)
            setattr(keep["t"].items[1], field, bad)
            assert call(a) == EINVAL, field
    a, keep = _valid_args(L)
    keep["t"].items[0].gt_elem = 2
    assert call(a) == EINVAL
    for field in ("xk", "yk"):
        a, keep = _valid_args(L)
        setattr(keep["t"].items[0], field, getattr(keep["t"].items[0], field) + 2)
        assert call(a) == ESHAPE, field
    a, keep = _valid_args(L)
    a.Ws = 128                                          # the table's x weights were made for Ws = 64: other ksize
    assert call(a) == ESHAPE
    a, keep = _valid_args(L)
    keep["t"].items[0].yc_off += 2                      # misaligned int32 weights
    assert call(a) == ESHAPE
    for field in ("h", "w"):
        a, keep = _valid_args(L)
        setattr(keep["t"].items[1], field, 65536)
        assert call(a) == ERANGE, field
    for field in ("Hs", "Ws", "B"):
        a, keep = _valid_args(L)
        setattr(a, field, 65536)
        assert call(a) == ERANGE, field
    a, keep = _valid_args(L)
    a.E_cap = (1 << 24) + 1
    assert call(a) == ERANGE
    # E = 65536 entries over 259 queries of at most 254: every offset and label valid, only grid z is out of range
    B, E = 259, 65536
    off = [min(q * 254, E) for q in range(B + 1)]
    assert off[-1] == E and max(b - a for a, b in zip(off, off[1:])) == 254
    a, keep = _valid_args(L, tab=off + [1] * E, E_cap=E, sizes=((8, 8),) * B, src=(8, 8), K=1)
    assert call(a) == ERANGE
    # ---- the workspace: K strides, K = 3 the longest list of GOOD_TAB
    for with_u8, fields in ((True, ("tmp_bytes", "out_u8_bytes", "labels_bytes", "gt_bytes")),
                            (False, ("tmp_bytes", "tmp_res_off", "labels_bytes"))):
        for field in fields:
            a, keep = _valid_args(L, with_u8=with_u8)
            setattr(a, field, getattr(a, field) - 16)   # position K - 1's last image no longer fits
            assert call(a) == EWORKSPACE, (with_u8, field)
    a, keep = _valid_args(L, with_u8=False)
    a.tmp_res_off = a.tmp_bytes + 16                    # the staged bytes start past the scratch
    assert call(a) == EWORKSPACE
    for field in ("tmp_cls_stride", "u8_cls_stride"):
        a, keep = _valid_args(L)
        setattr(a, field, getattr(a, field) - 16)       # smaller than one position's extent: positions would overlap
        assert call(a) == EWORKSPACE, field
        a, keep = _valid_args(L)
        setattr(a, field, getattr(a, field) + 16)       # position K - 1 leaves the buffer
        assert call(a) == EWORKSPACE, field
        a, keep = _valid_args(L, tab=[0, 1, 1, 2] + [1, 2] + [0] * 6)
        setattr(a, field, 0)                            # a stride holds one position even when K = 1
        assert call(a) == EWORKSPACE, field
    a, keep = _valid_args(L, K=2)                       # sized for two positions, the table's longest list has three
    assert call(a) == EWORKSPACE
    a, keep = _valid_args(L, with_u8=False, K=2)
    assert call(a) == EWORKSPACE
    a, keep = _valid_args(L)
    last = keep["t"].items[2]
    a.weights_bytes = last.yc_off + 4 * last.h * last.yk - 1    # one byte short of the last image's y weights
    assert call(a) == EWORKSPACE
    a, keep = _valid_args(L)
    keep["t"].items[1].u8_off = -16
    assert call(a) == EWORKSPACE


# ---------------------------------------------------------------------------------------------- reference against reference
@pytest.mark.parametrize("flags", [dict(r_threshold=0.25), dict(r_threshold=0.0, threshold=0.3)], ids=["dyn", "fixed"])
@pytest.mark.parametrize("ids", [None, [5, 200, 5, 77]], ids=["labelmaps", "class_ids"])
def test_full_lists_equal_the_nway_native_reference(flags, ids):
    """off = (0, N, 2N, ...), lab = 1 + c, seg_u8 permuted from class-major: labels, counts and maxima are
    nway_native_ref's (batch_max = False) on its own discriminating input; with class_ids also through entry_ids (every
    class is a candidate, so "every other id is background" means the same in both)."""
    x = nn.discriminating_input()
    N, B = x.shape[:2]
    rng = np.random.default_rng(3)
    gts = [rng.choice(np.array([0, 1, 2, 3, 4, 5, 77, 200, 255], np.uint8), size=s) for s in nn.DISC_SIZES]
    want = nn.nway_native_ref(x, nn.DISC_SIZES, gts, class_ids=ids, ignore_value=255, **flags)
    ent = x.transpose(0, 1).contiguous().view(B * N, *x.shape[2:])
    off, lab = [q * N for q in range(B + 1)], [1 + c for _ in range(B) for c in range(N)]
    forms = [dict(class_ids=ids)] + ([dict(entry_ids=[ids[c] for _ in range(B) for c in range(N)])] if ids else [])
    for form in forms:
        got = cn.cand_native_ref(ent, off, lab, N, nn.DISC_SIZES, gts, ignore_value=255, **form, **flags)
        for i in range(B):
            assert np.array_equal(got["labels"][i], want["labels"][i].numpy()), i
            assert np.array_equal(got["seg_u8"][i], want["seg_u8"][i].numpy()), i
        assert np.array_equal(got["counts"], want["counts"].numpy())
        assert np.array_equal(got["mx"].reshape(B, N).T, want["mx"].numpy())
    assert int(want["counts"][:, 0, 1:].sum()) > 0


@pytest.fixture(scope="module")
def disc():
    x = cn.discriminating_input()
    return dict(x=x, res=cn.resized(x, cn.DISC_OFF, cn.DISC_SIZES), ids=cn.disc_gts("ids"), labels=cn.disc_gts("labels"))


def _differs(a, b):
    return any(not np.array_equal(p, q) for p, q in zip(a["labels"], b["labels"])) or not np.array_equal(a["counts"], b["counts"])


def test_discriminating_input_discriminates(disc):
    """The input of the GPU tests separates the rule from its plausible misreadings: thresholds from the SOURCE maxima, the
    tie given to the later entry, a ground-truth class outside the candidates dropped instead of missed -- and from the
    processing-size rule resized, local from set labels, and the padding."""
    x, res = disc["x"], disc["res"]
    assert tuple(x.shape) == (cn.DISC_E_CAP, 3) + cn.DISC_SRC and cn.DISC_OFF[-1] == cn.DISC_E
    lab, nlabels, entry_ids = cn.disc_tables("set")
    assert lab == [1, 3, 1, 2, 4, 0, 0, 0] and nlabels == 4 and entry_ids == [10, 30, 10, 20, 40, 40, 40, 40]
    kw = dict(ignore_value=cn.DISC_IGNORE, res=res)
    r = cn.cand_native_ref(x, cn.DISC_OFF, lab, 4, cn.DISC_SIZES, disc["ids"], class_ids=cn.DISC_CLASS_IDS, **kw)
    assert [tuple(l.shape) for l in r["labels"]] == cn.DISC_SIZES
    src_mx = x.reshape(cn.DISC_E_CAP, -1).max(1).values.numpy().astype(np.int32)
    assert r["mx"].tolist() == [225, 93, 255, 199, 255, 0, 0, 0] and src_mx.tolist() == [200, 93, 230, 180, 230, 255, 255, 255]
    # 1. thresholds from the source maxima: the overshoot block's border falls on the other side
    before = cn.cand_native_ref(x, cn.DISC_OFF, lab, 4, cn.DISC_SIZES, disc["ids"], class_ids=cn.DISC_CLASS_IDS, mx=src_mx, **kw)
    assert not np.array_equal(before["labels"][0], r["labels"][0]) and _differs(before, r)
    # 2. the tie: entries 2 and 4 (classes 0 and 3 of query 2) hold the same bytes; the earlier one wins everywhere
    assert (r["labels"][2] == 1).any() and not (r["labels"][2] == 4).any()
    assert r["area"][4, 0] == r["area"][2, 0] > 0 and r["area"][4, 1] == 0 and r["area"][2, 1] > 0
    swapped = cn.cand_native_ref(x, cn.DISC_OFF, [1, 3, 4, 2, 1, 0, 0, 0], 4, cn.DISC_SIZES, disc["ids"],
                                 class_ids=cn.DISC_CLASS_IDS, **kw)
    assert (swapped["labels"][2] == 4).any() and _differs(swapped, r)
    # 3. a ground-truth class that is no candidate of the query: a miss in its label's union, not a dropped pixel
    cand_labels = [{0} | {lab[e] for e in range(cn.DISC_OFF[q], cn.DISC_OFF[q + 1])} for q in range(3)]

    def dropped(q, gt):
        g = nn.target_map(gt, 4, cn.DISC_CLASS_IDS, cn.DISC_IGNORE).numpy().copy()
        g[~np.isin(g, list(cand_labels[q]))] = 255
        return g
    drop = cn.cand_native_ref(x, cn.DISC_OFF, lab, 4, cn.DISC_SIZES, disc["ids"], target=dropped, **kw)
    assert not np.array_equal(drop["counts"], r["counts"])
    assert r["counts"][0, 1, 2] > 0 and r["counts"][0, 0, 2] == 0 and drop["counts"][0, 1, 2] == 0     # class 1 in query 0
    assert r["counts"][1, 1, 1:].sum() > 0 and not r["labels"][1].any()                                # the empty query misses all
    # the ground truth holds what the kernel must treat specially
    for g in disc["ids"]:
        assert set(np.unique(g)) == {0, 10, 20, 30, 40, 77, 255}
    kept = [(g != 255).sum() for g in disc["ids"]]
    assert [int(r["counts"][q, 1].sum() + 0) >= int(k) for q, k in enumerate(kept)] == [True] * 3
    # local labels: other labels, other counts; entry_ids: an id outside the query's candidates is background
    llab, lnl, _ = cn.disc_tables("local")
    assert llab == [1, 2, 1, 2, 3, 0, 0, 0] and lnl == 3
    loc = cn.cand_native_ref(x, cn.DISC_OFF, llab, 3, cn.DISC_SIZES, disc["ids"], entry_ids=entry_ids, **kw)
    assert loc["counts"].shape == (3, 2, 4) and (loc["labels"][0] == 2).any()
    assert loc["counts"][1, 1, 1:].sum() == 0 and loc["counts"][1, 0, 0] == kept[1]                     # empty query: all background
    # the label rule at the processing size, resized (nearest), is another map
    import cand_ref
    small = cand_ref.seg_labels_cand(x.numpy(), src_mx, cn.DISC_OFF, lab, 4)[0]
    for q in (0, 2):
        up = torch.nn.functional.interpolate(torch.from_numpy(small[q])[None, None].float(), size=cn.DISC_SIZES[q],
                                             mode="nearest")[0, 0].to(torch.uint8).numpy()
        assert not np.array_equal(up, r["labels"][q]), q
    # label maps without a table: 77 is above nlabels and dropped, as the ignore value
    m = cn.cand_native_ref(x, cn.DISC_OFF, lab, 4, cn.DISC_SIZES, disc["labels"], **kw)
    for q in range(3):
        g = disc["labels"][q]
        assert int(m["counts"][q, 1].sum()) >= int(((g != 255) & (g != 77)).sum()) > 0
    # int32 maps hold ids past the 256-entry table and negative ones
    wide = cn.disc_gts("ids", np.int32)
    assert all(g.dtype == np.int32 and (g == 1000).any() and (g == -3).any() for g in wide)


def test_padding_is_never_looked_at(disc):
    x = disc["x"].clone()
    lab, _, _ = cn.disc_tables("set")
    kw = dict(class_ids=cn.DISC_CLASS_IDS, ignore_value=cn.DISC_IGNORE)
    a = cn.cand_native_ref(x, cn.DISC_OFF, lab, 4, cn.DISC_SIZES, disc["ids"], res=disc["res"], **kw)
    x[cn.DISC_E:] = 7
    b = cn.cand_native_ref(x, cn.DISC_OFF, lab[:5] + [9, 9, 9], 4, cn.DISC_SIZES, disc["ids"], **kw)
    assert not _differs(a, b) and np.array_equal(a["area"], b["area"]) and not a["area"][cn.DISC_E:].any()
    assert np.array_equal(a["mx"], b["mx"])


# ---------------------------------------------------------------------------------------------- host logic
def _sets(nsets=4, shots=1):
    from diffews_amd import config
    from diffews_amd.unet import SupportBankSet, bank_layout
    cfg = config.get("tiny_unet")
    dt, hw = torch.bfloat16, (8, 8)
    layout = bank_layout(cfg, *hw)
    kv = lambda: [torch.zeros(nsets * shots, t, c, dtype=dt) for t, c in layout]
    return SupportBankSet(kv(), kv(), nsets, shots, hw, dt, dt, (1.0, "folded", 1), 1, layout)


def test_candidate_tables_gain_K_and_entry_sets():
    s = _sets()
    for labels in ("set", "local"):
        t = s.candidate_tables([(2, 0), (), (0, 1, 3)], 8, labels)
        assert t["K"] == 3 and t["E"] == 5 and t["E_pad"] == 8
        assert t["entry_sets"].dtype == torch.int32 and t["entry_sets"].tolist() == [0, 2, 0, 1, 3, 3, 3, 3]
        assert t["tab"][:4].tolist() == cn.DISC_OFF
        assert set(t) == {"entries", "rows", "tab", "E", "E_pad", "nlabels", "sets", "K", "entry_sets"}
    assert s.candidate_tables([(1,), (3,)], 1)["K"] == 1
    lab, nl, ids = cn.disc_tables("local")
    t = s.candidate_tables([(2, 0), (), (0, 1, 3)], 8, "local")
    assert t["tab"][4:].tolist() == lab and t["nlabels"] == nl
    assert [cn.DISC_CLASS_IDS[c] for c in t["entry_sets"].tolist()] == ids


def test_workspace_is_sized_by_the_longest_list():
    from diffews_amd import ops
    from diffews_amd.input_pipeline import NativeTargets
    t = NativeTargets(cn.DISC_SRC, cn.DISC_SIZES, device=None)
    for K in (1, 3, 254):
        assert ops.cand_native_workspace(t, K, want_u8=True) == (K * t.tmp_bytes, K * t.tmp_bytes, K * t.u8_bytes)
        assert ops.cand_native_workspace(t, K) == (K * (t.tmp_bytes + t.u8_bytes), K * t.tmp_bytes, 0)
    assert ops.cand_native_workspace(t, 0) == ops.cand_native_workspace(t, 1)           # a batch of empty lists
    # E_cap does not enter: 8 entries with a longest list of 3 need 3 strides, and the library agrees (see the
    # EWORKSPACE cases of test_validates_on_the_host_before_any_launch, sized with K and K - 1)
    assert ops.cand_native_workspace(t, 3)[0] < 8 * (t.tmp_bytes + t.u8_bytes)


def test_op_argument_errors():
    """ops.seg_labels_cand_native refuses, before it touches a GPU, tables of the wrong kind and both id tables."""
    from diffews_amd import ops
    from diffews_amd.input_pipeline import NativeTargets
    u8 = torch.zeros(8, 3, 32, 32, dtype=torch.uint8)
    t = torch.tensor(cn.DISC_OFF + cn.disc_tables()[0], dtype=torch.int32)
    tg = NativeTargets(cn.DISC_SRC, cn.DISC_SIZES, device=None)
    for tab, th in ((t[:9], t), (t.long(), t), (t, t.long()), (t[:1], t[:1]), (t.view(2, 6), t)):
        with pytest.raises(ValueError):
            ops.seg_labels_cand_native(u8, tg, tab, th, 4)
    with pytest.raises(ValueError):                            # the device table lives on the device
        ops.seg_labels_cand_native(u8, tg, t, t, 4)


def _fake_pipe():
    """The argument checks of segment_candidates_native / segment_stream run before anything touches the models: a pipeline
    object that has none."""
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise as P
    pipe = object.__new__(P)
    pipe.device = "cpu"
    return pipe


def test_pipeline_argument_errors():
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise as P
    s = _sets()
    q = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="NativeTargets"):     # class_ids without targets
        P.segment_candidates_native(_fake_pipe(), s, q, [(0,)], None, class_ids=[1, 2, 3, 4])
    with pytest.raises(ValueError):                            # still a SupportBankSet only
        P.segment_candidates_native(_fake_pipe(), object(), q, [(0,)], object())
    with pytest.raises(TypeError):                             # the plain call takes neither
        P.segment_candidates(_fake_pipe(), s, q, [(0,)], class_ids=[1, 2, 3, 4])
    pipe = _fake_pipe()
    pipe.vae = type("V", (), {"config": {"block_out_channels": [1, 1, 1, 1]}})()
    qs = [dict(query_img=np.zeros((8, 8, 3), np.uint8), cand=(0,))]
    with pytest.raises(ValueError, match="native"):            # class_ids only with native=True
        next(P.segment_stream(pipe, s, qs, candidates="cand", class_ids=[1, 2, 3, 4]))
    with pytest.raises(ValueError, match="batch_max"):
        next(P.segment_stream(pipe, s, qs, candidates="cand", batch_max=True, native=True))
    with pytest.raises(ValueError):                            # route and candidates together, as before
        next(P.segment_stream(pipe, s, qs, candidates="cand", route="cand", native=True))
    from diffews_amd import evaluate
    with pytest.raises(ValueError, match="use_original_imgsize"):
        evaluate.evaluate_candidates(pipe, s, [], class_ids=[1, 2, 3, 4])
