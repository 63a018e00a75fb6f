"""CPU tests (no GPU) of routed queries -- each query of a batch against ONE class of a SupportBankSet: the three entry
points of the routed launch through the header, the ctypes table and the host-only queries (validation, kernel name,
key-split plan, workspace -- none of which sees the route table), SupportBankSet.route_table on host tensors, and the
definition of the feature in the oracle's arithmetic, which tests/test_routed_gpu.py leans on."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import test_nway_cpu as nw
import test_support_bank_cpu as sb

DFW_EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(rows):
    flat = [int(x) for r in rows for x in r]
    return (C.c_int32 * len(flat))(*flat)


def _routed_name(L, a, nbank, min_shots):
    buf = C.create_string_buffer(96)
    L.check(L.lib().dfw_fsa_routed_kernel_name(C.byref(a), nbank, min_shots, buf, 96), "dfw_fsa_routed_kernel_name")
    return buf.value.decode()


def _routed_args(L, nbank, min_shots, workspace=True, **kw):
    """Host-only arguments of a routed launch; with `workspace`, the one the library asks for (so that the name shows the
    split plan)."""
    a = sb._fsa_args(L, **kw)
    if workspace:
        nb = L.lib().dfw_fsa_routed_workspace_bytes(C.byref(a), nbank, min_shots)
        if nb:
            a.workspace, a.workspace_bytes = 4096, nb
    return a


def _nsplit(name):
    return int(re.search(r"\+split(\d+)", name).group(1)) if "+split" in name else 1


def test_header_ctypes_and_symbols(hip_lib):
    """The three entry points are declared with the issue's signatures, bound in _lib.SYMBOLS with matching argument lists
    and exported; the library reports version >= 109; dfw_fsa_args is untouched."""
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int dfw_fsa_attention_routed(const dfw_fsa_args* a, const int32_t* table, const int32_t* table_host, "
            "int32_t nbank, int32_t min_shots, dfw_stream_t stream);") in flat
    assert ("int dfw_fsa_routed_kernel_name(const dfw_fsa_args* a, int32_t nbank, int32_t min_shots, char* buf, "
            "size_t n);") in flat
    assert "size_t dfw_fsa_routed_workspace_bytes(const dfw_fsa_args* a, int32_t nbank, int32_t min_shots);" in flat
    i32, vp, pi = C.c_int32, C.c_void_p, C.POINTER(C.c_int32)
    # table: a device pointer (an address), table_host: a host int32 array
    assert L.SYMBOLS["dfw_fsa_attention_routed"] == (i32, [C.POINTER(L.FsaArgs), vp, pi, i32, i32, vp])
    assert L.SYMBOLS["dfw_fsa_routed_kernel_name"] == (i32, [C.POINTER(L.FsaArgs), i32, i32, C.c_char_p, C.c_size_t])
    assert L.SYMBOLS["dfw_fsa_routed_workspace_bytes"] == (C.c_size_t, [C.POINTER(L.FsaArgs), i32, i32])
    for name in ("dfw_fsa_attention_routed", "dfw_fsa_routed_kernel_name", "dfw_fsa_routed_workspace_bytes"):
        assert getattr(hip_lib, name) is not None
    assert hip_lib.dfw_version() >= 109
    assert L.FsaArgs._fields_[-1] == ("bank_shared", i32)


def test_host_validation(hip_lib):
    """Everything that is not a routed launch is DFW_EINVAL from the launch and the name query (0 bytes from the workspace
    query); a bad table is DFW_EINVAL from the launch -- all on the host, before any launch, so safe without a GPU."""
    from diffews_amd import _lib as L
    h = L.lib()
    buf = C.create_string_buffer(96)
    ok = dict(batch=4, heads=2, n_q=128, n_kv=128, n_bank=128, nshot=3)
    nbank, mn = 6, 1                                     # a library of shots (1, 3, 2)
    good = [(4, 2), (0, 1), (1, 3), (1, 3)]
    a = sb._fsa_args(L, **ok)
    assert h.dfw_fsa_routed_kernel_name(C.byref(a), nbank, mn, buf, 96) == 0
    assert buf.value.decode().endswith("+routed")
    assert h.dfw_fsa_routed_kernel_name(C.byref(a), nbank, 3, buf, 96) == 0          # min_shots == nshot: the most
    assert h.dfw_fsa_routed_kernel_name(C.byref(a), 1, mn, buf, 96) == 0             # nbank 1: the least
    bad_plan = [
        ("null args", None, nbank, mn),
        ("null q", dict(ok, q=0), nbank, mn),
        ("batch 0", dict(ok, batch=0), nbank, mn),
        ("dtype", dict(ok, dtype=7), nbank, mn),
        ("n_plain > 0", dict(ok, n_plain=2), nbank, mn),
        ("bank_shared", dict(ok, bank_shared=1), nbank, mn),
        ("nshot 0", dict(ok, nshot=0, n_bank=0), nbank, mn),
        ("nshot < 0", dict(ok, nshot=-1), nbank, mn),
        ("nbank 0", ok, 0, mn),
        ("nbank < 0", ok, -3, mn),
        ("min_shots 0", ok, nbank, 0),
        ("min_shots < 0", ok, nbank, -1),
        ("min_shots > nshot", ok, nbank, 4),
    ]
    for what, fields, nb, m in bad_plan:
        a = None if fields is None else sb._fsa_args(L, **fields)
        ref = None if a is None else C.byref(a)
        assert h.dfw_fsa_attention_routed(ref, 4096, _table(good), nb, m, None) == DFW_EINVAL, what
        assert h.dfw_fsa_routed_kernel_name(ref, nb, m, buf, 96) == DFW_EINVAL, what
        assert h.dfw_fsa_routed_workspace_bytes(ref, nb, m) == 0, what
    a = sb._fsa_args(L, **ok)
    bad_rows = [
        ("null table", None, good, nbank, mn),
        ("null table_host", 4096, None, nbank, mn),
        ("first < 0", 4096, [(4, 2), (-1, 1), (1, 3), (1, 3)], nbank, mn),
        ("shots 0", 4096, [(4, 2), (0, 0), (1, 3), (1, 3)], nbank, mn),
        ("shots < 0", 4096, [(4, 2), (0, -2), (1, 3), (1, 3)], nbank, mn),
        ("shots < min_shots", 4096, [(4, 2), (0, 1), (1, 3), (1, 3)], nbank, 2),
        ("shots > nshot", 4096, [(2, 4), (0, 1), (1, 3), (1, 3)], nbank, mn),
        ("first + shots > nbank", 4096, [(5, 2), (0, 1), (1, 3), (1, 3)], nbank, mn),
        ("first + shots > nbank (last row)", 4096, [(4, 2), (0, 1), (1, 3), (4, 3)], nbank, mn),
        ("first == nbank", 4096, [(6, 1), (0, 1), (1, 3), (1, 3)], nbank, mn),
        ("first + shots overflows", 4096, [(2 ** 31 - 1, 3), (0, 1), (1, 3), (1, 3)], nbank, mn),
    ]
    for what, table, rows, nb, m in bad_rows:
        th = None if rows is None else _table(rows)
        assert h.dfw_fsa_attention_routed(C.byref(a), table, th, nb, m, None) == DFW_EINVAL, what
    from diffews_amd import ops
    q = torch.zeros(4, 128, 128, dtype=torch.bfloat16)
    t = torch.tensor(good, dtype=torch.int32)
    for tab, th in ((t[:3], t), (t, t[:3]), (t.long(), t), (t, t.t().contiguous().t())):
        with pytest.raises(ValueError):                  # ops: both tables are contiguous int32 [B, 2]
            ops.fsa_attention_routed(q, q, q, 2, q[:3], q[:3], tab, th, 3, 1)
    with pytest.raises(ValueError):                      # ops: the device table lives on the device
        ops.fsa_attention_routed(q, q, q, 2, q[:3], q[:3], t, t, 3, 1)


def test_plan_never_sees_the_table(hip_lib):
    """The name and workspace queries take no table, so two routes cannot plan differently: their signatures (C header,
    ctypes) hold no pointer to one.  The name is the unshared name + "+routed"; the split is dfw_fsa_attention's rule on
    batch * (1 + nshot) segments, clamped to 1 + min_shots, and the workspace is the partial buffer of the split shown."""
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for fn in ("dfw_fsa_routed_kernel_name", "dfw_fsa_routed_workspace_bytes"):
        decl = re.search(fn + r"\(([^)]*)\)", flat).group(1)
        assert "table" not in decl and "int32_t*" not in decl, decl
        assert C.POINTER(C.c_int32) not in L.SYMBOLS[fn][1] and L.SYMBOLS[fn][1].count(C.c_void_p) == 0, fn
    shape = dict(heads=2, n_q=2048, n_kv=2048, n_bank=2048)
    for dt in (L.BF16, L.F16):
        # the unclamped plan of (5, 5): the unshared launch's own name and workspace
        a = _routed_args(L, 10, 5, dtype=dt, batch=2, nshot=5, **shape)
        full = _routed_name(L, a, 10, 5)
        assert full == sb._name(L, a) + "+routed" and _nsplit(full) > 2, full
        assert L.lib().dfw_fsa_routed_workspace_bytes(C.byref(a), 10, 5) == L.lib().dfw_fsa_workspace_bytes(C.byref(a))
        seen = []
        for mn in (5, 4, 3, 2, 1):
            a = _routed_args(L, 8, mn, dtype=dt, batch=2, nshot=5, **shape)
            name = _routed_name(L, a, 8, mn)
            assert name.endswith("+routed") and _nsplit(name) <= 1 + mn, (mn, name)
            assert _nsplit(name) == min(_nsplit(full), 1 + mn), (mn, name, full)
            seen.append(_nsplit(name))
        assert seen == sorted(seen, reverse=True) and seen[-1] == 2 and seen[0] > seen[-1], seen
    cases = [(8, 3, dict(batch=4, nshot=5, **shape)), (6, 1, dict(batch=5, nshot=3, heads=1, n_q=1100, n_kv=1100, n_bank=1100)),
             (9, 2, dict(batch=4, nshot=7, heads=5, n_q=4096, n_kv=4096, n_bank=4096)),
             (3, 1, dict(batch=3, nshot=2, heads=2, n_q=256, n_kv=256, n_bank=321)),
             (3, 1, dict(batch=4, nshot=2, heads=4, n_q=1024, n_kv=1024, n_bank=1024))]
    some = set()
    for nbank, mn, shp in cases:
        a = _routed_args(L, nbank, mn, workspace=False, **shp)
        nb = L.lib().dfw_fsa_routed_workspace_bytes(C.byref(a), nbank, mn)
        assert "+split" not in _routed_name(L, a, nbank, mn)               # no workspace passed: unsplit
        a = _routed_args(L, nbank, mn, **shp)
        name = _routed_name(L, a, nbank, mn)
        assert name.startswith("fsa_ring_kernel<bf16,") and name.endswith(",1,pre>" + name[name.index(">") + 1:]), name
        assert name.endswith("+routed") and "+shared" not in name and "+ragged" not in name, name
        assert (nb == 0) == ("+split" not in name), (name, nb)
        assert _nsplit(name) <= 1 + mn, (mn, name)
        assert (",8,1," if shp["n_q"] > 1024 else ",4,1,") in name, name
        assert ("+xcd" in name) == ((shp["heads"] * shp["batch"] * _nsplit(name)) % 8 == 0), name
        if nb:
            assert nb == a.batch * _nsplit(name) * a.heads * a.n_q * 68 * 4, (name, nb)
        # nbank moves the bank descriptor, not the plan
        assert _routed_name(L, a, nbank + 5, mn) == name
        some.add(nb != 0)
    assert some == {True, False}


def test_route_table():
    """SupportBankSet.route_table on host tensors: row i = (offsets[route[i]], shots[route[i]]) as a contiguous int32
    [b, 2] host tensor, for a ragged and a uniform set, any order, repeats, unused sets; an empty route and an index
    outside [0, nsets) raise ValueError."""
    from diffews_amd import config
    from diffews_amd.unet import SupportBankSet, bank_layout
    cfg = config.get("tiny_unet")
    dt, hw = torch.bfloat16, (8, 8)
    layout = bank_layout(cfg, *hw)
    key = (1.0, "folded", 1)
    kv = lambda n: [torch.zeros(n, t, c, dtype=dt) for t, c in layout]
    ragged = SupportBankSet(kv(6), kv(6), 3, (1, 3, 2), hw, dt, dt, key, 1, layout)
    uniform = SupportBankSet(kv(6), kv(6), 3, 2, hw, dt, dt, key, 1, layout)
    t = ragged.route_table((2, 0, 2, 1))
    assert t.dtype == torch.int32 and t.device.type == "cpu" and t.is_contiguous() and tuple(t.shape) == (4, 2)
    assert t.tolist() == [[4, 2], [0, 1], [4, 2], [1, 3]]
    assert ragged.route_table([1]).tolist() == [[1, 3]]
    assert ragged.route_table(torch.tensor([0, 0, 0])).tolist() == [[0, 1]] * 3         # repeats; sets 1 and 2 unused
    assert ragged.route_table(range(3)).tolist() == [[0, 1], [1, 3], [4, 2]]
    assert uniform.route_table((2, 0, 2, 1)).tolist() == [[4, 2], [0, 2], [4, 2], [2, 2]]
    for st in (ragged, uniform):
        for i, (first, n) in enumerate(st.route_table(range(3)).tolist()):
            assert st.bank(i).nshot == n and first + n <= st.k[0].shape[0]
        for bad in ((), [], (0, 3), (-1, 0), (0, 1, 99)):
            with pytest.raises(ValueError):
                st.route_table(bad)


def test_public_signatures():
    """The Python surface the issue names, argument for argument."""
    from diffews_amd import evaluate, ops
    from diffews_amd.pipeline import MarigoldPipelineRGBLatentNoise as P
    from diffews_amd.unet import MyUNet2DConditionModel as U
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(ops.fsa_attention_routed) == ["q", "k", "v", "heads", "k_bank", "v_bank", "table", "table_host", "max_shots",
                                               "min_shots", "q_prescaled", "key_split", "out"]
    assert callable(ops._fsa_routed_call)
    assert names(U.forward_query_routed) == ["self", "z_tag", "timestep", "bankset", "table", "table_host",
                                             "encoder_hidden_states", "out_scale"]
    assert names(P.segment_routed) == ["self", "bankset", "query_img", "route", "query_gt", "r_threshold", "threshold",
                                       "batch_max", "captured", "native"]
    sig = inspect.signature(P.segment_stream).parameters
    assert "route" in sig and sig["route"].default is None
    assert names(evaluate.evaluate_routed)[:7] == ["pipe", "bankset", "queries", "class_of_set", "gt_ids", "benchmark", "fold"]


def test_oracle_definition_of_routed_queries():
    """The definition of the feature, in the reference's own arithmetic (fp32 oracle, tiny config, library shots (1, 3, 2),
    route (2, 0, 2, 1)): entry i is the reference's own episode -- oracle.pipeline.pipeline_call with b = 1, query i and the
    supports of class route[i].  The entries of a reference call are independent of each other (entry i of a b-query call
    against ONE class is the one-query call), so a batch whose entries read different classes is defined entry by entry
    although no single reference call can hold it; and the route matters: the same query against another class is another
    result."""
    from oracle import pipeline as op
    ou, ov, te = nw._oracle()
    g = torch.Generator().manual_seed(23)
    shots, route, H = (1, 3, 2), (2, 0, 2, 1), 64
    sup = [torch.rand(s, 3, H, H, generator=g) * 2 - 1 for s in shots]
    msk = [(torch.rand(s, 1, H, H, generator=g) > 0.5).float().repeat(1, 3, 1, 1) * 2 - 1 for s in shots]
    qry = torch.rand(len(route), 3, H, H, generator=g) * 2 - 1
    rep = lambda t, n: t.repeat(n, 1, 1, 1)
    one = []
    for i, c in enumerate(route):
        m1, r1 = op.pipeline_call(ou, ov, [sup[c], qry[i:i + 1], msk[c]], te)
        assert r1["z0"].shape[0] == 1 and len(m1) == 1
        one.append((m1[0], r1["z0"][0]))
    # entries 0 and 2 share class 2: the b = 2 reference call on them is, entry by entry, the two episodes
    pair = [0, 2]
    masks, whole = op.pipeline_call(ou, ov, [rep(sup[2], 2), qry[pair], rep(msk[2], 2)], te)
    scale = float(whole["z0"].abs().max())
    for j, i in enumerate(pair):
        assert torch.allclose(one[i][1], whole["z0"][j], rtol=1e-5, atol=1e-5 * scale), i
        assert (abs(one[i][0].astype(int) - masks[j].astype(int)) > 1).mean() < 1e-3, i
    # the route matters: query 1 against class 1 instead of class 0 is another function of the query
    _, other = op.pipeline_call(ou, ov, [sup[1], qry[1:2], msk[1]], te)
    d = float((other["z0"][0] - one[1][1]).norm() / one[1][1].norm())
    assert d > 1e-4, d          # ten times the tolerance of the equalities above
