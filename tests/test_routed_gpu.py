"""GPU tests of routed queries -- each query of a batch against ONE class of a SupportBankSet.

Attention: ops.fsa_attention_routed per entry against ops.fsa_attention on that entry's set (a slice of the stack; exact,
key split off), per element against the fp64 bound of tests/attention_bound.py under the default plan, with the table
rewritten in place between two launches and between two replays of one captured launch, with the stack at the very end
of its allocation, and against ops.fsa_attention_ragged on the identity route.

Pipeline (tiny config, 64 x 64, library shots (1, 3, 2) and a uniform one, b = 4, route (2, 0, 2, 1)): segment_routed per
entry against the fp32 oracle's b = 1 episode and against segment_queries on .bank(route[i]), counts exactly against the
post-processing reference, captured against eager with ONE graph for every route, at native sizes, through
segment_stream(route=...) and evaluate_routed.

The oracle side relies on test_routed_cpu.test_oracle_definition_of_routed_queries: entry i of a routed batch is the
reference's own episode with query i and the supports of class route[i]."""
import contextlib
import ctypes as C

import pytest
import torch

import attention_bound as ab
from test_glue_exact_gpu import seg_counts_ref
from test_model_gpu import TOL_EP
from test_native_gpu import _check_native, _gts
from test_ragged_sets_gpu import RAGGED_CASES, _classes, _cuda, _offsets
from test_support_bank_gpu import models, ops, rel, _bank, _qkv, _queries  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


# ------------------------------------------------------------------------------------------------ routed attention

@contextlib.contextmanager
def routed_names(ops, L):
    """Record dfw_fsa_routed_kernel_name of every dfw_fsa_attention_routed call ops makes (and launch it)."""
    names, orig = [], ops._fsa_routed_call

    def rec(a, table, table_host, nbank, min_shots):
        buf = C.create_string_buffer(96)
        L.check(L.lib().dfw_fsa_routed_kernel_name(C.byref(a), nbank, min_shots, buf, 96), "dfw_fsa_routed_kernel_name")
        names.append(buf.value.decode())
        orig(a, table, table_host, nbank, min_shots)

    ops._fsa_routed_call = rec
    try:
        yield names
    finally:
        ops._fsa_routed_call = orig


ROUTED_CASES = [   # (id, library shots, route, heads, n_q, n_bank)
    ("nw8_tail", (1, 3, 2), (2, 0, 1, 1, 2), 1, 1100, 1100),       # ragged last query block and key tile
    ("nw4_nbank321", (2, 1), (1, 0, 0), 2, 256, 321),              # 4-wave form, ragged bank tile
    ("xcd", (1, 2), (1, 0, 1, 1), 4, 1024, 1024),                  # heads x batch % 8 == 0: the XCD re-map
    ("split", (5, 3), (1, 0, 0, 1), 2, 2048, 2048),                # takes a key split, clamped to 1 + 3
    ("sd21_64x64", (1, 2, 1), (0, 2, 1, 1), 5, 4096, 4096),        # the UNet's 64^2-level shape
]
CASE_IDS = [c[0] for c in ROUTED_CASES]


def _table(shots, route):
    off = _offsets(shots)
    return torch.tensor([[off[c], shots[c]] for c in route], dtype=torch.int32)


def _inputs(case, dtype, seed):
    cid, shots, route, heads, n_q, n_bank = case
    g = torch.Generator(device="cuda").manual_seed(seed)
    q, k, v = _qkv(len(route), n_q, heads, dtype, g)
    kb, vb = _bank(sum(shots), n_bank, heads, dtype, g)       # random and distinct sets
    return q, k, v, kb, vb


def _routed(ops, q, k, v, heads, kb, vb, shots, route, table=None, mirror=None, **kw):
    host = _table(shots, route) if mirror is None else mirror
    table = host.cuda() if table is None else table
    return ops.fsa_attention_routed(q, k, v, heads, kb, vb, table, host, max(shots), min(shots), q_prescaled=True, **kw)


def _per_entry(ops, q, k, v, heads, kb, vb, shots, route):
    """The unsplit reference: every entry through ops.fsa_attention on its own set's slice of the stack."""
    off, out = _offsets(shots), []
    for i, c in enumerate(route):
        e, s = slice(i, i + 1), shots[c]
        out.append(ops.fsa_attention(q[e], k[e], v[e], heads, kb[off[c]:off[c] + s], vb[off[c]:off[c] + s], nshot=s,
                                     q_prescaled=True, bank_shared=True, key_split=False))
    return torch.cat(out)


def _other_route(shots, route):
    """Another valid route of the same length that differs from `route` in every entry."""
    n = len(shots)
    return tuple((c + 1) % n for c in route)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", ROUTED_CASES, ids=CASE_IDS)
def test_routed_equals_per_entry_launches_exactly(ops, case, dtype):
    """key_split=False: every entry of the routed launch is torch.equal to fsa_attention on that entry's set (bank_shared,
    unsplit) -- same kernel arithmetic, key order and tile sequence.  Another route gives another result, equal to ITS
    per-entry reference."""
    from diffews_amd import _lib as L
    cid, shots, route, heads, n_q, n_bank = case
    q, k, v, kb, vb = _inputs(case, dtype, 41)
    with routed_names(ops, L) as got:
        y = _routed(ops, q, k, v, heads, kb, vb, shots, route, key_split=False)
    assert got[0].endswith("+routed") and "+split" not in got[0], got
    assert (",8,1," if n_q > 1024 else ",4,1,") in got[0], got
    if cid == "xcd":
        assert "+xcd" in got[0], got
    ref = _per_entry(ops, q, k, v, heads, kb, vb, shots, route)
    for i in range(len(route)):
        assert torch.equal(y[i], ref[i]), (cid, i, got, rel(y[i], ref[i]))
    other = _other_route(shots, route)
    y2 = _routed(ops, q, k, v, heads, kb, vb, shots, other, key_split=False)
    assert not torch.equal(y2, y)
    assert torch.equal(y2, _per_entry(ops, q, k, v, heads, kb, vb, shots, other))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", ROUTED_CASES, ids=CASE_IDS)
def test_routed_per_element_bound(ops, case, dtype):
    """Default plan (key_split=True): every output element of every entry against the fp64 reference and error allowance
    of tests/attention_bound.py on that entry's keys [own ; its set].  `split` takes a key split (at most 1 + min(shots)):
    a split result is not bit-equal to the unsplit one, and both pass the bound."""
    from diffews_amd import _lib as L
    cid, shots, route, heads, n_q, n_bank = case
    q, k, v, kb, vb = _inputs(case, dtype, 43)
    off = _offsets(shots)

    def run(key_split):
        with routed_names(ops, L) as names:
            y = _routed(ops, q, k, v, heads, kb, vb, shots, route, key_split=key_split)
        return y, names[0]

    def bound(y, name, what):
        nsplit = int(name.split("+split")[1].split("+")[0]) if "+split" in name else 1
        rows = 256 if ",8,1," in name else 128
        worst = 0.0
        for i, c in enumerate(route):
            s = shots[c]
            segs = ab.key_segments(k[i:i + 1], v[i:i + 1], 0, 0, s, kb[off[c]:off[c] + s], vb[off[c]:off[c] + s])
            assert len(segs) == 1 + s
            r = torch.empty(1, n_q, heads * 64, dtype=ab.F64, device="cuda")
            e = torch.empty_like(r)
            for h in range(heads):
                sl = slice(h * 64, (h + 1) * 64)
                K = torch.cat([sg[1][:, sl] for sg in segs])
                V = torch.cat([sg[2][:, sl] for sg in segs])
                r[0, :, sl], e[0, :, sl], _, _ = ab.fwd_ref(q[i][:, sl], K, V, dtype, c=1.0, nsplit=nsplit)
            w = ab.check(y[i:i + 1], r, e, dtype, where=ab.Where(n_q, heads, rows), label=f"routed {cid} entry {i} {what}")
            worst = max(worst, w)
        print(f"[routed] {cid} {dtype} {what}: {name}: worst out {worst:.3f} of the allowance")

    y, name = run(True)
    assert name.endswith("+routed"), name
    if cid == "split":
        assert "+split" in name, name
    bound(y, name, "default plan")
    if "+split" in name:       # `split` must; the plan sizes every entry for the longest set, so sd21_64x64 does too
        nsplit = int(name.split("+split")[1].split("+")[0])
        assert 2 <= nsplit <= 1 + min(shots), name
        y0, name0 = run(False)
        assert "+split" not in name0 and not torch.equal(y, y0), (name, name0)
        bound(y0, name0, "unsplit")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", [ROUTED_CASES[0], ROUTED_CASES[1]], ids=CASE_IDS[:2])
def test_table_is_read_when_the_kernel_runs(ops, case, dtype):
    """Launch, overwrite the SAME device table tensor in place with another valid route, launch again with otherwise
    identical arguments (the host mirror still holds the first route: it is validated, never used by the kernel): the second
    result is the second route's per-entry reference exactly."""
    cid, shots, route, heads, n_q, n_bank = case
    q, k, v, kb, vb = _inputs(case, dtype, 45)
    mirror = _table(shots, route)
    table = mirror.cuda()
    y1 = _routed(ops, q, k, v, heads, kb, vb, shots, route, table=table, mirror=mirror, key_split=False).clone()
    assert torch.equal(y1, _per_entry(ops, q, k, v, heads, kb, vb, shots, route))
    other = _other_route(shots, route)
    ptr = table.data_ptr()
    table.copy_(_table(shots, other))
    assert table.data_ptr() == ptr
    y2 = _routed(ops, q, k, v, heads, kb, vb, shots, route, table=table, mirror=mirror, key_split=False)
    assert not torch.equal(y2, y1)
    assert torch.equal(y2, _per_entry(ops, q, k, v, heads, kb, vb, shots, other))


def test_one_captured_launch_serves_every_route(ops):
    """The launch captured in a torch.cuda.graph and replayed after the table changed: each replay equals its own route's
    per-entry reference exactly, with the key split on (`split`: the plan does not depend on the route either)."""
    case, dtype = ROUTED_CASES[3], torch.bfloat16
    cid, shots, route, heads, n_q, n_bank = case
    q, k, v, kb, vb = _inputs(case, dtype, 47)
    routes = [route, _other_route(shots, route), (0, 0, 1, 1)]
    mirror = _table(shots, route)
    table = mirror.cuda()
    out = torch.empty(q.shape, dtype=dtype, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _routed(ops, q, k, v, heads, kb, vb, shots, route, table=table, mirror=mirror, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _routed(ops, q, k, v, heads, kb, vb, shots, route, table=table, mirror=mirror, out=out)
    seen = []
    for rt in routes + [route]:
        table.copy_(_table(shots, rt), non_blocking=False)
        graph.replay()
        got = out.clone()
        eager = _routed(ops, q, k, v, heads, kb, vb, shots, rt)              # the same plan, launched eagerly
        assert torch.equal(got, eager), rt
        seen.append(got)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and torch.equal(seen[0], seen[3])
    # and, unsplit, bit for bit the per-entry launches
    graph2 = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _routed(ops, q, k, v, heads, kb, vb, shots, route, table=table, mirror=mirror, out=out, key_split=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph2):
        _routed(ops, q, k, v, heads, kb, vb, shots, route, table=table, mirror=mirror, out=out, key_split=False)
    for rt in routes:
        table.copy_(_table(shots, rt))
        graph2.replay()
        assert torch.equal(out, _per_entry(ops, q, k, v, heads, kb, vb, shots, rt)), rt


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_routed_stack_at_the_end_of_its_allocation(ops, dtype):
    """The bank descriptor spans exactly nbank images: a stack that is the LAST bytes of its allocation, most entries
    routed to its last set, gives the unsplit per-entry result (a read past it would fault, an index past it would read
    zeros)."""
    from diffews_amd import _lib as L
    g = torch.Generator(device="cuda").manual_seed(48)
    shots, route, heads, N = (1, 3, 2), (2, 0, 2, 1, 2), 5, 1024
    C_, tot = heads * 64, sum(shots)
    q, k, v = _qkv(len(route), N, heads, dtype, g)
    big = torch.randn(3 * tot * N * 2 * C_, generator=g, device="cuda").to(dtype)
    kv = big[-tot * N * 2 * C_:].view(tot, N, 2 * C_)          # ends exactly where the allocation ends
    assert kv.data_ptr() + kv.numel() * kv.element_size() == big.data_ptr() + big.numel() * big.element_size()
    kb, vb = kv[..., :C_], kv[..., C_:]
    with routed_names(ops, L) as names:
        y = _routed(ops, q, k, v, heads, kb, vb, shots, route)
    assert names[0].endswith("+routed") and "+split" not in names[0], names       # short rows: the default plan is unsplit
    assert torch.equal(y, _per_entry(ops, q, k, v, heads, kb, vb, shots, route))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", RAGGED_CASES, ids=[c[0] for c in RAGGED_CASES])
def test_identity_route_is_the_ragged_launch(ops, case, dtype):
    """The identity route on a ragged stack, key_split=False, equals ops.fsa_attention_ragged with group = 1 exactly: the
    same two ints reach the same kernel body from another place."""
    cid, shots, b, heads, n_q, n_bank = case
    g = torch.Generator(device="cuda").manual_seed(49)
    q, k, v = _qkv(len(shots), n_q, heads, dtype, g)
    kb, vb = _bank(sum(shots), n_bank, heads, dtype, g)
    y = _routed(ops, q, k, v, heads, kb, vb, shots, tuple(range(len(shots))), key_split=False)
    ref = ops.fsa_attention_ragged(q, k, v, heads, kb, vb, shots, 1, q_prescaled=True, key_split=False)
    assert torch.equal(y, ref), (cid, rel(y, ref))


# ------------------------------------------------------------------------------------------------ pipeline

SHOTS, ROUTE, RES = (1, 3, 2), (2, 0, 2, 1), 64
B_Q = len(ROUTE)
FLAGS = [dict(), dict(batch_max=True), dict(r_threshold=0.0, threshold=0.3)]     # the three threshold modes
KEYS = ("z0", "dec", "seg_u8", "counts")


def _gt01(b, seed):
    g = torch.Generator().manual_seed(seed)
    gt = (torch.rand(b, RES, RES, generator=g) > 0.5).to(torch.uint8)
    gt[torch.rand(b, RES, RES, generator=g) < 0.05] = 255
    return gt


@pytest.mark.parametrize("library", ["ragged", "uniform"])
def test_segment_routed_vs_references(models, library):
    """segment_routed(bankset, qry, route).  Entry i against oracle.pipeline.pipeline_call with b = 1, query i and the
    supports of class route[i]: the bounds of test_segment_classes_ragged_vs_oracle (z0 < TOL_EP, mean |delta| of the decoded
    [0, 255] image < 1.0 fp16 / 4.0 bf16); against segment_queries(bankset.bank(route[i]), qry[i:i+1]) within 1.5 x TOL_EP.
    counts are the post-processing reference's on the engine's own seg_u8, exactly, in the three threshold modes."""
    from oracle import pipeline as op
    pipe, dt = models["pipe"], models["dt"]
    shots = SHOTS if library == "ragged" else (2, 2, 2)
    sup, msk = _classes(seed=900, shots=shots)
    qry = _queries(B_Q, RES, seed=910)
    gt = _gt01(B_Q, 7)
    if library == "ragged":
        bankset = pipe.prepare_support_classes(_cuda(sup), _cuda(msk))
    else:
        bankset = pipe.prepare_support_classes(torch.stack(sup).cuda(), torch.stack(msk).cuda())
    assert bankset.ragged == (library == "ragged") and bankset.shots == shots
    h, w = bankset.hw
    r = pipe.segment_routed(bankset, qry.cuda(), ROUTE, gt.cuda(), captured=False)
    assert set(r) == set(KEYS)
    assert r["z0"].shape == (B_Q, 4, h, w) and r["dec"].shape == (B_Q, 3, RES, RES)
    assert r["seg_u8"].shape == (B_Q, 3, RES, RES) and r["seg_u8"].dtype == torch.uint8 and r["counts"].shape == (B_Q, 4)
    for i, c in enumerate(ROUTE):
        _, ref = op.pipeline_call(models["ou"], models["ov"], [sup[c], qry[i:i + 1], msk[c]], models["te"])
        e_z0 = rel(r["z0"][i:i + 1], ref["z0"])
        d_seg = float(((r["dec"][i:i + 1].cpu() * 0.5 + 0.5) * 255 - ref["seg"]).abs().mean())
        one = pipe.segment_queries(bankset.bank(c), qry[i:i + 1].cuda(), captured=False)
        e_one = rel(r["z0"][i:i + 1], one["z0"])
        print(f"[routed] {library} entry {i} -> class {c} (s = {shots[c]}) {dt}: z0 vs oracle {e_z0:.3e}, decoded mean |d| "
              f"{d_seg:.3f}, z0 vs segment_queries {e_one:.3e}")
        assert e_z0 < TOL_EP[dt], e_z0
        assert d_seg < (1.0 if dt == torch.float16 else 4.0), d_seg
        assert e_one < 1.5 * TOL_EP[dt], e_one
    assert pipe.segment_routed(bankset, qry.cuda(), ROUTE, captured=False)["counts"] is None
    for flags in FLAGS:
        rf = pipe.segment_routed(bankset, qry.cuda(), ROUTE, gt.cuda(), captured=False, **flags)
        want = seg_counts_ref(rf["seg_u8"].cpu(), gt, flags.get("r_threshold", 0.25), flags.get("threshold", 0.0),
                              flags.get("batch_max", False))
        assert rf["counts"].cpu().tolist() == want, flags
        assert torch.equal(rf["z0"], r["z0"])
    # errors: a set outside the stack, a route that is not b long, a SupportBank
    for bad in ((2, 0, 3, 1), (2, 0, -1, 1), (2, 0, 2), (2, 0, 2, 1, 0), ()):
        with pytest.raises(ValueError):
            pipe.segment_routed(bankset, qry.cuda(), bad, captured=False)
    with pytest.raises(ValueError):
        pipe.segment_routed(bankset.bank(0), qry.cuda(), ROUTE, captured=False)


def test_segment_routed_captured_equals_eager(models):
    """captured=True replays the same kernels: identical bits on every output for three different routes of the same
    shape, through ONE graph (the route is not in the key; the table is a static input copied per call); each replay is its
    own route's eager result and two routes give different z0."""
    pipe = models["pipe"]
    pipe._graphs = {}
    sup, msk = _classes(seed=920)
    bankset = pipe.prepare_support_classes(_cuda(sup), _cuda(msk))
    gt = _gt01(B_Q, 9).cuda()
    routes = [ROUTE, (0, 1, 2, 0), (1, 1, 1, 2)]
    try:
        z0s = []
        for n, route in enumerate(routes + [ROUTE]):
            qry = _queries(B_Q, RES, 930 + n % 2).cuda()
            e = {k: v.clone() for k, v in pipe.segment_routed(bankset, qry, route, gt, captured=False).items()}
            c = pipe.segment_routed(bankset, qry, route, gt, captured=True)
            for k in KEYS:
                assert torch.equal(e[k], c[k]), (route, k)
            assert len(pipe._graphs) == 1, list(pipe._graphs)
            z0s.append(e["z0"])
        key = next(iter(pipe._graphs))
        assert key[:3] == ("queries", "routed", bankset.uid) and not any(x in (ROUTE, list(ROUTE)) for x in key)
        qry = _queries(B_Q, RES, 930).cuda()
        a = pipe.segment_routed(bankset, qry, routes[0], gt, captured=True)["z0"].clone()
        b_ = pipe.segment_routed(bankset, qry, routes[1], gt, captured=True)["z0"].clone()
        assert not torch.equal(a, b_) and torch.equal(a, z0s[0])
        # it is a query graph like the others: bounded together with them
        for i in range(pipe.MAX_QUERY_GRAPHS):
            pipe.segment_queries(bankset.bank(i % 3), _queries(1 + i, RES, 940).cuda(), captured=True)
        assert sum(1 for k in pipe._graphs if k[0] == "queries") == pipe.MAX_QUERY_GRAPHS
        assert not any(k[1] == "routed" for k in pipe._graphs)          # the least recently used went first
    finally:
        pipe._graphs = {}


def test_segment_routed_native(models):
    """segment_routed(..., native=t) with a class value per query: r["native"] equals tests/native_ref.py on the call's own
    seg_u8 exactly, eager and captured; every other entry is the call without it."""
    from diffews_amd.input_pipeline import NativeTargets
    pipe = models["pipe"]
    pipe._graphs = {}
    ids = [7, 3, 9]
    sup, msk = _classes(seed=950)
    bankset = pipe.prepare_support_classes(_cuda(sup), _cuda(msk))
    sizes = [(48, 64), (97, 131), (23, 37), (64, 64)]
    gts = _gts(sizes, "ids8", 71)
    cv = [ids[c] for c in ROUTE]
    t = NativeTargets((RES, RES), sizes, gt=gts, class_value=cv, ignore_value=255)
    qry = _queries(B_Q, RES, 951).cuda()
    try:
        for captured in (False, True):
            plain = {k: (None if v is None else v.clone())
                     for k, v in pipe.segment_routed(bankset, qry, ROUTE, captured=captured).items()}
            r = pipe.segment_routed(bankset, qry, ROUTE, captured=captured, native=t)
            assert set(r) == set(plain) | {"native"}
            for k in plain:
                assert (plain[k] is None and r[k] is None) or torch.equal(plain[k], r[k]), (captured, k)
            _check_native(r, sizes, gts, cv, 255, (0.25, 0.0, False))
    finally:
        pipe._graphs = {}


def _stream_setup(pipe, n, seed):
    import test_query_loader_gpu as ql
    from diffews_amd.input_pipeline import DeviceImageTransform
    tf = DeviceImageTransform(RES)
    ids = ql.CLASS_IDS
    qs = ql._host_queries(n, seed=seed)
    for i, q in enumerate(qs):
        q["cls"] = (2, 0, 2, 1, 1, 0, 2)[i % 7]
    simg, smap = ql._host_supports(ids, max(SHOTS), seed=8)
    simg = [ims[:s] for ims, s in zip(simg, SHOTS)]
    smap = [mps[:s] for mps, s in zip(smap, SHOTS)]
    sup = [torch.stack([tf.image(im) for im in ims]) for ims in simg]
    msk = [torch.stack([tf.mask(m, c - 1)[0] for m in mps]) for mps, c in zip(smap, ids)]
    return tf, ids, qs, pipe.prepare_support_classes(sup, msk)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_segment_stream_with_a_route(models, captured):
    """segment_stream(bankset, queries, route=...) over seven queries in batches of four (the last one short): per batch
    the dict of segment_routed on the hand-built batch with the ground-truth id class_ids[route_i] -- native counts and
    processing-size counts -- plus `route`; a key name and a callable route agree; route= with a SupportBank, and a route
    outside the set, raise ValueError."""
    from diffews_amd.input_pipeline import NativeTargets
    pipe = models["pipe"]
    pipe._graphs = {}
    try:
        tf, ids, qs, bankset = _stream_setup(pipe, 7, seed=53)
        got = []
        for index, r in pipe.segment_stream(bankset, qs, batch=4, size=RES, depth=1, class_ids=ids, ignore_value=255,
                                            captured=captured, route="cls"):
            assert set(r) == set(KEYS) | {"native", "route"}
            got.append((index, r["route"], r["native"]["counts"].clone(), r["counts"].clone(),
                        [p.clone() for p in r["native"]["pred"]]))
        assert [g[0] for g in got] == [[0, 1, 2, 3], [4, 5, 6]]
        assert [g[1] for g in got] == [[q["cls"] for q in qs[:4]], [q["cls"] for q in qs[4:]]]
        for index, route, ncounts, counts, pred in got:
            part = [qs[i] for i in index]
            qry = torch.stack([tf.image(q["query_img"]) for q in part])
            qm = torch.stack([tf.mask(q["gt"], ids[q["cls"]] - 1)[1] for q in part])
            t = NativeTargets((RES, RES), [q["gt"].shape for q in part], gt=[q["gt"] for q in part],
                              class_value=[ids[q["cls"]] for q in part], ignore_value=255)
            r = pipe.segment_routed(bankset, qry, route, qm, captured=captured, native=t)
            assert torch.equal(ncounts, r["native"]["counts"]) and torch.equal(counts, r["counts"]), index
            assert int(ncounts[:, 2:].sum()) > 0
            for x, y, q in zip(pred, r["native"]["pred"], part):
                assert x.shape == q["gt"].shape and torch.equal(x, y), index
        again = [(index, r["native"]["counts"].clone()) for index, r in
                 pipe.segment_stream(bankset, qs, batch=4, size=RES, depth=1, class_ids=ids, ignore_value=255,
                                     captured=captured, route=lambda q: q["cls"])]
        for (i0, _, n0, _, _), (i1, n1) in zip(got, again):
            assert i0 == i1 and torch.equal(n0, n1)
        with pytest.raises(ValueError):
            next(pipe.segment_stream(bankset.bank(0), qs, route="cls"))
        with pytest.raises(ValueError):
            next(pipe.segment_stream(bankset, qs, batch=4, size=RES, depth=1, route=lambda q: 3))
    finally:
        pipe._graphs = {}


def test_evaluate_routed_equals_the_hand_fed_meter(models):
    """evaluate_routed over seven queries whose class changes from one to the next == an AverageMeter fed by hand from
    per-query segment_queries(bankset.bank(c), one query) native counts under class_of_set[c]: equal integer buffers, equal
    scores.

    Integer counts can be EQUAL only between two evaluations that round alike, and this engine's GEMM / conv plans depend
    on the batch (which is why an entry of a batch of four is held to 1.5 x TOL_EP against segment_queries on one query,
    not to equality): so the equality with the per-query calls is asserted with evaluate_routed at batch = 1, where both
    sides run the same plans and the routed attention is bit for bit the shared-bank one.  At batch = 4 evaluate_routed is
    held, exactly, to the meter fed by hand from segment_routed on the same batches; its distance from the per-query meter
    is printed, not asserted (measured on an MI355X, fp16: row 0 of the intersection buffer at the three classes (35, 35, 38)
    against (36, 35, 37), both rows summed 6396 against 6395, mIoU 1.7074 against 1.7072 -- single pixels of the seven
    native-size masks on the other side of the threshold)."""
    from diffews_amd import evaluate
    from diffews_amd.input_pipeline import NativeTargets
    from diffews_amd.metrics import AverageMeter, fold_class_ids
    pipe = models["pipe"]
    pipe._graphs = {}
    try:
        tf, ids, qs, bankset = _stream_setup(pipe, 7, seed=57)
        class_of_set = [c - 1 for c in ids]                       # gt_ids default: class_of_set[c] + 1 (coco.py:74-75)
        dev = pipe.device
        cls_t = lambda cs: torch.tensor([class_of_set[c] for c in cs], dtype=torch.int64, device=dev)
        hand = AverageMeter("coco", fold_class_ids("coco", 0), device=dev)
        for q in qs:
            c = q["cls"]
            t = NativeTargets((RES, RES), [q["gt"].shape], gt=[q["gt"]], class_value=ids[c], ignore_value=255)
            r = pipe.segment_queries(bankset.bank(c), tf.image(q["query_img"])[None], None, captured=False, native=t)
            hand.update_from_counts(r["native"]["counts"], cls_t([c]))
        h_miou, h_fb, _ = hand.compute_iou()
        for captured in (False, True):
            miou, fb_iou, meter = evaluate.evaluate_routed(pipe, bankset, qs, class_of_set, route="cls", batch=1, size=RES,
                                                           depth=1, captured=captured, ignore_value=255)
            assert meter.intersection_buf.dtype == torch.int64 and int(meter.union_buf.sum()) > 0
            assert torch.equal(meter.intersection_buf, hand.intersection_buf), captured
            assert torch.equal(meter.union_buf, hand.union_buf), captured
            assert miou == float(h_miou) and fb_iou == float(h_fb) and miou > 0
        assert sum(1 for k in pipe._graphs if k[1] == "routed") == 1        # seven routes, one graph
        # batches of four (the last one short): the meter fed by hand from segment_routed on the same batches
        miou4, fb4, meter4 = evaluate.evaluate_routed(pipe, bankset, qs, class_of_set, route="cls", batch=4, size=RES,
                                                      depth=1, captured=False, ignore_value=255)
        hand4 = AverageMeter("coco", fold_class_ids("coco", 0), device=dev)
        for i in range(0, len(qs), 4):
            part = qs[i:i + 4]
            route = [q["cls"] for q in part]
            t = NativeTargets((RES, RES), [q["gt"].shape for q in part], gt=[q["gt"] for q in part],
                              class_value=[ids[c] for c in route], ignore_value=255)
            r = pipe.segment_routed(bankset, torch.stack([tf.image(q["query_img"]) for q in part]), route, captured=False,
                                    native=t)
            hand4.update_from_counts(r["native"]["counts"], cls_t(route))
        assert torch.equal(meter4.intersection_buf, hand4.intersection_buf) and torch.equal(meter4.union_buf, hand4.union_buf)
        m4, f4, _ = hand4.compute_iou()
        assert miou4 == float(m4) and fb4 == float(f4)
        seen = sorted(set(class_of_set))
        print(f"[routed] evaluate_routed {models['dt']}: batch 4 inter {meter4.intersection_buf[1, seen].tolist()} union "
              f"{meter4.union_buf[1, seen].tolist()} miou {miou4:.4f}; per-query inter {hand.intersection_buf[1, seen].tolist()} "
              f"union {hand.union_buf[1, seen].tolist()} miou {float(h_miou):.4f}")
        same = evaluate.evaluate_routed(pipe, bankset, qs, class_of_set, gt_ids=ids, route=lambda q: q["cls"], batch=4,
                                        size=RES, depth=1, captured=False, ignore_value=255)
        assert torch.equal(same[2].intersection_buf, meter4.intersection_buf) and same[0] == miou4
        with pytest.raises(ValueError):
            evaluate.evaluate_routed(pipe, bankset, qs, class_of_set[:2], route="cls", size=RES)
    finally:
        pipe._graphs = {}
