"""The instance split without a GPU: the definition of the nearest seed inside the object against the two-pass form the
kernels use (tests/split_ref.py), the worked examples, what the definition promises (the opening is covered, labels never
change across passes), that the case tables of the GPU tests reach what they claim, and the C ABI of the two calls that
carry it, both on dfw_seg_components -- the fields appended to dfw_seg_components_args (dfw_seg_boundary_args is what it
was), the new workspace query, every new refusal in its documented order on host memory with a null stream, and the
overlap matrix for seeds, nearest and keys."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import components_ref as cr
import edt_ref as er
import split_ref as sr
import test_object_boundaries_cpu as tb
from seg_args_cases import check_overlap_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFW_EINVAL, DFW_ESHAPE, DFW_ERANGE, DFW_EWORKSPACE = -1, -2, -3, -4


# ------------------------------------------------------------------------------------------------ the definition

def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_search_and_two_pass_form_agree_on_random_maps():
    rs = np.random.RandomState(0)
    for t in range(60):
        H, W = rs.randint(1, 13), rs.randint(1, 15)
        m = (rs.rand(H, W) < 0.8) * rs.randint(1, 3, (H, W))
        s = (rs.rand(H, W) < (0.04, 0.15, 0.5)[t % 3]) * rs.randint(-3, 4, (H, W))
        for R in (1, 2, 3, 6, 20):
            assert _same(sr.nearest_search(m, s, R), sr.nearest_two_pass(m, s, R)), (t, R)


def test_search_and_two_pass_form_agree_on_the_named_shapes_and_the_family():
    for name, (m, s, R) in sr.named_cases().items():
        for r in {1, 2, R}:
            assert _same(sr.nearest_search(m, s, r), sr.nearest_two_pass(m, s, r)), (name, r)
    lab = sr.family(sr.FAMILY_SEEDS[0], 40, 52)
    o = cr.components(lab[None], 8, 0, 64)
    seeds = np.where(er.dist2_ref(o["ids"], 2) > 4, o["ids"], 0)[0]
    assert _same(sr.nearest_search(o["ids"][0], seeds, 5), sr.nearest_two_pass(o["ids"][0], seeds, 5))


def test_the_named_shapes_say_what_their_names_say():
    c = sr.named_cases()
    near = {k: sr.nearest_ref(m, s, R) for k, (m, s, R) in c.items()}
    n, d = near["a tie left and right in a row: the smaller value"]
    assert n[0].tolist() == [7, 7, 7, 7, 3, 3, 3, 3, 3] and d[0].tolist() == [4, 1, 0, 1, 4, 1, 0, 1, 4]
    n, d = near["a tie up and down in a column"]
    assert n[:, 0].tolist() == [7, 7, 7, 7, 3, 3, 3, 3, 3]
    n, d = near["equal distances, different values"]
    assert n[3, 3] == 2 and d[3, 3] == 9                                   # four seeds 3 away, the smallest value
    n, d = near["a seed behind a gap of another value"]
    assert n[1].tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 5] and d[1, 3] == 81   # row 1 left of the gap: not a candidate
    assert n[0, 1] == 0 and n[0, 7] == 5 and n[0, 5] == 5                  # row 0 goes down column 5 and along
    n, d = near["a seed of another object in the same row"]
    assert not n[:, :6].any() and (n[:, 6:] == 6).all()
    n, d = near["seed values 2^31 - 1 and negative"]
    assert n[0, 0] == (1 << 31) - 1 and n[4, 4] == -(1 << 31) and n[0, 4] == -1 and n[2, 2] == -(1 << 31)
    n, d = near["a seed on background"]
    assert (n[1:5, 1:4] == 1).all() and n[0, 0] == 0 and d[0, 0] == 0
    m, s, R = c["a comb seeded at the tip of its first tooth"]
    one, two = sr.nearest_ref(m, s, R, 1)[0], sr.nearest_ref(m, s, R, 2)[0]
    assert (one[1:11, 1] == 3).all() and not one[:, 2:].any()              # the seeded tooth alone: the spine is row-first
    assert np.array_equal(two != 0, m != 0)                                # ... the spine and every other tooth with pass 2
    m, s, R = c["a U seeded at the top of its left arm"]
    one, two, three = (sr.nearest_ref(m, s, R, p)[0] for p in (1, 2, 3))
    assert (one[1:11, 1] == 8).all() and not one[:, 2:].any()               # the left arm alone
    assert np.array_equal(two != 0, m != 0) and np.array_equal(two, three)   # the far arm only with pass 2


def test_worked_example_of_the_header():
    m = np.array([[5, 5, 5, 5], [5, 0, 0, 5]], np.int32)
    s = np.array([[0, 0, 0, 0], [9, 0, 0, 3]], np.int32)
    for one in (sr.nearest_search, sr.nearest_two_pass):
        n, d = sr.nearest_ref(m, s, 3, 1, one)
        assert n.tolist() == [[9, 0, 0, 3], [9, 0, 0, 3]] and d.tolist() == [[1, 16, 16, 1], [0, 0, 0, 0]]
        n, d = sr.nearest_ref(m, s, 3, 2, one)
        assert n.tolist() == [[9, 9, 3, 3], [9, 0, 0, 3]] and d.tolist() == [[1, 1, 1, 1], [0, 0, 0, 0]]


def _two_discs():
    yy, xx = np.mgrid[:64, :64]
    return (((yy - 32) ** 2 + (xx - 20) ** 2 <= 196) | ((yy - 32) ** 2 + (xx - 42) ** 2 <= 196)).astype(np.uint8)


def _squares_and_bridge():
    lab = np.zeros((14, 26), np.uint8)
    lab[2:12, 1:11] = lab[2:12, 15:25] = 1
    lab[6:8, 11:15] = 1
    return lab


def test_two_discs():
    lab = _two_discs()
    o = cr.components(lab[None], 8, 0, 16)
    r = sr.split_ref(o["ids"], o["filtered"], 10, 22, 1, cap=16)
    assert o["n"][0, 0] == 1 and r["cores"][0, 0] == 2 and r["n"][0].tolist() == [2, 2]
    assert r["stats"][0, :3, 1].tolist() == [586, 569, 0] and not (r["nearest"][0] == 0)[lab != 0].any()
    assert r["parent"][0, :3].tolist() == [1, 1, 0]


def test_two_squares_and_a_bridge():
    lab = _squares_and_bridge()
    o = cr.components(lab[None], 8, 0, 16)
    r = sr.split_ref(o["ids"], o["filtered"], 3, 8, 1, cap=16)
    assert r["n"][0].tolist() == [2, 2] and r["stats"][0, :2, 1].tolist() == [104, 104]
    assert r["ids"][0, 6:8, 11:15].tolist() == [[1, 1, 2, 2], [1, 1, 2, 2]]  # the bridge is cut down its middle


def test_the_opening_is_covered_in_one_pass():
    """With reach >= radius every pixel within radius^2 of a core pixel lies in the object and receives a label."""
    rs = np.random.RandomState(5)
    for t in range(18):
        H, W, radius = 30, 34, (1, 2, 3)[t % 3]
        lab = ((np.kron(rs.rand(6, 7), np.ones((5, 5))) + 0.3 * rs.rand(H, W + 1)) > 0.55).astype(np.uint8)[:H, :W]
        o = cr.components(lab[None], 8, 0, 256)
        ids = o["ids"][0]
        core = np.where(er.dist2_ref(ids, radius).astype(np.int64) > radius * radius, ids, 0)
        near, _ = sr.nearest_ref(ids, core, radius + t % 2, 1)
        ys, xs = np.nonzero(core)
        opened = np.zeros((H, W), bool)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if dy * dy + dx * dx <= radius * radius:
                    opened[ys + dy, xs + dx] = True                        # inside the image: dist2 > radius^2 at the core
        assert core.any() and (ids[opened] != 0).all() and (near[opened] != 0).all(), t
        assert np.array_equal(near[opened], ids[opened])                   # ... and it is the own object's core, as ids here


def test_labels_never_change_across_passes():
    for seed in sr.FAMILY_SEEDS:
        lab = sr.family(seed)
        o = cr.components(lab[None], 8, 0, 256)
        r = sr.split_ref(o["ids"], o["filtered"], cap=256, **sr.FAMILY)
        trace = []
        sr.nearest_image(o["ids"][0], r["core_ids"][0], sr.FAMILY["reach"], 5, trace=trace)
        for a, b in zip(trace, trace[1:]):
            assert np.array_equal(b[a != 0], a[a != 0]) and (b != 0).sum() >= (a != 0).sum()
        assert (trace[1] != 0).sum() > (trace[0] != 0).sum()


@pytest.mark.parametrize("seed", sr.FAMILY_SEEDS)
def test_the_family_reaches_what_it_claims(seed):
    F = sr.FAMILY
    lab = sr.family(seed)
    o = cr.components(lab[None], F["connectivity"], 0, 256)
    r = sr.split_ref(o["ids"], o["filtered"], cap=256, **F)
    ids, core = o["ids"][0], r["core_ids"][0]
    ncores = [len(set(np.unique(core[ids == k]).tolist()) - {0}) for k in range(1, int(o["n"][0, 0]) + 1)]
    assert sum(c >= 2 for c in ncores) >= 1, "no object is split in two or more"
    assert sum(c == 0 for c in ncores) >= 1, "no coreless object"
    near = [sr.nearest_ref(ids, core, F["reach"], p)[0] for p in (1, 2, F["passes"])]
    assert ((near[0] == 0) & (near[1] != 0)).any(), "no pixel that only pass 2 reaches"
    cored = np.isin(ids, [k + 1 for k, c in enumerate(ncores) if c > 0])
    assert (cored & (near[2] == 0)).any(), "no pixel left unassigned after the last pass"
    assert int(r["n"][0, 0]) > int(o["n"][0, 0]) and int(r["n"][0, 0]) <= 256


def test_keyed_components_of_the_reference():
    lab = np.array([[1, 1, 1, 0], [1, 1, 2, 2], [0, 1, 2, 2]], np.uint8)
    keys = np.array([[5, 5, 7, 0], [5, 7, 7, 7], [0, 5, 7, -1]], np.int32)
    r8 = sr.components_keyed(lab[None], keys[None], 8, cap=8)
    assert r8["ids"][0].tolist() == [[1, 1, 2, 0], [1, 2, 3, 3], [0, 1, 3, 4]] and r8["n"][0].tolist() == [4, 4]
    assert r8["stats"][0, :4, :2].tolist() == [[1, 4], [1, 2], [2, 3], [2, 1]]
    r4 = sr.components_keyed(lab[None], keys[None], 4, cap=8)
    assert r4["ids"][0].tolist() == [[1, 1, 2, 0], [1, 3, 4, 4], [0, 5, 4, 6]]
    same = sr.components_keyed(lab[None], np.full((1, 3, 4), -9), 8, cap=8)
    plain = cr.components(lab[None], 8, 0, 8)
    assert all(np.array_equal(same[k], plain[k]) for k in ("ids", "filtered", "n", "stats"))
    rs = np.random.RandomState(3)
    lab = rs.randint(0, 3, (2, 9, 11)).astype(np.uint8)
    keys = rs.randint(-1, 2, (2, 9, 11))
    code = np.where(lab != 0, lab * 3 + keys + 1, 0).astype(np.uint8)      # one byte per pair: the keyless reference on it
    for conn in (4, 8):
        a, b = sr.components_keyed(lab, keys, conn, min_area=2, cap=16), cr.components(code, conn, 2, 16)
        assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["n"], b["n"])
        assert np.array_equal(a["stats"][..., 1:], b["stats"][..., 1:]) and np.array_equal(a["filtered"], np.where(b["filtered"] != 0, lab, 0))


# ------------------------------------------------------------------------------------------------ the C ABI

def test_struct_mirrors_sizeof_offsetof_version_and_query(hip_lib, tmp_path):
    from diffews_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "diffews_hip.h")).read()
    bf, cf = tb._fields(hdr, "dfw_seg_boundary_args"), tb._fields(hdr, "dfw_seg_components_args")
    assert bf[-3:] == ["metric", "peaks", "cap"] and bf == [f[0] for f in L.SegBoundaryArgs._fields_]   # as it was
    new = ["keys", "map", "seeds", "nearest", "dist", "reach", "passes"]
    assert cf[-7:] == new and cf == [f[0] for f in L.SegComponentsArgs._fields_]
    A, Cm = L.SegBoundaryArgs, L.SegComponentsArgs
    names = {A: "dfw_seg_boundary_args", Cm: "dfw_seg_components_args"}
    fields = [("map", A), ("ws_bytes", A), ("d", A), ("metric", A), ("peaks", A), ("cap", A), ("labels", Cm), ("ws_bytes", Cm),
              ("B", Cm), ("nlabels", Cm)] + [(f, Cm) for f in new]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "diffews_hip.h"\nint main(){printf("%zu %zu", '
                   'sizeof(dfw_seg_boundary_args), sizeof(dfw_seg_components_args));\n'
                   + "".join(f'printf(" %zu", offsetof({names[s]}, {f}));\n' for f, s in fields) + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(A), C.sizeof(Cm)] + [getattr(s, f).offset for f, s in fields]
    assert Cm.keys.offset == Cm.nlabels.offset + 8 and C.sizeof(A) == A.cap.offset + 8       # appended behind the padding
    assert L.SYMBOLS["dfw_seg_nearest_workspace_bytes"] == (C.c_size_t, [C.c_int32] * 3)
    assert hip_lib.dfw_version() >= 125


def test_the_new_query_is_monotone_and_zero_for_refused_sizes(hip_lib):
    q = hip_lib.dfw_seg_nearest_workspace_bytes
    sizes = [1, 2, 5, 15, 16, 17, 64, 65, 2048, 4096]
    for B in (1, 2, 3, 7):
        for H in sizes:
            for W in sizes:
                got, n = q(B, H, W), B * H * W
                assert 5 * n <= got <= 5 * n + 30 and got % 16 == 0, (B, H, W)
                assert q(B + 1, H, W) >= got and q(B, H + 1, W) >= got and q(B, H, W + 1) >= got
    assert q(1, 32768, 32768) == 5 << 30                                   # no 32-bit arithmetic on the way
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, -2), (65536, 1, 1), (1, 65536, 1), (1, 1, 65536), (1, 65535, 32768)):
        assert q(*bad) == 0, bad
    old = hip_lib.dfw_seg_boundary_workspace_bytes                         # the other query is what it was
    assert old(2, 17, 65, 4) == (2 * 17 * 65 + 15) // 16 * 16


B_, H_, W_ = 2, 5, 7


def _valid_seeds(lib, passes=2, reach=3):
    """A fully valid nearest-seed call (dfw_seg_components with seeds) on host memory (never launched: every test breaks one
    thing).  labels, ids, n and keys stay null: the stage does not look at them."""
    from diffews_amd import _lib as L
    ws_bytes = lib.dfw_seg_nearest_workspace_bytes(B_, H_, W_)
    assert 0 < ws_bytes < lib.dfw_seg_components_workspace_bytes(B_, H_, W_)
    keep = dict(map=np.zeros((B_, H_, W_), np.int32), dist=np.zeros((B_, H_, W_ + 1), np.uint16), seeds=np.zeros((B_, H_, W_), np.int32),
                nearest=np.zeros((B_, H_, W_), np.int32), ws=np.zeros(ws_bytes // 8 + 2, np.int64))
    a = L.SegComponentsArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.ws_bytes, a.B, a.H, a.W, a.reach, a.passes = ws_bytes, B_, H_, W_, reach, passes
    return a, keep


def test_every_refusal_of_a_seeded_call_comes_from_the_host(hip_lib):
    kept = []
    call = lambda a: hip_lib.dfw_seg_components(C.byref(a), None)  # noqa: E731

    def broken(**kw):
        a, keep = _valid_seeds(hip_lib)
        kept.append(keep)
        for k, v in kw.items():
            setattr(a, k, v)
        return call(a)

    # DFW_EINVAL: null pointers, then the scalars
    for field in ("map", "nearest", "dist", "ws"):
        assert broken(**{field: None}) == DFW_EINVAL, field
    for v in (0, -1, 255, 1000):
        assert broken(reach=v) == DFW_EINVAL, v
    for v in (0, -1, 9, 1 << 20):
        assert broken(passes=v) == DFW_EINVAL, v
    for v in range(1, 9):
        assert broken(passes=v, ws_bytes=0) == DFW_EWORKSPACE, v           # 1..8 pass the scalars
    for v in (1, 254):
        assert broken(reach=v, ws_bytes=0) == DFW_EWORKSPACE, v
    for field in ("B", "H", "W"):
        for v in (0, -1):
            assert broken(**{field: v}) == DFW_EINVAL, field
    # without seeds the call is the components call: null labels; and with them, nearest without seeds
    assert broken(seeds=None) == DFW_EINVAL
    import test_components_cpu as tc
    a, keep = tc._valid(hip_lib)
    a.nearest = keep["ids"].ctypes.data
    assert call(a) == DFW_EINVAL
    a.H = 65536                                                            # ... before the sizes
    assert call(a) == DFW_EINVAL
    a, keep = tc._valid(hip_lib)
    a.map, a.dist, a.reach, a.passes, a.ws_bytes = keep["ids"].ctypes.data, keep["ids"].ctypes.data, 999, 77, 0
    assert call(a) == DFW_EWORKSPACE                                       # not looked at without seeds
    # the order: scalars before the sizes, the sizes before the workspace
    assert broken(passes=0, H=65536) == DFW_EINVAL
    assert broken(nearest=None, B=65536) == DFW_EINVAL
    assert broken(H=65536) == DFW_ERANGE and broken(B=65536) == DFW_ERANGE and broken(H=65535, W=32768) == DFW_ERANGE
    assert broken(H=65536, ws_bytes=0) == DFW_ERANGE
    # DFW_EWORKSPACE against the new query
    a, keep = _valid_seeds(hip_lib)
    a.ws_bytes -= 1
    assert call(a) == DFW_EWORKSPACE
    assert broken(B=3) == DFW_EWORKSPACE
    # DFW_ESHAPE: map, seeds and nearest aligned to 4, dist to 2
    for field, shifts in (("map", (1, 2)), ("seeds", (1, 2)), ("nearest", (1, 2)), ("dist", (1,))):
        for shift in shifts:
            a, keep = _valid_seeds(hip_lib)
            setattr(a, field, getattr(a, field) + shift)
            assert call(a) == DFW_ESHAPE, (field, shift)
    # the overlap matrix: nearest may share no byte with map, seeds, dist or ws; map and seeds may alias each other
    n = B_ * H_ * W_
    check_overlap_rule(call, lambda: _valid_seeds(hip_lib), dict(map=(4 * n, 4), seeds=(4 * n, 4)),
                       dict(dist=(2 * n, 2), ws=(hip_lib.dfw_seg_nearest_workspace_bytes(B_, H_, W_), 4), nearest=(4 * n, 4)))
    a, keep = _valid_seeds(hip_lib)
    a.seeds, a.ws_bytes = a.map, a.ws_bytes - 1                            # two inputs on each other: as far as the workspace
    assert call(a) == DFW_EWORKSPACE


def test_with_the_new_fields_zero_the_old_refusals_come_in_the_old_order(hip_lib):
    import test_object_thickness_cpu as tt
    import test_components_cpu as tc
    tt.test_struct_mirrors_sizeof_offsetof_and_version(hip_lib, __import__("pathlib").Path(__import__("tempfile").mkdtemp()))
    tt.test_every_refusal_of_a_euclidean_call_comes_from_the_host(hip_lib)
    tb.test_every_refusal_of_seg_boundary_comes_from_the_host(hip_lib)
    a, keep = tc._valid(hip_lib)
    assert not a.keys and not a.seeds and not a.nearest and a.passes == 0
    tc.test_every_refusal_comes_from_the_host_before_any_launch(hip_lib)
    tc.test_workspace_query_is_monotone_and_bounded(hip_lib)


def _valid_keyed(lib):
    import test_components_cpu as tc
    a, keep = tc._valid(lib)
    keep["keys"] = np.zeros((2, 5, 7), np.int32)
    a.keys = keep["keys"].ctypes.data
    return a, keep


def test_every_refusal_of_a_keyed_call_comes_from_the_host(hip_lib):
    call = lambda a: hip_lib.dfw_seg_components(C.byref(a), None)  # noqa: E731

    def broken(**kw):
        a, keep = _valid_keyed(hip_lib)
        for k, v in kw.items():
            setattr(a, k, v)
        return call(a)

    for field in ("labels", "ids", "n", "ws"):
        assert broken(**{field: None}) == DFW_EINVAL, field
    assert broken(connectivity=6) == DFW_EINVAL and broken(min_area=-1) == DFW_EINVAL and broken(H=65536) == DFW_ERANGE
    assert broken(ws_bytes=0) == DFW_EWORKSPACE
    for shift in (1, 2):
        a, keep = _valid_keyed(hip_lib)
        a.keys += shift
        assert call(a) == DFW_ESHAPE, shift
    a, keep = _valid_keyed(hip_lib)
    a.keys, a.ws_bytes = a.ids, 0                                          # the workspace before the overlap
    assert call(a) == DFW_EWORKSPACE
    px, ws = 2 * 5 * 7, hip_lib.dfw_seg_components_workspace_bytes(2, 5, 7)
    check_overlap_rule(call, lambda: _valid_keyed(hip_lib), dict(labels=(px, 1), gt=(px, 1), keys=(4 * px, 4)),
                       dict(ids=(4 * px, 4), n=(2 * 8, 4), filtered=(px, 1), stats=(2 * 4 * 32, 4), counts=(2 * 2 * 4 * 8, 8),
                            ws=(ws, 4)))


# ------------------------------------------------------------------------------------------------ the objects layer

def test_the_objects_layer_checks_its_arguments(hip_lib):
    from diffews_amd import objects
    z = torch.zeros(4, 4, dtype=torch.int32)
    o = dict(ids=z, labels=z.to(torch.uint8), stats=torch.zeros(3, 8, dtype=torch.int32), n=torch.zeros(2, dtype=torch.int32))
    for radius in (-1, 255, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="radius"):
            objects.split_objects(o, radius)
    for bad in (z, {"ids": z}, None):
        with pytest.raises(ValueError):
            objects.split_objects(bad, 1)
    with pytest.raises(ValueError):
        objects.split_objects(o, 1)                                        # host tensors
    with pytest.raises(ValueError):
        objects.nearest_seeds(z, z, 3)                                     # host tensors
    with pytest.raises(ValueError, match="one seed map per id map"):
        objects.nearest_seeds([z], [z, z], 3)
    with pytest.raises(ValueError, match="max_components"):
        objects.SplitBuffers(1, 4, 4, 0, device="cpu")
    b = objects.SplitBuffers(2, 8, 9, 5, device="cpu")
    assert b.nearest.shape == (2, 8, 9) and b.nearest.dtype == torch.int32 and b.dist.dtype == torch.uint16
    assert b.parent.shape == (2, 5) and b.ws.numel() == hip_lib.dfw_seg_nearest_workspace_bytes(2, 8, 9)
    assert b.thick.peaks.shape == (2, 5) and b.seeds.stats.shape == (2, 5, 8) and b.out.ids.shape == (2, 8, 9)
    import inspect
    sig = inspect.signature(objects.split_objects).parameters
    assert sig["reach"].default is None and sig["passes"].default == 3 and sig["min_area"].default == 0
    assert inspect.signature(objects.label_objects).parameters["keys"].default is None
    assert inspect.signature(objects.nearest_seeds).parameters["passes"].default == 1


def test_ops_split_allocates_nothing():
    import test_launch_guard_cpu as scan
    assert not scan._allocating_functions(os.path.join(ROOT, "diffews_amd", "ops_split.py"))
