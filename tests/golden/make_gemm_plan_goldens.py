"""Generate tests/golden/gemm_plan_goldens.json: what the host-only plan queries of dfw_gemm (dfw_gemm_kernel_name,
dfw_gemm_gn_chunks, dfw_gemm_workspace_bytes) answer on a grid of dfw_gemm_args x dfw_config, recorded from the library
built at the commit named inside the file.  tests/test_gemm_plan_goldens_cpu.py re-enumerates the same grid (it imports
this module) against the library of the working tree: a change of the planner that is meant to keep every plan must
leave the file as it is.

    python tests/golden/make_gemm_plan_goldens.py          (needs the built library, no GPU: nothing is dereferenced)

A row is "name|gn_chunks|workspace_bytes" with the storage dtype written {T}, or "E<code>" for rejected arguments.
Two tiers keep the fixture small: the CORE table holds every value (the default config on the whole shape set, every
other config on a reduced set), the WIDE grid (every config on the whole set) is one SHA-256 per (op, config) block.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "gemm_plan_goldens.json")

# ---- dfw_config settings (tests/test_gemm_plans_gpu.py's GK / BIG / ANY and the sweeps' forced plans)
GK = dict(big_kernels=0, conv_patch=0)
BIG = dict(k8=0, conv_patch=0, big_min_tiles=1)
ANY = dict(big_min_tiles=1)
CONFIGS = {
    "default": {}, "GK": GK, "BIG": BIG, "ANY": ANY,
    **{f"big{m}x{n}x{k}": dict(BIG, big_bm=m, big_bn=n, big_bk=k)
       for m, n, k in ((256, 256, 32), (512, 128, 32), (256, 128, 64), (256, 128, 32))},
    **{f"gk{m}x{n}": dict(GK, gemm_bm=m, gemm_bn=n) for m, n in ((128, 128), (128, 64), (64, 64))},
    **{f"k8={v}": dict(k8=v) for v in (0, 1, 2, 3)},
    **{f"conv_patch={v}": dict(conv_patch=v) for v in (0, 1, 2, 4)},
}
PLAN_FIELDS = ("conv_patch", "big_kernels", "big_bm", "big_bn", "big_bk", "gemm_bm", "gemm_bn", "big_min_tiles", "k8")

# ---- shapes: (whole set, reduced set)
LIN_M = ((96, 257, 1024, 2048, 4097, 8192, 16384, 32768, 65536), (257, 4097, 32768))
LIN_N = ((64, 128, 160, 192, 256, 320, 512, 640, 960, 1280, 2560, 10240), (128, 320, 512, 960, 1280))
LIN_K = ((64, 128, 320, 640, 1280, 5120), (64, 1280))
LIN_VARIANTS = ("plain", "res", "rf32", "rf32_f32o", "geglu", "silu", "colscale", "splitk1", "splitk4", "view")
BMM = ((3, 300, 256, 128, False), (4, 100, 64, 192, True), (2, 4096, 4096, 512, False))     # Bt, M, N, K, fp32 output
CONV_B = ((1, 4, 12), (4,))
CONV_HW = (((8, 8), (16, 16), (13, 19), (32, 32), (32, 48), (64, 64), (128, 128), (256, 256), (512, 512)),
           ((13, 19), (32, 48), (64, 64), (128, 128)))
CONV_CIN = ((64, 128, 320, 512, 1280), (64, 320))
CONV_COUT = ((64, 128, 256, 320, 512, 640, 1280), (128, 256, 320))
CONV_GEOM = ((1, 1, 0), (2, 1, 0), (2, 0, 0), (1, 1, 1))       # stride, pad, ups
CONV_VARIANTS = ("T", "T_gn", "f32o", "f32o_gn", "nchw", "silu", "splitk2")
OPS = ("linear", "bmm", "conv")

# fake device pointers, 256-byte aligned; the queries read no memory
P_A, P_W, P_C, P_BIAS, P_RES = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000


def rows(op, tier):
    """The argument rows of one op, in the order the goldens store them: tuples the test can print."""
    t = 0 if tier == "whole" else 1
    if op == "linear":
        return [("linear", M, N, K, v) for M in LIN_M[t] for N in LIN_N[t] for K in LIN_K[t] for v in LIN_VARIANTS]
    if op == "bmm":
        return [("bmm",) + s for s in BMM]
    return [("conv", B, H, W, Cin, Cout, g, v) for B in CONV_B[t] for H, W in CONV_HW[t] for Cin in CONV_CIN[t]
            for Cout in CONV_COUT[t] for g in CONV_GEOM for v in CONV_VARIANTS]


def fill(L, a, row, dtype):
    """dfw_gemm_args of a row, built as diffews_amd.ops builds them (linear / bmm_nt / conv3x3)."""
    C.memset(C.byref(a), 0, C.sizeof(a))
    a.A, a.W, a.C, a.bias, a.dtype, a.batch, a.out_scale = P_A, P_W, P_C, P_BIAS, dtype, 1, 1.0
    if row[0] == "linear":
        _, M, N, K, v = row
        a.M, a.N, a.K, a.lda, a.ldc, a.taps, a.Cin = M, N, K, K, N, 1, K
        a.a_elems, a.w_elems = M * K, N * K
        if v in ("res", "rf32", "rf32_f32o"):
            a.residual, a.ldr, a.residual_f32 = P_RES, N, int(v != "res")
        if v == "rf32_f32o":
            a.out_mode = L.OUT_F32
        elif v == "geglu":
            a.geglu, a.ldc = 1, N // 2
        elif v == "silu":
            a.act = L.ACT_SILU
        elif v == "colscale":
            a.colscale, a.colscale_n = 0.5, 64
        elif v in ("splitk1", "splitk4"):
            a.splitk = int(v[-1])
        elif v == "view":           # out = wide[:, 4:4 + N]: C eight bytes past a 16-byte boundary, ldc % 8 == 4
            a.C, a.ldc = P_C + 8, N + 12
    elif row[0] == "bmm":
        _, Bt, M, N, K, f32 = row
        a.M, a.N, a.K, a.lda, a.ldc, a.taps, a.Cin = M, N, K, K, N, 1, K
        a.a_elems, a.w_elems, a.bias = M * K, N * K, None
        a.out_mode, a.splitk, a.batch = (L.OUT_F32 if f32 else L.OUT_T), 1, Bt
        a.strideA, a.strideW, a.strideC = M * K, N * K, M * N
    else:
        _, B, Hi, Wi, Cin, Cout, (stride, pad, ups), v = row
        if ups:
            Ho, Wo = 2 * Hi, 2 * Wi
        elif stride == 1:
            Ho, Wo = Hi, Wi
        else:
            Ho, Wo = ((Hi + 2 * pad - 3) // stride + 1, (Wi + 2 * pad - 3) // stride + 1) if pad else (Hi // 2, Wi // 2)
        M = B * Ho * Wo
        a.M, a.N, a.K, a.lda, a.ldc = M, Cout, 9 * Cin, Cin, Cout
        a.a_elems, a.w_elems = B * Hi * Wi * Cin, Cout * 9 * Cin
        a.taps, a.Cin, a.Hi, a.Wi, a.Ho, a.Wo = 9, Cin, Hi, Wi, Ho, Wo
        a.stride, a.pad, a.ups, a.rows_per_img = stride, pad, ups, Ho * Wo
        if v.startswith("f32o"):
            a.out_mode, a.residual, a.ldr, a.residual_f32 = L.OUT_F32, P_RES, Cout, 1
        elif v == "nchw":
            a.out_mode = L.OUT_NCHW_F32
        elif v == "silu":
            a.act = L.ACT_SILU
        elif v == "splitk2":
            a.splitk = 2
        if v.endswith("_gn"):
            a.gn_groups = 32


def plan_values(L, lib, op, tier, dtype=None, buffers=False):
    """One value per row of rows(op, tier) under the config in effect.  buffers: also pass the workspace and the
    partial-sum buffer, which the queries run before and the launch runs with."""
    dtype = L.BF16 if dtype is None else dtype
    tname = "bf16" if dtype == L.BF16 else "f16"
    a, buf = L.GemmArgs(), C.create_string_buffer(96)
    ref = C.byref(a)
    out = []
    for row in rows(op, tier):
        fill(L, a, row, dtype)
        if buffers:
            a.workspace, a.workspace_bytes, a.gn_partial = 0x60000000, 1 << 40, 0x70000000
        rc = lib.dfw_gemm_kernel_name(ref, buf, 96)
        if rc:
            assert lib.dfw_gemm_gn_chunks(ref) == 0 and lib.dfw_gemm_workspace_bytes(ref) == 0, row
            out.append(f"E{rc}")
            continue
        name = buf.value.decode().replace("<" + tname + ",", "<{T},", 1)
        out.append(f"{name}|{lib.dfw_gemm_gn_chunks(ref)}|{lib.dfw_gemm_workspace_bytes(ref)}")
    return out


def configured(L, cfg):
    L.configure()
    return L.configure(**cfg) if cfg else L.configure()


def block_hash(values):
    return hashlib.sha256("\n".join(values).encode()).hexdigest()


def instantiations(row, value):
    """Keys of tests/test_gemm_plans_cpu.py::FORWARD_INSTANTIATIONS a planned row launches."""
    name, _, ws = value.split("|")
    base, plus, _ = name.partition("+")
    base = base.replace("{T}", "T")
    v = row[-1] if row[0] != "bmm" else ""
    rf32 = v in ("rf32", "rf32_f32o") or str(v).startswith("f32o")
    f32o = v == "rf32_f32o" or str(v).startswith("f32o") or (row[0] == "bmm" and row[-1])
    if base.startswith("gemm_kernel") and rf32 and not plus:
        base = base[:-1] + ",RF32>"
    if base.startswith(("gemm_big_kernel", "conv_patch_kernel")) and f32o:
        base = base[:-1] + ",F32O>"
    assert bool(plus) == (int(ws) > 0), (row, value)
    return {base} | ({"splitk_reduce_kernel<T>"} if plus else set())


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from diffews_amd import _lib as L, build
    from test_gemm_plans_cpu import FORWARD_INSTANTIATIONS
    build.build()
    lib = L.lib()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "diffews_amd/csrc", "include"],
                           capture_output=True, text=True, check=True).stdout.strip()
    assert not dirty, "the library sources differ from the commit:\n" + dirty
    defaults = configured(L, {})
    table, index, core, wide = [], {}, {}, {}
    total = rejected = chunked = with_ws = 0
    reached, names, nondefault = set(), set(), set()
    for cname, cfg in CONFIGS.items():
        now = configured(L, cfg)
        nondefault |= {k for k in PLAN_FIELDS if now[k] != defaults[k]}
        for op in OPS:
            values = plan_values(L, lib, op, "whole")
            wide[f"{op}/{cname}"] = block_hash(values)
            for row, v in zip(rows(op, "whole"), values):
                total += 1
                if v[0] == "E":
                    rejected += 1
                    names.add(v)
                    continue
                reached |= instantiations(row, v)
                names.add(v.split("|")[0])
                chunked += int(v.split("|")[1]) > 0
                with_ws += int(v.split("|")[2]) > 0
            if cname != "default":
                values = plan_values(L, lib, op, "reduced")
            core[f"{op}/{cname}"] = " ".join(str(index.setdefault(v, len(index))) for v in values)
    configured(L, {})
    # the plan ignores the storage dtype: fp16 on the reduced set gives the bf16 rows
    for op in OPS:
        assert plan_values(L, lib, op, "reduced", L.F16) == plan_values(L, lib, op, "reduced", L.BF16), op
    table = sorted(index, key=index.get)
    want = set(FORWARD_INSTANTIATIONS)
    assert reached == want, (want - reached, reached - want)
    assert nondefault == set(PLAN_FIELDS), set(PLAN_FIELDS) - nondefault
    assert rejected <= 0.05 * total, (rejected, total)
    assert chunked >= 1000, chunked
    core_rows = sum(len(v.split()) for v in core.values())
    doc = dict(commit=commit, rows=total, core_rows=core_rows, rejected=rejected, gn_rows=chunked, workspace_rows=with_ws,
               names=sorted(names), values=table, core=core, wide=wide)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    size = os.path.getsize(OUT)
    assert size < 256 * 1024, size
    print(f"{total} rows, {len(names)} names, {rejected} rejected ({100.0 * rejected / total:.1f} %), {chunked} with chunks, "
          f"{with_ws} with a workspace; core {core_rows} rows, {len(table)} distinct values, {size} bytes -> {OUT}")


if __name__ == "__main__":
    main()
