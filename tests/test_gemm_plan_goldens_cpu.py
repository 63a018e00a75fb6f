"""CPU test (no GPU): the plan of dfw_gemm -- kernel, tile, split-K workspace and GroupNorm chunk count, read through the
host-only queries -- on the grid of tests/golden/make_gemm_plan_goldens.py equals what the library answered at the
commit recorded in tests/golden/gemm_plan_goldens.json.  CORE rows are compared value by value, the WIDE grid (every
config on the whole shape set) by one SHA-256 per (op, config) block."""
import importlib.util
import json
import os

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_gemm_plan_goldens", os.path.join(GOLD, "make_gemm_plan_goldens.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "gemm_plan_goldens.json")) as f:
        return json.load(f)


def test_fixture_is_small_and_covers_every_block(gold):
    assert os.path.getsize(os.path.join(GOLD, "gemm_plan_goldens.json")) < 256 * 1024
    blocks = {f"{op}/{c}" for c in gen.CONFIGS for op in gen.OPS}
    assert set(gold["core"]) == blocks and set(gold["wide"]) == blocks
    assert len(gold["commit"]) == 40 and gold["rejected"] <= 0.05 * gold["rows"] and gold["gn_rows"] >= 1000


@pytest.mark.parametrize("cname", list(gen.CONFIGS))
def test_plans_are_the_recorded_plans(hip_lib, gold, cname):
    from diffews_amd import _lib as L
    cfg = gen.CONFIGS[cname]
    wrong, wrong_blocks = [], []
    try:
        gen.configured(L, cfg)
        for op in gen.OPS:
            whole = gen.plan_values(L, hip_lib, op, "whole")
            tier = "whole" if cname == "default" else "reduced"
            new = whole if tier == "whole" else gen.plan_values(L, hip_lib, op, tier)
            old = [gold["values"][int(i)] for i in gold["core"][f"{op}/{cname}"].split()]
            args = gen.rows(op, tier)
            assert len(old) == len(new) == len(args)
            wrong += [(a, o, n) for a, o, n in zip(args, old, new) if o != n]
            if gen.block_hash(whole) != gold["wide"][f"{op}/{cname}"]:
                wrong_blocks.append(f"{op}/{cname}")
    finally:
        L.configure()
    assert not wrong, f"{len(wrong)} core rows differ under config {cname} = {cfg} (recorded at {gold['commit']}):\n" + "\n".join(
        f"  {a}: recorded {o}, now {n}" for a, o, n in wrong[:20])
    assert not wrong_blocks, f"wide blocks differ from {gold['commit']}: {wrong_blocks}"


@pytest.mark.parametrize("op", gen.OPS)
def test_plan_ignores_the_storage_dtype(hip_lib, op):
    from diffews_amd import _lib as L
    L.configure()
    assert gen.plan_values(L, hip_lib, op, "reduced", L.F16) == gen.plan_values(L, hip_lib, op, "reduced", L.BF16)


@pytest.mark.parametrize("op", gen.OPS)
def test_plan_ignores_workspace_and_partial_sum_buffers(hip_lib, op):
    """The queries run before those buffers exist, the launch with them: both must see one plan."""
    from diffews_amd import _lib as L
    L.configure()
    assert gen.plan_values(L, hip_lib, op, "reduced", buffers=True) == gen.plan_values(L, hip_lib, op, "reduced")
