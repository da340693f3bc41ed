"""CPU (-m "not gpu"): plan_gemm (csrc/gemm.hip) as one function per rung decides what the one 290-line function decided.

tests/golden/plans_gemm_parent.json was recorded from a build of the PARENT commit of that split (tests/golden/make_plans_gemm_parent.py): 43 layers (2 / 3 / 4 / 8
bits, fp16 / bf16 / fp32, seven shapes, with and without the decode copy, plain and act-order, the flagged 2-bit copy in both forms) x 27 row counts x
{no tuning + 38 lab-knob settings}.  This build reproduces it exactly: gptq_describe_plan's line or error text, gptq_workspace_bytes_ex / _max / _multi_ex.
Plan queries on fake pointers: host arithmetic, no GPU."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_plans_gemm_parent as GEN  # noqa: E402

WANT = json.load(open(os.path.join(ROOT, "tests", "golden", "plans_gemm_parent.json")))


def test_the_fixture_exercises_every_rule_of_the_ladder():
    """Asked of the FIXTURE (the parent's answers without tuning), not of this build: every GemmKernel name, a balanced tail, two K groups, the wide kernel on
    the decode copy and the low-bit body occur -- and both K steps of the tiled kernel."""
    assert len(WANT) == len(GEN.LAYERS) == 43 and all(len(v["rows"]) == len(GEN.ROWS) == 27 for v in WANT.values())
    lines = [row["none"][0] for v in WANT.values() for row in v["rows"].values() if row["none"][0].startswith("path=gemm ")]
    kernels = {re.search(r"kernel=(\S+)", ln).group(1) for ln in lines}
    assert kernels == {"tiled", "f32_mfma", "panel", "rows", "wide_sk", "wide", "wide_copy", "mid", "stream64", "strip16", "skinny64"}, kernels
    assert any(int(re.search(r" tail=(\d+)", ln).group(1)) > 0 for ln in lines)
    assert any(" kg=2 " in ln for ln in lines) and any(ln.endswith(" body=lowbit") for ln in lines)
    assert {re.search(r" bk=(\d+)", ln).group(1) for ln in lines if "kernel=tiled " in ln} == {"32", "64"}
    assert all(re.fullmatch(r"[0-9a-f]{64}", row["knobs"]) for v in WANT.values() for row in v["rows"].values())


def test_every_plan_is_the_parent_commits():
    bad = []
    for c in GEN.cases():
        got, ref = GEN.query(GEN.layer(*c)), WANT[GEN.key(*c)]
        if got["max"] != ref["max"]:
            bad.append((GEN.key(*c), "max", got["max"], ref["max"]))
        for M, row in ref["rows"].items():
            if got["rows"][M]["none"] != row["none"]:
                bad.append((GEN.key(*c), M, "none", got["rows"][M]["none"], row["none"]))
            if got["rows"][M]["knobs"] != row["knobs"]:      # (which knob: run the generator with --full against both builds and diff)
                bad.append((GEN.key(*c), M, "knob sweep"))
    assert not bad, (len(bad), bad[:8])
