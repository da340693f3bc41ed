"""CPU (host-only queries): which decode-copy launches stage x and the constants in TWO steps (TiledPlan.xsteps, "xstage" of describe_plan()).

The rule: a plain 4-bit fp16 layer with its decode copy, one strip per workgroup, no K slices, K deeper than one pass of the planned workgroup
(waves x u chunks of 128 k).  Pinned over the projections of Llama-7B, 13B and a 70B tensor-parallel shard, next to the forms that must stay one-step:
act-order, bf16, 2- / 3- / 8-bit, the gated pair, two strips per workgroup, K slices, 5..8 rows on other kernels, and the lab switch.  The C line of
gptq_describe_plan does not carry the key (tests/test_forward_entry_contract.py pins it byte for byte): gptq_describe_plan_xstage answers beside it."""
import ctypes

import pytest

from autogptq_amd import _lib


def _layer(K, N, *, bits=4, gs=128, dtype=0, act=False, epilogue=0, copy=True):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000                              # never dereferenced by the planner
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode, L.epilogue = K, N, bits, gs, dtype, 0, epilogue
    if copy:
        L.qweight_tiled = L.qconst_tiled = 0x2000
        L.tiled_cols = 16
    if act:
        L.g_idx = L.qweight_seq = L.perm = 0x1000
    return L


def _plan(L, M, tuning=None):
    return _lib.describe_plan(L, M, tuning)


def _want(d, K):
    return 2 if (d["ksplit"] == 1 and K > d["waves"] * d["u"] * 128) else 1


# (K, N): q / k / v / o, gate / up, down of Llama-7B and 13B; the 70B projections cut in eight column- / row-wise
SHAPES_7B = [(4096, 4096), (4096, 11008), (11008, 4096)]
SHAPES_13B = [(5120, 5120), (5120, 13824), (13824, 5120)]
SHAPES_70B_SHARD = [(8192, 1024), (8192, 3584), (1024, 8192), (3584, 8192), (28672, 1024)]


@pytest.mark.parametrize("K,N", SHAPES_7B + SHAPES_13B + SHAPES_70B_SHARD)
def test_plain_fp16_layers_follow_the_rule(K, N):
    L = _layer(K, N)
    for M in (1, 2, 3, 4):
        d = _plan(L, M)
        if d["kernel"] != "strips":
            assert "xstage" not in d, d
            continue
        assert d["xstage"] == _lib.load().gptq_describe_plan_xstage(ctypes.byref(L), M, None)
        two_strips = d["strips"] * 16 != N                                # two strips per workgroup: gemv_tiled_multi.hip, one step
        assert d["xstage"] == (1 if two_strips else _want(d, K)), (K, N, M, d)


def test_the_headline_launches():
    """o (one pass of 16 waves x 2 chunks = 4096 k): one step.  down (11008 = 2.7 passes) and a q / k / v layer on its own (4 waves x 4 chunks = 2048 k): two."""
    assert _plan(_layer(4096, 4096), 1)["xstage"] == 1
    d = _plan(_layer(11008, 4096), 1)
    assert (d["waves"], d["u"], d["ksplit"], d["xstage"]) == (16, 2, 1, 2), d
    d = _plan(_layer(4096, 12288), 1)
    assert (d["waves"], d["u"], d["xstage"]) == (4, 4, 2), d
    d = _plan(_layer(13824, 5120), 1)                                     # 13B down: 27 KB of x in front of the first decode before
    assert d["ksplit"] == 1 and d["xstage"] == 2, d
    d = _plan(_layer(28672, 1024), 1)                                     # 70B down shard: K slices stage a slice each
    assert d["ksplit"] > 1 and d["xstage"] == 1, d


@pytest.mark.parametrize("what,kw", [("act-order", dict(act=True)), ("bf16", dict(dtype=1)), ("3-bit", dict(bits=3)), ("8-bit", dict(bits=8)), ("2-bit", dict(bits=2)),
                                      ("whole-K group", dict(gs=11008))])
def test_the_other_forms_stay_one_step(what, kw):
    L = _layer(11008, 4096, **kw)
    for M in (1, 4):
        d = _plan(L, M)
        if d["kernel"] == "strips":
            assert d["xstage"] == (2 if what == "whole-K group" else 1), (what, M, d)


def test_pair_and_two_strip_forms_stay_one_step():
    d = _plan(_layer(4096, 22016, epilogue=_lib.EPI_SILU_MUL), 1)
    assert d["kernel"] == "strips" and d["pair"] == 1 and d["xstage"] == 1, d
    d = _plan(_layer(4096, 22016), 1)                                     # 1376 strips: two per workgroup
    assert d["kernel"] == "strips" and d["strips"] == 688 and d["xstage"] == 1, d


def test_the_lab_switch_keeps_one_step_and_nothing_else_moves():
    L = _layer(11008, 4096)
    t = _lib.GptqTuning()
    t.reserved[_lib.LAB.GEMM_VARIANT] = _lib.LAB.VARIANT_TILED_ONE_STEP
    d, d1 = _plan(L, 1), _plan(L, 1, t)
    assert d["xstage"] == 2 and d1["xstage"] == 1
    assert {k: v for k, v in d.items() if k != "xstage"} == {k: v for k, v in d1.items() if k != "xstage"}
    lib = _lib.load()
    assert lib.gptq_workspace_bytes_ex(ctypes.byref(L), 1, None) == lib.gptq_workspace_bytes_ex(ctypes.byref(L), 1, ctypes.byref(t))


def test_layers_without_a_decode_copy_have_no_staging_to_report():
    L = _layer(11008, 4096, copy=False)
    assert "xstage" not in _plan(L, 1)
    assert _lib.load().gptq_describe_plan_xstage(ctypes.byref(L), 1, None) == 0
    assert _lib.load().gptq_describe_plan_xstage(ctypes.byref(L), 0, None) == 0
