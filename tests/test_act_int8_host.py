"""CPU: the C ABI of the opt-in int8-activation path (gptq_act_int8_workspace_bytes, gptq_act_quant, gptq_gemm_a8, gptq_forward_a8, gptq_describe_a8_plan):
exports, the documented workspace formula, every decline and the host-only plan string.  Every call below returns before a launch."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear  # noqa: E402

SYMBOLS = ("gptq_act_int8_workspace_bytes", "gptq_act_quant", "gptq_gemm_a8", "gptq_forward_a8", "gptq_describe_a8_plan")
FAKE = 0x1000                              # never dereferenced


def _layer(K=4096, N=4096, bits=4, gs=128, dtype=_lib.GPTQ_F16, copy=True, act=False, perm=True):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = FAKE
    L.K, L.N, L.bits, L.group_size, L.dtype = K, N, bits, gs, dtype
    if copy:
        L.qweight_tiled = L.qconst_tiled = FAKE
        L.tiled_cols = _lib.STRIP_COLS
    if act:
        L.g_idx = FAKE
        if perm:
            L.qweight_seq = L.perm = FAKE
    return L


def test_symbols_exported_and_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    for s in SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(lib, s) and s + "(" in header, s
    assert lib.gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert QuantLinear.ACT_INT8 is False and QuantLinear.ACT_INT8_MIN_ROWS == 128


@pytest.mark.parametrize("K,N,gs,M", [(128, 16, 128, 1), (384, 144, 32, 129), (4096, 11008, 128, 4096), (11008, 4096, 11008, 257), (160, 32, 64, 5)])
def test_workspace_is_the_documented_formula_and_the_plan_parses(K, N, gs, M):
    L = _layer(K, N, gs=gs)
    want = (4 * M + 255) // 256 * 256 + (M * 128 * ((K + 127) // 128) + 255) // 256 * 256
    assert _lib.load().gptq_act_int8_workspace_bytes(ctypes.byref(L), M) == want
    d = _lib.describe_a8_plan(L, M)
    assert d["path"] == "act_int8" and d["tile"] == "128x128" and d["waves"] == 4 and d["zero"] == "signed_bytes" and d["launches"] == 2
    assert d["workspace"] == want and d["tiles"] == f"{(M + 127) // 128}x{(N + 127) // 128}" and d["chunks"] == (K + 127) // 128
    assert d["group_mode"] == ("one" if gs >= K else {32: "g32", 64: "g64", 128: "g128"}[gs]) and d["groups"] == (K + gs - 1) // gs


@pytest.mark.parametrize("kw,word", [(dict(bits=3), "4-bit"), (dict(bits=2), "4-bit"), (dict(bits=8), "4-bit"), (dict(dtype=_lib.GPTQ_F32), "fp16"),
                                     (dict(copy=False), "decode copy"), (dict(act=True, perm=False), "perm"), (dict(gs=96), "group sizes"),
                                     (dict(gs=384), "group sizes")])
def test_declined_layers_get_no_workspace_and_a_reason(kw, word):
    lib = _lib.load()
    L = _layer(**kw)
    assert lib.gptq_act_int8_workspace_bytes(ctypes.byref(L), 128) == 0
    assert lib.gptq_forward_a8(ctypes.byref(L), FAKE, FAKE, 128, FAKE, 1 << 30, None) == 3          # GPTQ_ERR_UNSUPPORTED, before any launch
    assert word in lib.gptq_last_error().decode()
    assert lib.gptq_act_quant(ctypes.byref(L), FAKE, 128, FAKE, 1 << 30, None) == 3 and lib.gptq_gemm_a8(ctypes.byref(L), FAKE, FAKE, 128, None) == 3
    d = _lib.describe_a8_plan(L, 128)
    assert d["path"] == "none" and word.replace(" ", "_") in d["reason"]


def test_the_switch_is_off_until_post_init_and_held_off_under_a_wrapper():
    """The flag lives in QuantLinear, not in gptq_layer_t (flag off against flag absent on an initialised layer: tests/test_gpu_act_int8.py).  Without a GPU: a
    fresh layer has no int8 rows, and a tensor-parallel wrapper marks its shard so that a later post_init(act_int8=True) leaves the path off."""
    from autogptq_amd.tensor_parallel import ColumnParallelQuantLinear
    q = QuantLinear(4, 128, 256, 128, False)
    assert q._a8_rows == 0 and q._a8_hold is False
    q._a8_rows = 128                                   # as post_init(act_int8=True) would leave it
    ColumnParallelQuantLinear(q, 128)
    assert q._a8_hold is True and q._a8_rows == 0
