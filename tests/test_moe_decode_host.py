"""CPU: the decode path of the mixture-of-experts layers in the C ABI (gptq_moe_decode_*: exports, plan, workspace formula, declines), that the grouped
path's answers are unchanged, and -- read off the built code objects -- that the new kernels are scratch-free and the load-time kernels that paid for their
instantiations are compiled once."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402

DECODE_SYMBOLS = ("gptq_moe_decode_table_bytes", "gptq_moe_build_decode_table", "gptq_moe_decode_workspace_bytes", "gptq_moe_decode_forward",
                  "gptq_describe_moe_decode_plan")


def _layer(K, N, bits=4, gs=128, dtype=_lib.GPTQ_F16, copy=True, act=False):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000          # never dereferenced by the host-only queries
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = K, N, bits, min(gs, K) if gs > 0 else K, dtype, 0
    if copy:
        L.qweight_tiled, L.qconst_tiled, L.tiled_cols = 0x5000, 0x6000, 16
    if act:
        L.g_idx, L.qweight_seq, L.perm = 0x2000, 0x3000, 0x4000
    return L


def _moe(E=8, H=256, I=512, **kw):
    layers = [[_layer(H, I, **kw) for _ in range(E)], [_layer(H, I, **kw) for _ in range(E)], [_layer(I, H, **kw) for _ in range(E)]]
    arrs = [(ctypes.POINTER(_lib.GptqLayer) * E)(*[ctypes.pointer(l) for l in ls]) for ls in layers]
    m = _lib.GptqMoe()
    m.E = E
    m.gate, m.up, m.down = (ctypes.addressof(a) for a in arrs)
    m._keep = (layers, arrs)
    return m


def _a256(b):
    return (b + 255) // 256 * 256


def test_decode_symbols_exported_and_declared_abi_8():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in DECODE_SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert "#define GPTQ_MI355X_ABI_VERSION 8" in header
    assert int(lib.gptq_moe_decode_table_bytes(8)) == 3 * 8 * 32 and int(lib.gptq_moe_decode_table_bytes(0)) == 0


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [32, 128, -1])
@pytest.mark.parametrize("bits", [4, 8])
def test_plan_accepts_1_to_4_tokens(bits, gs, act):
    lib = _lib.load()
    for E, topk, H, I, dtype in ((8, 2, 256, 512, _lib.GPTQ_F16), (60, 4, 2048, 1408, _lib.GPTQ_BF16), (8, 2, 4096, 14336, _lib.GPTQ_F16)):
        m = _moe(E, H, I, bits=bits, gs=gs, dtype=dtype, act=act)
        for T in (1, 2, 3, 4):
            d = _lib.describe_moe_decode_plan(m, T, topk)
            assert d["path"] == "decode" and d["launches"] == 2, d
            assert d["wg_pair"] == T * topk * I // 16 and d["wg_down"] == T * H // 16, d
            assert d["lds_pair"] <= 160 * 1024 and d["lds_down"] <= 160 * 1024, d
            got = int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), T, topk))
            assert got == _lib.WS_HEADER_BYTES + _a256(T * topk * I * 2) + _a256(4 * T * topk), (T, got)
        d0 = _lib.describe_moe_decode_plan(m, 0, topk)
        assert d0["path"] == "decode" and d0["launches"] == 0, d0
        # T = 0: nothing is launched, nothing is dereferenced
        assert lib.gptq_moe_decode_forward(ctypes.byref(m), None, None, None, None, 0, topk, None, None, None, 0, None) == 0


@pytest.mark.parametrize("kw,T,topk,frag", [
    (dict(), 5, 2, "T = 5"),
    (dict(copy=False), 1, 2, "no decode copy"),
    (dict(bits=3), 1, 2, "3-bit"),
    (dict(bits=2), 1, 2, "2-bit"),
    (dict(dtype=_lib.GPTQ_F32), 1, 2, "fp32"),
    (dict(), 1, 9, "topk = 9"),
    (dict(gs=48), 1, 2, "group_size"),
])
def test_plan_declines_with_a_reason(kw, T, topk, frag):
    lib = _lib.load()
    m = _moe(**kw)
    d = _lib.describe_moe_decode_plan(m, T, topk)
    assert d["path"] == "none" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
    assert int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), T, topk)) == 0
    rc = lib.gptq_moe_decode_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, T, topk, 0x1000, None, 0x1000, 1 << 30, None)
    assert rc == 3 and frag in lib.gptq_last_error().decode()


def test_one_expert_without_a_copy_declines():
    m = _moe()
    m._keep[0][2][5].qweight_tiled = m._keep[0][2][5].qconst_tiled = None
    m._keep[0][2][5].tiled_cols = 0
    d = _lib.describe_moe_decode_plan(m, 1, 2)
    assert d["path"] == "none" and "expert_5_down" in d["reason"], d


@pytest.mark.parametrize("copy", [False, True])
def test_grouped_answers_are_unchanged(copy):
    """The grouped entry points answer for layers with and without a decode copy exactly as before this path existed."""
    lib = _lib.load()
    for E, topk, H, I in ((8, 2, 256, 512), (8, 2, 4096, 14336)):
        m = _moe(E, H, I, copy=copy)
        for T in (0, 1, 4, 64):
            d = _lib.describe_moe_plan(m, T, topk)
            assert d["path"] == "grouped" and d["bn"] == 64 and d["launches"] == (4 if T else 0), d
            R = T * topk
            assert d["tiles"] == R // d["bm"] + min(E, R)
            want = (_lib.WS_HEADER_BYTES + _a256(4 * (E + 1)) + 256 + _a256(16 * d["tiles"]) + 2 * _a256(4 * R) + _a256(R * I * 2)
                    + _a256(4 * d["ksplit"] * R * H))
            assert int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), T, topk)) == want
        assert int(lib.gptq_moe_table_bytes(E)) == 3 * E * 32
    buf = ctypes.create_string_buffer(256)
    assert lib.gptq_describe_moe_plan(ctypes.byref(_moe(copy=copy)), 1, 2, buf, len(buf)) == 0
    assert buf.value.decode() == "path=grouped bm=16 bn=64 tiles=2 ksplit=1 launches=4"


def test_decode_kernels_are_scratch_free_and_the_load_time_kernels_are_compiled_once():
    from test_kernel_resources import _kernels
    ks = _kernels()
    dec = {n: v for n, v in ks.items() if "moe_decode_kernel" in n}
    assert len(dec) == 8, sorted(dec)                                # <T, BITS, PAIR>: fp16 / bf16 x 4 / 8 bits x the two launches
    for n, v in dec.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0) and (v["vgpr"] or 0) <= 128, (n, v)      # 16-wave workgroups: 4 waves per SIMD
    for fam in ("resequence_kernel", "prepack_decode_weights_kernel", "unprepack_decode_weights_kernel"):
        assert sum(1 for n in ks if re.search(r"\d" + fam, n)) == 1, fam          # (mangled: <length><name>)
    assert len(ks) <= 1160, len(ks)
