"""CPU: the mixture-of-experts entry points of the C ABI (exports, workspace formula, plan), and a tiny Mixtral that round-trips through
pack_moe_experts -> a checkpoint with AutoGPTQ's ``block_sparse_moe`` names -> load_packed_layers into a fresh transformers-5 skeleton."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402

MOE_SYMBOLS = ("gptq_moe_table_bytes", "gptq_moe_build_table", "gptq_moe_workspace_bytes", "gptq_moe_forward", "gptq_describe_moe_plan")


def _layer(K, N, bits=4, gs=128, dtype=_lib.GPTQ_F16, **kw):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000          # never dereferenced by the host-only queries
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = K, N, bits, gs, dtype, 0
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def _moe(E=8, H=256, I=512, **kw):
    layers = [[_layer(H, I, **kw) for _ in range(E)], [_layer(H, I, **kw) for _ in range(E)], [_layer(I, H, **kw) for _ in range(E)]]
    arrs = [(ctypes.POINTER(_lib.GptqLayer) * E)(*[ctypes.pointer(l) for l in ls]) for ls in layers]
    m = _lib.GptqMoe()
    m.E = E
    m.gate, m.up, m.down = (ctypes.addressof(a) for a in arrs)
    m._keep = (layers, arrs)
    return m


def test_moe_symbols_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in MOE_SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and hasattr(lib, s), s


def _a256(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("E,topk,H,I,dtype", [(8, 2, 256, 512, _lib.GPTQ_F16), (60, 4, 2048, 1408, _lib.GPTQ_BF16), (8, 2, 4096, 14336, _lib.GPTQ_F16)])
def test_workspace_bytes_formula(E, topk, H, I, dtype):
    lib = _lib.load()
    m = _moe(E, H, I, dtype=dtype)
    prev = 0
    for T in (0, 1, 2, 7, 64, 300, 2048):
        got = int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), T, topk))
        d = _lib.describe_moe_plan(m, T, topk)
        assert d["path"] == "grouped", d
        R = T * topk
        assert d["tiles"] == R // d["bm"] + min(E, R)
        want = (_lib.WS_HEADER_BYTES + _a256(4 * (E + 1)) + 256 + _a256(16 * d["tiles"]) + 2 * _a256(4 * R) + _a256(R * I * 2)
                 + _a256(4 * d["ksplit"] * R * H))
        assert got == want, (T, got, want, d)
        assert got >= prev
        prev = got
    assert int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), 2048, topk)) > int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), 1, topk))
    assert int(lib.gptq_moe_table_bytes(E)) == 3 * E * 32


@pytest.mark.parametrize("bits,gs", [(4, 32), (4, 128), (4, 256), (8, 32), (8, 128), (8, 256)])
def test_plan_accepts_4_and_8_bits(bits, gs):
    m = _moe(bits=bits, gs=gs)         # gs 256 = K of gate / up: group_size -1 resolved
    d = _lib.describe_moe_plan(m, 1, 2)
    assert d["path"] == "grouped" and d["bn"] == 64 and d["launches"] == 4, d
    assert _lib.describe_moe_plan(m, 0, 2)["launches"] == 0


@pytest.mark.parametrize("kw,frag", [(dict(bits=3), "3-bit"), (dict(bits=2), "2-bit"), (dict(dtype=_lib.GPTQ_F32), "fp32"), (dict(gs=48), "group_size")])
def test_plan_declines_with_a_reason(kw, frag):
    lib = _lib.load()
    m = _moe(**kw)
    d = _lib.describe_moe_plan(m, 1, 2)
    assert d["path"] == "per_expert" and frag in d["reason"], d
    assert int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), 1, 2)) == 0
    rc = lib.gptq_moe_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, 1, 2, 0x1000, None, 0x1000, 1 << 30, None)
    assert rc == 3 and frag in lib.gptq_last_error().decode()


def test_plan_declines_raw_act_order_and_topk_over_8():
    assert _lib.describe_moe_plan(_moe(g_idx=0x2000), 1, 2)["path"] == "per_expert"
    assert _lib.describe_moe_plan(_moe(g_idx=0x2000, qweight_seq=0x3000, perm=0x4000), 1, 2)["path"] == "grouped"
    assert _lib.describe_moe_plan(_moe(), 1, 9)["path"] == "per_expert"


def test_quant_moe_experts_state_dict_names():
    from autogptq_amd.moe import QuantMoEExperts
    q = QuantMoEExperts(4, 256, 512, 4, 128)
    keys = set(q.state_dict())
    assert "0.w1.qweight" in keys and "3.w2.g_idx" in keys and "2.w3.scales" in keys and "1.w1.qzeros" in keys
    q2 = QuantMoEExperts(2, 256, 512, 4, 128, names=("gate_proj", "up_proj", "down_proj"))
    assert "1.down_proj.qweight" in q2.state_dict()
    assert q.plan(1)["path"] == "per_expert"                  # CPU module: the composition (QuantLinear refuses CPU tensors itself)


@pytest.mark.parametrize("desc_act", [False, True])
def test_tiny_mixtral_checkpoint_round_trip(tmp_path, desc_act):
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    import _tiny_mixtral as TM
    from autogptq_amd.moe import QuantMoEExperts

    model = TM.fresh_model(0)
    TM.quantize_and_pack(model, desc_act)
    TM.save_checkpoint(model, str(tmp_path), desc_act)
    loaded, sd, _ = TM.load_checkpoint(str(tmp_path))
    assert any(".block_sparse_moe.experts.0.w1.qweight" in k for k in sd)
    for li in range(2):
        ex = loaded.model.layers[li].mlp.experts
        assert isinstance(ex, QuantMoEExperts) and ex.num_experts == TM.E and ex.top_k == TM.TOPK
    src = TM.autogptq_names(model.state_dict())
    got = TM.autogptq_names(loaded.state_dict())
    assert set(src) == set(got)
    for k, v in src.items():
        assert torch.equal(got[k].cpu(), v.cpu()), k
