"""CPU (-m "not gpu"): the GeGLU epilogue ('gelu_tanh_mul', gptq_epilogue_t 2) and the fused MLP callers for Gemma (three projections, tanh-GELU) and
Phi-3 / GLM-4 (one ``gate_up_proj``, SiLU) -- constructor rules, the C ABI's additions, plans equal to the SiLU layer's, the kernel inventory unchanged (the
activation is an argument of the code objects that were there), and the injection on the host model's own MLP classes."""
import ctypes

import pytest
import torch
import torch.nn as nn

from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear

TILED_FORMS = 248      # gemv_tiled_kernel code objects of the parent build: 212 plain / act-order / tensor-parallel / multi-strip + 36 pair forms


def test_constructor_takes_the_geglu_epilogue():
    q = QuantLinear(4, 64, 256, 128, False, epilogue="gelu_tanh_mul")
    assert q.epilogue == "gelu_tanh_mul" and q.out_width == 64
    assert QuantLinear(4, 64, 256, 128, False, epilogue="silu_mul").out_width == 64 and QuantLinear(4, 64, 256, 128, False).out_width == 128
    with pytest.raises(ValueError, match="divisible by 64"):
        QuantLinear(4, 64, 256, 96, False, epilogue="gelu_tanh_mul")
    with pytest.raises(ValueError, match="epilogue must be"):
        QuantLinear(4, 64, 256, 128, False, epilogue="gelu_mul")
    assert (_lib.EPI_NONE, _lib.EPI_SILU_MUL, _lib.EPI_GELU_TANH_MUL) == (0, 1, 2)


def test_lora_wrappers_refuse_the_geglu_layer_as_they_refuse_silu_mul():
    from autogptq_amd.adapter_bank import LoraBankQuantLinear
    from autogptq_amd.lora import LoraQuantLinear
    for epi in ("silu_mul", "gelu_tanh_mul"):
        q = QuantLinear(4, 64, 256, 128, False, epilogue=epi)
        with pytest.raises(ValueError, match=epi):
            LoraQuantLinear(q, 8, 16.0)
        with pytest.raises(ValueError, match=epi):
            LoraBankQuantLinear(q, 8, 2)


def test_library_exports_mlp_forward_act_under_the_same_abi():
    lib = _lib.load()
    assert hasattr(lib, "gptq_mlp_forward_act") and "gptq_mlp_forward_act" in _lib.EXPORTS
    assert lib.gptq_abi_version() == 8


def _layer(**kw):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000      # never dereferenced: host-only queries and refusals
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = 4096, 2 * 1408, 4, 128, 0, 0
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def _with_copy(L):
    L.qweight_tiled = L.qconst_tiled = 0x2000
    L.tiled_cols = 16
    return L


@pytest.mark.parametrize("kw", [dict(), dict(copy=True), dict(copy=True, bits=3, group_size=32), dict(copy=True, bits=8, group_size=32), dict(copy=True, dtype=1),
                                dict(act=True), dict(copy=True, act=True), dict(K=1024, N=2 * 5632), dict(copy=True, bits=2)],
                         ids=["rows", "copy", "copy-int3", "copy-int8", "copy-bf16", "act", "copy-act", "wide", "copy-int2"])
def test_plans_and_workspaces_are_those_of_the_silu_layer(kw):
    lib = _lib.load()
    kw = dict(kw)
    copy, act = kw.pop("copy", False), kw.pop("act", False)
    seen = set()
    for M in (1, 4, 8, 64):
        Ls = []
        for epi in (1, 2):
            L = _layer(epilogue=epi, **kw)
            if copy:
                _with_copy(L)
            if act:
                L.g_idx = L.qweight_seq = L.perm = 0x1000
            Ls.append(L)
        a, b = (_lib.describe_plan(L, M) for L in Ls)
        assert a == b and a["epilogue"] in ("fused", "separate"), (M, a, b)
        assert lib.gptq_workspace_bytes(ctypes.byref(Ls[0]), M) == lib.gptq_workspace_bytes(ctypes.byref(Ls[1]), M)
        seen.add((a["kernel"], a["epilogue"]))
    if copy and not act and kw.get("bits") != 2:
        assert _lib.describe_plan(_with_copy(_layer(epilogue=2, **kw)), 1)["pair"] in (1, "1")      # the pair form of the decode-copy kernel
    assert len(seen) >= 2, seen                                                                # the row counts cover more than one route


def test_unknown_epilogue_and_shape_rule():
    lib = _lib.load()
    with pytest.raises(_lib.GptqError, match="unknown epilogue 3"):
        _lib.describe_plan(_layer(epilogue=3), 1)
    L = _layer(epilogue=2, N=96)
    assert lib.gptq_forward(ctypes.byref(L), 0x1000, 0x1000, 1, None, 0, None) == 2
    assert "GELU_TANH_MUL epilogue needs out_features (96)" in lib.gptq_last_error().decode()
    L = _layer(epilogue=1, N=96)
    assert lib.gptq_forward(ctypes.byref(L), 0x1000, 0x1000, 1, None, 0, None) == 2
    assert "SILU_MUL epilogue needs out_features (96)" in lib.gptq_last_error().decode()


def test_mlp_forward_act_refuses_any_other_activation_before_a_launch():
    lib = _lib.load()
    g, u, d = _layer(N=1408), _layer(N=1408), _layer(K=1408, N=4096)
    for act in (0, 3, -1):
        rc = lib.gptq_mlp_forward_act(ctypes.byref(g), ctypes.byref(u), ctypes.byref(d), act, 0x1000, 0x1000, 1, None, 0, None)
        assert rc == 3 and "act must be" in lib.gptq_last_error().decode(), (act, rc)
    for act in (1, 2):          # a served activation goes on to the ordinary checks: no workspace -> refused with that status, nothing launched
        rc = lib.gptq_mlp_forward_act(ctypes.byref(g), ctypes.byref(u), ctypes.byref(d), act, 0x1000, 0x1000, 1, None, 0, None)
        assert rc == 4, (act, rc, lib.gptq_last_error())
    a = _lib.describe_mlp_plan(g, u, d, 4)
    assert a["kernel"] == "unfused" and "silu_mul" in a["steps"]                                 # gptq_describe_mlp_plan: unchanged


def test_the_activation_is_an_argument_not_a_new_code_object():
    from test_kernel_resources import _kernels
    ks = _kernels()                                         # skips where the LLVM tools or the library are missing
    assert len([n for n in ks if "silu_mul_kernel" in n]) == 1
    assert len([n for n in ks if "silu_mul2_kernel" in n]) == 1
    perm = sorted(n for n in ks if "silu_mul2_permute_rows4_kernel" in n)
    assert len(perm) == 2 and "IDF16_E" in perm[0] and "IDF16bE" in perm[1], perm
    # each of them takes one more int than on the parent (the mangled parameter lists end in the new `i`)
    assert [n for n in ks if "silu_mul_kernel" in n][0].endswith("EPKvPviiii") and [n for n in ks if "silu_mul2_kernel" in n][0].endswith("EPKvS2_Pvmii")
    assert all(n.endswith("PKiiiPti") for n in perm)
    tiled = {n: v for n, v in ks.items() if "gemv_tiled_kernel" in n}
    assert len(tiled) == TILED_FORMS, len(tiled)
    pair = {n: v for n, v in tiled.items() if "ELi4ELi0EEEvNS_11TiledParamsE" in n}              # XM = 4
    assert len(pair) == 36 and all(v["vgpr"] <= 128 and not v["spill"] and not v["scratch"] for v in pair.values())
    assert len(ks) <= 1160, len(ks)


# ---- injection on the host model's own MLP modules (CPU: nothing is initialised, nothing runs) ------------------------------------------------------
def _quantised(mlp):
    from autogptq_amd.model_utils import find_layers, make_quant
    make_quant(mlp, list(find_layers(mlp)), 4, 64)
    assert all(isinstance(m, QuantLinear) for n, m in mlp.named_children() if n.endswith("_proj"))
    return mlp


def _tiny(kind, **kw):
    if kind == "gemma":
        from transformers import GemmaConfig
        from transformers.models.gemma.modeling_gemma import GemmaMLP
        return GemmaMLP(GemmaConfig(hidden_size=128, intermediate_size=256, **kw))
    if kind == "gemma2":
        from transformers import Gemma2Config
        from transformers.models.gemma2.modeling_gemma2 import Gemma2MLP
        return Gemma2MLP(Gemma2Config(hidden_size=128, intermediate_size=256, **kw))
    from transformers import Phi3Config
    from transformers.models.phi3.modeling_phi3 import Phi3MLP
    return Phi3MLP(Phi3Config(hidden_size=128, intermediate_size=256, **kw))


@pytest.mark.parametrize("kind", ["gemma", "gemma2"])
def test_inject_fuses_the_geglu_mlp_of_gemma(kind):
    from autogptq_amd.fused import FusedGateUpMLP, inject_fused_llama
    mlp = _quantised(_tiny(kind))
    assert type(mlp.act_fn).__name__ == "GELUTanh"
    keys = list(mlp.state_dict())
    assert inject_fused_llama(mlp, fuse_mlp=False) == 0 and "forward" not in mlp.__dict__
    assert inject_fused_llama(mlp) == 1
    fm = mlp.__dict__["fused_mlp"]
    assert isinstance(fm, FusedGateUpMLP) and fm.act == "gelu_tanh" and fm.gate_up is None
    assert mlp.__dict__["forward"].__self__ is fm
    assert list(mlp.state_dict()) == keys


def test_inject_maps_activation_classes_and_leaves_erf_gelu_alone():
    from transformers.activations import ACT2FN
    from autogptq_amd.fused import gated_act_name, inject_fused_llama
    assert [gated_act_name(ACT2FN[k]) for k in ("silu", "gelu_pytorch_tanh", "gelu_new", "gelu", "relu")] == ["silu", "gelu_tanh", "gelu_tanh", None, None]
    assert [gated_act_name(f) for f in (nn.SiLU(), nn.GELU(approximate="tanh"), nn.GELU(), None)] == ["silu", "gelu_tanh", None, None]
    g = torch.linspace(-6, 6, 1001, dtype=torch.float64)
    assert float((ACT2FN["gelu_new"](g) - torch.nn.functional.gelu(g, approximate="tanh")).abs().max()) <= 1e-15      # gelu_new IS tanh-GELU
    mlp = _quantised(_tiny("gemma2", hidden_activation="gelu"))
    assert type(mlp.act_fn).__name__ == "GELUActivation"
    assert inject_fused_llama(mlp) == 0 and "forward" not in mlp.__dict__
    phi = _quantised(_tiny("phi3", hidden_act="gelu"))
    assert inject_fused_llama(phi) == 0 and phi.gate_up_proj.epilogue == "none" and "forward" not in phi.__dict__


def test_inject_gives_phi3_gate_up_proj_its_epilogue_in_place_and_remove_restores_it():
    from autogptq_amd.fused import inject_fused_llama, remove_fused_mlp
    mlp = _quantised(_tiny("phi3"))
    gu, sd = mlp.gate_up_proj, mlp.state_dict()
    keys, ptrs = list(sd), {k: v.data_ptr() for k, v in sd.items()}
    assert (gu.infeatures, gu.outfeatures, gu.epilogue, gu.out_width) == (128, 512, "none", 512)
    assert inject_fused_llama(mlp, fuse_mlp=False) == 0 and gu.epilogue == "none"
    assert inject_fused_llama(mlp) == 1
    assert mlp.gate_up_proj is gu and (gu.epilogue, gu.out_width) == ("silu_mul", 256) and "forward" in mlp.__dict__
    sd2 = mlp.state_dict()
    assert list(sd2) == keys and {k: v.data_ptr() for k, v in sd2.items()} == ptrs          # no tensor copied or renamed
    assert inject_fused_llama(mlp) == 0                                                      # already a gated layer: not counted twice
    assert remove_fused_mlp(mlp) == 1
    assert (gu.epilogue, gu.out_width) == ("none", 512) and "forward" not in mlp.__dict__ and mlp.forward.__func__ is type(mlp).forward
    assert list(mlp.state_dict()) == keys and remove_fused_mlp(mlp) == 0
    # a tanh-GELU gate_up_proj module gets the GeGLU epilogue; a width that is no multiple of 64 is left alone
    geglu = _quantised(_tiny("phi3", hidden_act="gelu_pytorch_tanh"))
    assert inject_fused_llama(geglu) == 1 and geglu.gate_up_proj.epilogue == "gelu_tanh_mul"
    odd = _quantised(_tiny("phi3"))
    odd.gate_up_proj = QuantLinear(4, 64, 128, 96, False)
    assert inject_fused_llama(odd) == 0 and odd.gate_up_proj.epilogue == "none" and "forward" not in odd.__dict__
