"""CPU (-m "not gpu"): the ungated epilogues 'relu' / 'gelu' / 'gelu_tanh' (gptq_epilogue_t 16 .. 18) -- act(fc1(x) + b) of OPT, GPT-NeoX, Falcon, BLOOM, GPT-J,
CodeGen, StarCoder2 and Phi.  Constructor rules, the C ABI's additions and refusals, plans (the pair form of the decode-copy kernel in split mode at 1 - 4 rows
of a layer with its copy, the in-place activation pass everywhere else), the kernel inventory unchanged (a launch-uniform branch in the 36 pair code objects and
in silu_mul_kernel, no new instantiation), plain_act_name, and inject_fused_act / remove_fused_act on the eight host classes."""
import ctypes

import pytest
import torch
import torch.nn as nn

from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear

NAMES = {"relu": 16, "gelu": 17, "gelu_tanh": 18}


def test_constructor_takes_the_three_names():
    for name, val in NAMES.items():
        q = QuantLinear(4, 64, 256, 96, True, epilogue=name)          # no N % 64 rule: that one belongs to the gated epilogues
        assert q.epilogue == name and q.out_width == 96 == q.outfeatures and _lib.EPILOGUE_ENUM[name] == val
    assert (_lib.EPI_RELU, _lib.EPI_GELU, _lib.EPI_GELU_TANH) == (16, 17, 18)
    with pytest.raises(ValueError, match="epilogue must be") as e:
        QuantLinear(4, 64, 256, 128, False, epilogue="quick_gelu")
    assert all(f"'{n}'" in str(e.value) for n in ("none", "silu_mul", "gelu_tanh_mul", "relu", "gelu", "gelu_tanh"))


def test_wrappers_refuse_the_ungated_epilogues_as_they_refuse_the_gated_ones():
    from autogptq_amd.adapter_bank import LoraBankQuantLinear
    from autogptq_amd.lora import LoraQuantLinear
    from autogptq_amd.qlinear_mi355x import mlp_forward
    from autogptq_amd.fused import fuse_gate_up
    for epi in NAMES:
        q = QuantLinear(4, 64, 256, 128, False, epilogue=epi)
        with pytest.raises(ValueError, match=epi):
            LoraQuantLinear(q, 8, 16.0)
        with pytest.raises(ValueError, match=epi):
            LoraBankQuantLinear(q, 8, 2)
    a, b = QuantLinear(4, 64, 256, 128, False), QuantLinear(4, 64, 256, 128, False)
    with pytest.raises(ValueError, match="act must be"):            # the act= namespace of the MLP callers is the gated one, unchanged
        fuse_gate_up(a, b, act="gelu")
    with pytest.raises(ValueError, match="act must be"):
        mlp_forward(a, b, QuantLinear(4, 64, 128, 256, False), torch.zeros(1, 256), act="relu")


def test_tensor_parallel_wrappers_refuse_the_ungated_epilogues():
    import inspect
    from autogptq_amd import tensor_parallel as TP
    # both constructors test `epilogue != "none"` before they touch a device (the text of the check: the classes need a process group to be built)
    src = inspect.getsource(TP)
    assert src.count('getattr(full, "epilogue", "none") != "none"') == 2


# ---- the C ABI: host-only layer structs, never dereferenced ------------------------------------------------------------------------------------------
def _layer(**kw):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = 4096, 16384, 4, 128, 0, 0
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def _with_copy(L):
    L.qweight_tiled = L.qconst_tiled = 0x2000
    L.tiled_cols = 16
    return L


def _act_order(L):
    L.g_idx = L.qweight_seq = L.perm = 0x1000
    return L


def test_abi_values_and_refusals():
    lib = _lib.load()
    assert lib.gptq_abi_version() == 8
    for epi in (16, 17, 18):
        assert _lib.describe_plan(_layer(epilogue=epi), 1)["epilogue"] == "separate"
        assert _lib.describe_plan(_layer(epilogue=epi, N=96), 1)["epilogue"] == "separate"      # no N % 64 rule
    for epi in (3, 15, 19, -1):
        with pytest.raises(_lib.GptqError, match=f"unknown epilogue {epi}"):
            _lib.describe_plan(_layer(epilogue=epi), 1)
    g, u, d = _layer(N=1408), _layer(N=1408), _layer(K=1408, N=4096)
    for act in (16, 17, 18, 19):
        rc = lib.gptq_mlp_forward_act(ctypes.byref(g), ctypes.byref(u), ctypes.byref(d), act, 0x1000, 0x1000, 1, None, 0, None)
        assert rc == 3 and "act must be" in lib.gptq_last_error().decode(), (act, rc)
    # gptq_gemv / gptq_gemm: no fused form of their own, refused before a launch
    L = _layer(epilogue=16)
    assert lib.gptq_gemv(ctypes.byref(L), 0x1000, 0x1000, 1, None, 0, None, None) == 3 and "no fused epilogue" in lib.gptq_last_error().decode()
    assert lib.gptq_gemm(ctypes.byref(L), 0x1000, 0x1000, 64, None, 0, None, None) == 3 and "no fused epilogue" in lib.gptq_last_error().decode()


def test_a_width_that_is_no_multiple_of_32_is_no_layer():
    """N = 80: every entry point refuses it with or without an epilogue (check_layer: the packed layout holds whole words of 32 / bits columns, and the module's
    constructor says the same), so there is no such layer for the separate pass to serve."""
    for epi in (0, 16):
        with pytest.raises(_lib.GptqError, match="multiples of 32"):
            _lib.describe_plan(_layer(epilogue=epi, N=80), 2)
    with pytest.raises(ValueError, match="divisible by 32"):
        QuantLinear(4, 32, 160, 80, True, epilogue="relu")


SHAPES = [dict(), dict(bits=3, group_size=32), dict(bits=8, group_size=32), dict(dtype=1)]
SHAPE_IDS = ["int4-fp16", "int3", "int8", "bf16"]


@pytest.mark.parametrize("epi", [16, 17, 18])
@pytest.mark.parametrize("kw", SHAPES, ids=SHAPE_IDS)
def test_decode_rows_of_a_layer_with_its_copy_plan_the_pair_form(kw, epi):
    lib = _lib.load()
    for M in (1, 2, 3, 4):
        L = _with_copy(_layer(epilogue=epi, **kw))
        d = _lib.describe_plan(L, M)
        assert (d["path"], d["kernel"], int(d["pair"]), d["epilogue"], int(d["ksplit"])) == ("gemv", "strips", 1, "fused", 1), (M, d)
        assert int(d["strips"]) == L.N // 32 and int(d["mt"]) == (M if M <= 2 else 4)
        assert lib.gptq_workspace_bytes(ctypes.byref(L), M) == 0                                  # one launch, no scratch
        g = _lib.describe_plan(_with_copy(_layer(epilogue=1, **kw)), M)                            # the geometry of the gated layer of the same tensors
        assert {k: d[k] for k in ("waves", "u", "mt", "strips")} == {k: g[k] for k in ("waves", "u", "mt", "strips")}


def _separate_cases():
    yield "rows5", lambda e: _with_copy(_layer(epilogue=e)), (5, 8, 64)
    yield "int3-rows", lambda e: _with_copy(_layer(epilogue=e, bits=3, group_size=32)), (5, 8, 64)
    yield "int8-rows", lambda e: _with_copy(_layer(epilogue=e, bits=8, group_size=32)), (5, 8, 64)
    yield "bf16-rows", lambda e: _with_copy(_layer(epilogue=e, dtype=1)), (5, 8, 64)
    yield "act-order", lambda e: _act_order(_with_copy(_layer(epilogue=e))), (1, 4, 8)
    yield "int2", lambda e: _with_copy(_layer(epilogue=e, bits=2)), (1, 4, 8)
    yield "fp32", lambda e: _layer(epilogue=e, dtype=2), (1, 4, 8, 64)
    yield "no-copy", lambda e: _layer(epilogue=e), (1, 2, 4, 8, 64)
    yield "no-copy-int3", lambda e: _layer(epilogue=e, bits=3, group_size=32), (1, 4, 64)
    yield "no-copy-bf16", lambda e: _layer(epilogue=e, dtype=1), (1, 4, 64)


@pytest.mark.parametrize("epi", [16, 17, 18])
@pytest.mark.parametrize("name,make,rows", list(_separate_cases()), ids=[c[0] for c in _separate_cases()])
def test_everything_else_plans_the_separate_pass_on_the_plan_of_the_plain_layer(name, make, rows, epi):
    """The pass runs in place on `out`: nothing is staged, so the plan (but for its epilogue word) and every workspace query equal those of the same layer
    with epilogue NONE."""
    lib = _lib.load()
    for M in rows:
        L, P = make(epi), make(0)
        d, p = _lib.describe_plan(L, M), _lib.describe_plan(P, M)
        assert d["epilogue"] == "separate" and p["epilogue"] == "none" and int(d.get("pair", 0)) == 0, (name, M, d)
        assert {k: v for k, v in d.items() if k != "epilogue"} == {k: v for k, v in p.items() if k != "epilogue"}, (name, M, d, p)
        assert lib.gptq_workspace_bytes(ctypes.byref(L), M) == lib.gptq_workspace_bytes(ctypes.byref(P), M), (name, M)
    assert lib.gptq_workspace_bytes_max(ctypes.byref(make(epi)), 64) == lib.gptq_workspace_bytes_max(ctypes.byref(make(0)), 64)


def test_the_decode_copy_of_an_ungated_layer_is_the_copy_of_the_plain_layer():
    lib = _lib.load()
    for mk in (lambda e: _layer(epilogue=e), lambda e: _act_order(_layer(epilogue=e)), lambda e: _layer(epilogue=e, bits=2), lambda e: _layer(epilogue=e, N=96),
               lambda e: _layer(epilogue=e, dtype=2)):
        ans = []
        for epi in (0, 16, 17, 18):
            tb, cb = ctypes.c_size_t(0), ctypes.c_size_t(0)
            L = mk(epi)
            ans.append((lib.gptq_prepack_decode_bytes(ctypes.byref(L), ctypes.byref(tb), ctypes.byref(cb)), tb.value, cb.value))
        assert len(set(ans)) == 1, ans


def test_groups_run_an_ungated_layer_as_a_single_call():
    """gptq_forward_multi: a group with such a layer fits no one-launch kernel -- its workspace is the largest single-call need (the one-by-one route)."""
    lib = _lib.load()
    a, b = _with_copy(_layer(N=4096)), _with_copy(_layer(N=4096, epilogue=16))
    for pair in ((a, b), (b, a)):
        arr = (ctypes.POINTER(_lib.GptqLayer) * 2)(*[ctypes.pointer(l) for l in pair])
        for M in (1, 4, 8):
            assert lib.gptq_workspace_bytes_multi(arr, 2, M) == max(lib.gptq_workspace_bytes(ctypes.byref(l), M) for l in pair)


def test_a_launch_uniform_branch_and_no_new_code_object():
    from test_kernel_resources import _kernels
    ks = _kernels()                                         # skips where the LLVM tools or the library are missing
    one = [n for n in ks if "silu_mul_kernel" in n]
    assert len(one) == 1 and one[0].endswith("EPKvPviiii") and not ks[one[0]]["scratch"] and not ks[one[0]]["spill"]
    assert len([n for n in ks if "silu_mul2_kernel" in n]) == 1
    tiled = {n: v for n, v in ks.items() if "gemv_tiled_kernel" in n}
    assert len(tiled) == 248, len(tiled)
    pair = {n: v for n, v in tiled.items() if "ELi4ELi0EEEvNS_11TiledParamsE" in n}              # XM = 4
    assert len(pair) == 36
    assert all(v["vgpr"] <= 128 and not v["spill"] and not v["scratch"] for v in pair.values()), {n: v for n, v in pair.items() if v["vgpr"] > 128 or v["spill"] or v["scratch"]}
    assert len(ks) <= 1160, len(ks)
    assert not any((v["scratch"] or v["spill"]) and "gemm_wide_kernel" not in n for n, v in ks.items())      # test_kernel_resources' own exception


# ---- activation names --------------------------------------------------------------------------------------------------------------------------------------
def _gelu_tanh64(g):
    return torch.nn.functional.gelu(g, approximate="tanh")


def test_plain_act_name_over_the_host_models_activations():
    """Every ACT2FN key and the nn modules.  A tanh name is mapped only where the module IS the epilogue's function in fp64 (1e-15 over [-6, 6], the check the
    gated callers' test makes for gelu_new).  BloomGelu and FastGELUActivation write the same expression with sqrt(2/pi) cut to 0.79788456 / 0.7978845608;
    measured here in fp64 over [-6, 6]: up to 2.6e-10 / 9.1e-13 away from tanh-GELU (printed below), a different constant and not a rounding, so they miss the
    1e-15 criterion and are left alone (None) -- a BLOOM MLP keeps its own activation kernel."""
    from transformers.activations import ACT2FN
    from autogptq_amd.fused import plain_act_name
    want = {"relu": "relu", "gelu": "gelu", "gelu_python": "gelu", "gelu_new": "gelu_tanh", "gelu_pytorch_tanh": "gelu_tanh", "gelu_python_tanh": "gelu_tanh"}
    got = {k: plain_act_name(ACT2FN[k]) for k in ACT2FN.keys()}
    assert {k: v for k, v in got.items() if v is not None} == {k: v for k, v in want.items() if k in got}, got
    for k in ("quick_gelu", "relu2", "relu6", "gelu_10", "gelu_fast", "gelu_accurate", "silu", "swish", "tanh", "linear"):
        assert k not in got or got[k] is None, k
    assert [plain_act_name(f) for f in (nn.ReLU(), nn.GELU(), nn.GELU(approximate="tanh"), nn.SiLU(), nn.ReLU6(), nn.Tanh(), None, torch.relu)] == \
        ["relu", "gelu", "gelu_tanh", None, None, None, None, None]
    g = torch.linspace(-6, 6, 1001, dtype=torch.float64)
    for k, v in got.items():
        if v == "gelu_tanh":
            assert float((ACT2FN[k](g) - _gelu_tanh64(g)).abs().max()) <= 1e-15, k
        if v == "gelu":
            assert float((ACT2FN[k](g) - torch.nn.functional.gelu(g)).abs().max()) <= 1e-15, k
        if v == "relu":
            assert torch.equal(ACT2FN[k](g), g.clamp_min(0))
    from transformers.models.bloom.modeling_bloom import BloomGelu
    for name, fn in (("BloomGelu", BloomGelu()), ("FastGELUActivation", ACT2FN["gelu_fast"])):
        diff = float((fn(g) - _gelu_tanh64(g)).abs().max())
        print(f"{name}: max |f(g) - gelu_tanh(g)| in fp64 over [-6, 6] = {diff:.3e}")
        assert diff > 1e-15 and plain_act_name(fn) is None, (name, diff)
        assert diff < 2.0 ** -24                            # (the same function to fp32: what keeps it a candidate, not what the criterion asks)


# ---- injection on the host models' own modules (CPU: nothing is initialised, nothing runs) ---------------------------------------------------------------
def _quantised(mod):
    from autogptq_amd.model_utils import find_layers, make_quant
    make_quant(mod, list(find_layers(mod)), 4, 64)
    return mod


def _site(kind, **kw):
    """(module of the class, first linear's attribute, activation attribute, expected epilogue) -- built tiny from the class's own config."""
    if kind == "opt":
        from transformers import OPTConfig
        from transformers.models.opt.modeling_opt import OPTDecoderLayer
        return OPTDecoderLayer(OPTConfig(hidden_size=128, ffn_dim=256, num_attention_heads=4, num_hidden_layers=1, word_embed_proj_dim=128, **kw)), "fc1", "activation_fn", "relu"
    if kind == "neox":
        from transformers import GPTNeoXConfig
        from transformers.models.gpt_neox.modeling_gpt_neox import GPTNeoXMLP
        return GPTNeoXMLP(GPTNeoXConfig(hidden_size=128, intermediate_size=256, num_attention_heads=4, **kw)), "dense_h_to_4h", "act", "gelu"
    if kind == "falcon":
        from transformers import FalconConfig
        from transformers.models.falcon.modeling_falcon import FalconMLP
        return FalconMLP(FalconConfig(hidden_size=128, num_attention_heads=4, **kw)), "dense_h_to_4h", "act", "gelu"
    if kind == "bloom":
        from transformers import BloomConfig
        from transformers.models.bloom.modeling_bloom import BloomMLP
        return BloomMLP(BloomConfig(hidden_size=128, n_head=4, **kw)), "dense_h_to_4h", "gelu_impl", None       # BloomGelu: not mapped (above)
    if kind == "gptj":
        from transformers import GPTJConfig
        from transformers.models.gptj.modeling_gptj import GPTJMLP
        return GPTJMLP(256, GPTJConfig(n_embd=128, n_head=4, rotary_dim=16, **kw)), "fc_in", "act", "gelu_tanh"
    if kind == "codegen":
        from transformers import CodeGenConfig
        from transformers.models.codegen.modeling_codegen import CodeGenMLP
        return CodeGenMLP(256, CodeGenConfig(n_embd=128, n_head=4, rotary_dim=16, **kw)), "fc_in", "act", "gelu_tanh"
    if kind == "starcoder2":
        from transformers import Starcoder2Config
        from transformers.models.starcoder2.modeling_starcoder2 import Starcoder2MLP
        return Starcoder2MLP(Starcoder2Config(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=4, **kw)), "c_fc", "act", "gelu_tanh"
    from transformers import PhiConfig
    from transformers.models.phi.modeling_phi import PhiMLP
    return PhiMLP(PhiConfig(hidden_size=128, intermediate_size=256, num_attention_heads=4, **kw)), "fc1", "activation_fn", "gelu_tanh"


@pytest.mark.parametrize("kind", ["opt", "neox", "falcon", "bloom", "gptj", "codegen", "starcoder2", "phi"])
def test_inject_fused_act_on_the_host_classes(kind):
    from autogptq_amd.fused import PLAIN_ACT_SITES, inject_fused_act, plain_act_name, remove_fused_act
    mod, lin_name, act_name, want = _site(kind)
    assert PLAIN_ACT_SITES[type(mod).__name__] == (lin_name, act_name)
    mod = _quantised(mod)
    lin, fn = getattr(mod, lin_name), getattr(mod, act_name)
    assert isinstance(lin, QuantLinear) and lin.epilogue == "none" and plain_act_name(fn) == want
    sd = mod.state_dict()
    keys, ptrs = list(sd), {k: v.data_ptr() for k, v in sd.items()}
    if want is None:                                        # an activation that is not served: the module is left alone
        assert inject_fused_act(mod) == 0 and getattr(mod, act_name) is fn and lin.epilogue == "none" and "_fused_act_undo" not in mod.__dict__
        return
    assert inject_fused_act(mod) == 1
    assert getattr(mod, lin_name) is lin and (lin.epilogue, lin.out_width) == (want, lin.outfeatures)
    assert isinstance(getattr(mod, act_name), nn.Identity)
    assert mod.__dict__["_fused_act_undo"] is fn
    sd2 = mod.state_dict()
    assert list(sd2) == keys and {k: v.data_ptr() for k, v in sd2.items()} == ptrs          # no tensor copied or renamed
    assert "forward" not in mod.__dict__                                                     # the host forward is untouched
    assert inject_fused_act(mod) == 0                                                        # not counted twice
    assert remove_fused_act(mod) == 1
    assert getattr(mod, act_name) is fn and lin.epilogue == "none" and "_fused_act_undo" not in mod.__dict__
    assert list(mod.state_dict()) == keys and [n for n, _ in mod.named_modules()] == [n for n, _ in _quantised(_site(kind)[0]).named_modules()]
    assert remove_fused_act(mod) == 0


def test_inject_fused_act_leaves_everything_else_alone():
    from transformers import GemmaConfig, LlamaConfig, Phi3Config
    from transformers.models.gemma.modeling_gemma import GemmaMLP
    from transformers.models.llama.modeling_llama import LlamaMLP
    from transformers.models.phi3.modeling_phi3 import Phi3MLP
    from autogptq_amd.fused import inject_fused_act, inject_fused_llama
    for mlp in (GemmaMLP(GemmaConfig(hidden_size=128, intermediate_size=256)), LlamaMLP(LlamaConfig(hidden_size=128, intermediate_size=256))):
        mlp = _quantised(mlp)
        assert inject_fused_act(mlp) == 0 and all(m.epilogue == "none" for m in mlp.modules() if isinstance(m, QuantLinear))
    # a served class whose activation is not (quick GELU), whose linear is not quantised, or already carries an epilogue
    mod, lin_name, act_name, _ = _site("neox", hidden_act="quick_gelu")
    assert inject_fused_act(_quantised(mod)) == 0 and type(getattr(mod, act_name)).__name__ == "QuickGELUActivation"
    mod = _site("neox")[0]
    assert inject_fused_act(mod) == 0 and isinstance(mod.dense_h_to_4h, nn.Linear)
    mod = _quantised(_site("phi")[0])
    mod.fc1.epilogue = "relu"
    assert inject_fused_act(mod) == 0 and mod.fc1.epilogue == "relu"
    # inject_fused_llama's behaviour on erf-GELU gate_up_proj modules is what it was
    phi3 = _quantised(Phi3MLP(Phi3Config(hidden_size=128, intermediate_size=256, hidden_act="gelu")))
    assert inject_fused_llama(phi3) == 0 and phi3.gate_up_proj.epilogue == "none" and "forward" not in phi3.__dict__
    assert inject_fused_act(phi3) == 0


def test_set_epilogue_on_a_layer_that_was_never_initialised_touches_nothing():
    from autogptq_amd.fused import _set_epilogue
    q = QuantLinear(4, 64, 256, 128, True)
    ptrs = {k: v.data_ptr() for k, v in q.state_dict().items()}
    for name in ("relu", "gelu", "gelu_tanh", "none"):
        _set_epilogue(q, name)
        assert q.epilogue == name and q._layer is None and q.out_width == 128
    assert {k: v.data_ptr() for k, v in q.state_dict().items()} == ptrs
