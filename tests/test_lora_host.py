"""CPU: LoRA adapters on QuantLinear -- the C ABI (gptq_lora_*: exports, struct layout, the host-only plan and every decline reason), the built code
objects (the lora_* kernels are the four intended instantiations, scratch-free, and the library stays inside its kernel budget), and the module logic of
autogptq_amd/lora.py that needs no kernel (injection, peft-format state dicts, the refusals)."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import autogptq_amd as A  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from autogptq_amd import lora as LR  # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear  # noqa: E402

LORA_SYMBOLS = ("gptq_lora_down", "gptq_lora_up", "gptq_lora_apply", "gptq_describe_lora_plan")


def _lora(K=4096, N=4096, r=16, dtype=_lib.GPTQ_F16, scale=2.0):
    L = _lib.GptqLora()
    L.A = L.B = 0x1000                     # never dereferenced by the host-only queries
    L.K, L.N, L.r, L.dtype, L.scale = K, N, r, dtype, scale
    return L


# ---------------------------------------------------------------- ABI
def test_lora_symbols_exported_and_declared_abi_still_8():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in LORA_SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and hasattr(lib, s), s
    assert "typedef struct gptq_lora_t" in header and "} gptq_lora_t;" in header
    assert lib.gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert "#define GPTQ_MI355X_ABI_VERSION 8" in header


def test_struct_layout_matches_header():
    # 2 pointers, 4 x int32, float, int32 (include/gptq_mi355x.h: gptq_lora_t)
    S = _lib.GptqLora
    assert ctypes.sizeof(S) == 2 * 8 + 4 * 4 + 4 + 4 == 40
    assert [getattr(S, f).offset for f in ("A", "B", "K", "N", "r", "dtype", "scale", "reserved")] == [0, 8, 16, 20, 24, 28, 32, 36]
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    body = header[header.index("typedef struct gptq_lora_t"):header.index("} gptq_lora_t;")]
    order = [body.index(t) for t in ("*A;", "*B;", "int32_t K, N, r, dtype;", "float   scale;", "int32_t reserved;")]
    assert order == sorted(order)
    assert _lib.LORA_MAX == int(re.search(r"#define GPTQ_LORA_MAX (\d+)", header).group(1)) == 4


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("dtype", [_lib.GPTQ_F16, _lib.GPTQ_BF16])
def test_plan_row_regimes(dtype):
    for r in (8, 16, 24, 40, 64):
        for K, N in ((4096, 4096), (4096, 11008), (11008, 4096), (96, 48)):
            for M in range(1, 9):
                d = _lib.describe_lora_plan([_lora(K, N, r, dtype)], M)
                assert d["path"] == "lora" and d["rows"] == "gemv" and d["launches"] == 2, (M, d)
                assert d["wg_down"] == r and d["wg_up"] == -(-N // 64), d                       # a row of A / 64 columns per workgroup
            for M in (9, 16, 17, 64, 2048):
                d = _lib.describe_lora_plan([_lora(K, N, r, dtype)], M)
                assert d["path"] == "lora" and d["rows"] == "mfma" and d["launches"] == 2, (M, d)
                assert d["wg_down"] == -(-r // 16) * -(-M // 16) and d["wg_up"] == -(-N // 256) * -(-M // 16), d
    d0 = _lib.describe_lora_plan([_lora()], 0)
    assert d0["path"] == "lora" and d0["wg_down"] == 0 and d0["wg_up"] == 0, d0


def test_plan_of_a_multi_call_is_the_sum_of_its_adapters():
    group = [_lora(4096, 4096, 64), _lora(4096, 1024, 24), _lora(4096, 1024, 8)]
    for M in (1, 4, 16, 100):
        d = _lib.describe_lora_plan(group, M)
        singles = [_lib.describe_lora_plan([g], M) for g in group]
        assert d["path"] == "lora" and d["wg_down"] == sum(s["wg_down"] for s in singles) and d["wg_up"] == sum(s["wg_up"] for s in singles), d


@pytest.mark.parametrize("kw,n,frag", [
    (dict(r=4), 1, "r = 4"),
    (dict(r=72), 1, "r = 72"),
    (dict(r=12), 1, "r = 12"),
    (dict(dtype=_lib.GPTQ_F32), 1, "fp32"),
    (dict(), 5, "n = 5"),
    (dict(K=4112), 1, "K = 4112"),
    (dict(N=4104), 1, "N = 4104"),
])
def test_plan_declines_with_a_reason(kw, n, frag):
    lib = _lib.load()
    group = [_lora(**kw) for _ in range(n)]
    d = _lib.describe_lora_plan(group, 4)
    assert d["path"] == "none" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
    arr = (ctypes.POINTER(_lib.GptqLora) * n)(*[ctypes.pointer(g) for g in group])
    ptrs = (ctypes.c_void_p * n)(*[0x1000] * n)
    for rc in (lib.gptq_lora_apply(arr, n, 0x1000, ptrs, ptrs, 4, None), lib.gptq_lora_down(arr, n, 0x1000, ptrs, 4, None),
               lib.gptq_lora_up(arr, n, ptrs, ptrs, 4, None)):
        assert rc == 3 and frag in lib.gptq_last_error().decode()          # GPTQ_ERR_UNSUPPORTED, before any launch


def test_misaligned_pointers_and_mixed_groups_decline_and_zero_rows_launch_nothing():
    lib = _lib.load()
    one = _lora()
    arr = (ctypes.POINTER(_lib.GptqLora) * 1)(ctypes.pointer(one))
    good, odd = (ctypes.c_void_p * 1)(0x1000), (ctypes.c_void_p * 1)(0x1008)
    assert lib.gptq_lora_apply(arr, 1, 0x1008, good, good, 4, None) == 3 and "16-byte aligned" in lib.gptq_last_error().decode()
    assert lib.gptq_lora_apply(arr, 1, 0x1000, odd, good, 4, None) == 3 and "u[0]" in lib.gptq_last_error().decode()
    assert lib.gptq_lora_apply(arr, 1, 0x1000, good, odd, 4, None) == 3 and "outs[0]" in lib.gptq_last_error().decode()
    bad = _lora()
    bad.B = 0x1004
    assert _lib.describe_lora_plan([bad], 4)["path"] == "none"
    d = _lib.describe_lora_plan([_lora(K=4096), _lora(K=2048)], 4)
    assert d["path"] == "none" and "share_K_and_dtype" in d["reason"], d
    assert lib.gptq_lora_apply(arr, 1, 0x1000, good, good, 0, None) == 0                   # M = 0: nothing is launched, nothing is dereferenced
    assert lib.gptq_lora_apply(arr, 1, None, good, good, 4, None) == 1                     # GPTQ_ERR_NULL


# ---------------------------------------------------------------- built code objects
def test_lora_kernels_are_the_four_intended_and_scratch_free():
    from test_kernel_resources import _kernels
    ks = _kernels()
    mine = {n: v for n, v in ks.items() if re.search(r"lora_\w*kernel", n)}
    down = sorted(n for n in mine if "lora_down_kernel" in n)
    up = sorted(n for n in mine if "lora_up_kernel" in n)
    assert len(down) == 2 and len(up) == 2 and len(mine) == 4, sorted(mine)               # two kernels x fp16 / bf16: the row regime is a run-time branch
    for n, v in mine.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0), (n, v)
        assert (v["vgpr"] or 0) <= 128 and (v["lds"] or 0) <= 8192, (n, v)
    assert sum(1 for n in ks if re.search(r"\d+pack_weights_kernel", n)) == 1              # the load-time kernel that paid for them: bits at run time
    assert len(ks) <= 1160, len(ks)


# ---------------------------------------------------------------- module logic (no kernel)
class _Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.q_proj = QuantLinear(4, 32, 64, 64, False)
        self.k_proj = QuantLinear(4, 32, 64, 32, False)
        self.o_proj = QuantLinear(4, 32, 64, 64, False)
        self.dense = torch.nn.Linear(64, 64)


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = torch.nn.ModuleList([_Block(), _Block()])
        self.head = torch.nn.Linear(64, 8)


def test_inject_wraps_exactly_the_targets():
    m = _Model()
    before = set(m.state_dict())
    got = A.inject_lora(m, ["q_proj", "k_proj", "dense"], r=8, lora_alpha=16, lora_dropout=0.1)
    assert sorted(got) == ["layers.0.k_proj", "layers.0.q_proj", "layers.1.k_proj", "layers.1.q_proj"]          # `dense` is no QuantLinear
    for name, mod in got.items():
        assert isinstance(mod, A.LoraQuantLinear) and m.get_submodule(name) is mod and isinstance(mod.base, QuantLinear)
        assert mod.lora_A.weight.shape == (8, 64) and mod.lora_B.weight.shape == (mod.base.outfeatures, 8)
        assert mod.lora_A.weight.dtype == torch.float32 and mod.scaling == 2.0 and mod.lora_dropout == 0.1
        assert float(mod.lora_A.weight.detach().abs().max()) > 0 and not bool(mod.lora_B.weight.any())                   # xavier-uniform / zero
    assert isinstance(m.layers[0].o_proj, QuantLinear) and isinstance(m.layers[0].dense, torch.nn.Linear)
    after = set(m.state_dict())
    assert {k.replace("q_proj.", "q_proj.base.").replace("k_proj.", "k_proj.base.") for k in before} <= after      # the base's keys, unchanged underneath
    assert A.inject_lora(m, ["q_proj"], r=8, lora_alpha=16) == {}                                               # nothing is wrapped twice


def test_state_dict_round_trip_in_peft_format():
    torch.manual_seed(0)
    m = _Model()
    got = A.inject_lora(m, ["q_proj", "o_proj"], r=8, lora_alpha=16)
    for mod in got.values():
        with torch.no_grad():
            mod.lora_B.weight.normal_()
    sd = A.lora_state_dict(m)
    assert sorted(sd) == sorted(f"base_model.model.{n}.{w}.weight" for n in got for w in ("lora_A", "lora_B"))
    cfg = {"r": 8, "lora_alpha": 16, "target_modules": ["q_proj", "o_proj"], "lora_dropout": 0.0}
    m2 = _Model()
    loaded = A.load_lora_adapter(m2, sd, cfg)
    assert sorted(loaded) == sorted(got)
    sd2 = A.lora_state_dict(m2)
    assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd)                              # bit for bit
    m3 = _Model()
    A.load_lora_adapter(m3, {k.replace(".weight", ".default.weight"): v for k, v in sd.items()}, cfg)           # peft's in-memory key form
    sd3 = A.lora_state_dict(m3)
    assert all(torch.equal(sd[k], sd3[k]) for k in sd)
    with pytest.raises(KeyError):
        A.load_lora_adapter(_Model(), {k: v for k, v in sd.items() if "lora_B" not in k}, cfg)
    with pytest.raises(KeyError):
        A.load_lora_adapter(_Model(), dict(sd, **{"base_model.model.layers.0.k_proj.lora_A.weight": torch.zeros(8, 64)}), cfg)


def test_merge_raises_and_silu_mul_base_is_refused():
    lq = A.LoraQuantLinear(QuantLinear(4, 32, 64, 64, False), 8, 16)
    for fn in (lq.merge, lq.unmerge):
        with pytest.raises(NotImplementedError, match="gptq model not support merge lora adapter"):
            fn()
    with pytest.raises(ValueError, match="silu_mul"):
        A.LoraQuantLinear(QuantLinear(4, 32, 64, 128, False, epilogue="silu_mul"), 8, 16)
    with pytest.raises(TypeError):
        A.LoraQuantLinear(torch.nn.Linear(64, 64), 8, 16)


def test_mark_only_lora_trainable():
    m = _Model()
    A.inject_lora(m, ["q_proj"], r=8, lora_alpha=16)
    A.mark_only_lora_trainable(m)
    on = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert on == sorted(f"layers.{i}.q_proj.{w}.weight" for i in (0, 1) for w in ("lora_A", "lora_B"))
    assert not m.head.weight.requires_grad and not m.layers[0].dense.weight.requires_grad


def test_kernel_copies_are_refreshed_in_place():
    lq = A.LoraQuantLinear(QuantLinear(4, 32, 64, 64, False), 8, 16)
    with torch.no_grad():
        a16, b16 = lq._kernel_weights(torch.float16)
        assert a16.dtype == torch.float16 and torch.equal(a16, lq.lora_A.weight.half()) and not bool(b16.any())
        lq.lora_B.weight.add_(1.0)                                   # an optimiser-style in-place update
        a2, b2 = lq._kernel_weights(torch.float16)
    assert a2 is a16 and b2 is b16 and b2.data_ptr() == b16.data_ptr() and bool((b16 == 1).all())               # same storage, new values
    assert LR.MERGE_MESSAGE == "gptq model not support merge lora adapter"


def test_autograd_formulas_on_the_composition_path():
    """An fp32 layer is declined by the kernels, so LoraQuantLinear composes the branch in torch -- on the CPU too, with the base product stubbed: the
    Function's backward (dA, dB, dX_lora, dY passed through) against torch autograd of the same expression."""
    torch.manual_seed(0)
    K, N, r = 64, 32, 8
    q = QuantLinear(4, 32, K, N, False, weight_dtype=torch.float32)
    W = torch.randn(K, N)
    q.forward = lambda x: x @ W                                      # stands in for the quantized product (no kernel on the CPU)
    lq = A.LoraQuantLinear(q, r, 16)
    assert not lq.fused_ok()
    with torch.no_grad():
        lq.lora_B.weight.normal_()
    x = torch.randn(3, 5, K, requires_grad=True)
    y = lq(x)
    g = torch.randn_like(y)
    y.backward(g)
    x2 = x.detach().clone().requires_grad_(True)
    a = lq.lora_A.weight.detach().clone().requires_grad_(True)
    b = lq.lora_B.weight.detach().clone().requires_grad_(True)
    y2 = x2 @ W + lq.scaling * ((x2 @ a.t()) @ b.t())
    y2.backward(g)
    assert torch.allclose(y, y2, atol=1e-5)
    for got, want in ((x.grad, x2.grad), (lq.lora_A.weight.grad, a.grad), (lq.lora_B.weight.grad, b.grad)):
        assert torch.allclose(got, want, atol=1e-4, rtol=1e-4)
    with torch.no_grad():
        assert torch.equal(lq(x), y.detach())                        # values under grad == values under no_grad
