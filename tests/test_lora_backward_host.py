"""CPU: the fused LoRA backward -- the C ABI of gptq_lora_backward (exports, struct layout, the host-only plan: slice counts, workspace formula, every
decline reason before any launch), the built code objects (exactly three wgrad kernels, scratch-free, the figures DESIGN.md section 4.9 records, the
library inside its kernel budget) and the module logic of autogptq_amd/lora.py that needs no kernel (the opt-in switch and its fall-back)."""
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
from autogptq_amd.qlinear_mi355x import QuantLinear  # noqa: E402

SYMBOLS = ("gptq_lora_backward_workspace_bytes", "gptq_lora_backward", "gptq_describe_lora_backward_plan")
FIELDS = ("At", "Bt", "u", "dY", "du", "dA", "dB")


def _lora(K=4096, N=4096, r=16, dtype=_lib.GPTQ_F16, scale=2.0):
    L = _lib.GptqLora()
    L.K, L.N, L.r, L.dtype, L.scale = K, N, r, dtype, scale        # A / B stay NULL: the backward reads the transposed copies instead
    return L


def _grad(**kw):
    G = _lib.GptqLoraGrad()
    for f in FIELDS:
        setattr(G, f, kw.get(f, 0x1000))                            # fake pointers: nothing is dereferenced before a launch
    return G


def _arrs(loras, grads):
    return ((ctypes.POINTER(_lib.GptqLora) * len(loras))(*[ctypes.pointer(l) for l in loras]),
            (ctypes.POINTER(_lib.GptqLoraGrad) * len(grads))(*[ctypes.pointer(g) for g in grads]))


def _slices(M, P, Q):
    """The header's formula."""
    steps, blocks = -(-M // 32), -(-max(P, Q) // 64)
    s0 = min(64, max(1, steps // 4), -(-512 // blocks))
    sps = -(-steps // s0)
    return -(-steps // sps), sps


def _a256(v):
    return (v + 255) // 256 * 256


# ---------------------------------------------------------------- ABI
def test_symbols_exported_and_declared_abi_still_8():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and callable(getattr(lib, s)), s
    assert lib.gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert "#define GPTQ_MI355X_ABI_VERSION 8" in header


def test_struct_layout_matches_header():
    S = _lib.GptqLoraGrad
    assert ctypes.sizeof(S) == 7 * 8
    assert [getattr(S, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 48]
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    body = header[header.index("typedef struct gptq_lora_grad_t"):header.index("} gptq_lora_grad_t;")]
    order = [body.index(t) for t in ("*At;", "*Bt;", "*u;", "*dY;", "*du;", "*dA;", "*dB;")]
    assert order == sorted(order) and len(re.findall(r"\*\w+;", body)) == 7


# ---------------------------------------------------------------- the plan
SHAPES = [(4096, 4096, 16), (4096, 11008, 16), (11008, 4096, 64), (96, 96, 24), (352, 512, 40), (256, 64, 8), (64, 64, 64)]
ROWS = [1, 8, 9, 31, 32, 33, 127, 128, 129, 255, 256, 1000, 2048, 2100, 4090, 4096, 8192, 65536, 1 << 20]


@pytest.mark.parametrize("dtype", [_lib.GPTQ_F16, _lib.GPTQ_BF16])
def test_slice_counts_and_workspace_follow_the_documented_function(dtype):
    lib = _lib.load()
    seen = set()
    for K, N, r in SHAPES:
        for M in ROWS:
            L = _lora(K, N, r, dtype)
            d = _lib.describe_lora_backward_plan([L], M)
            sa, spa = _slices(M, r, K)
            sb, spb = _slices(M, N, r)
            assert d["path"] == "lora_backward" and d["S_dA"] == [sa] and d["S_dB"] == [sb], (K, N, r, M, d)
            for s, sps in ((sa, spa), (sb, spb)):
                assert 1 <= s <= 64 and (s - 1) * sps * 32 < M <= s * sps * 32               # whole 32-row steps per slice, none empty
            want = (_a256(4 * sa * r * K) if sa > 1 else 0) + (_a256(4 * sb * N * r) if sb > 1 else 0)
            arr, _ = _arrs([L], [])
            assert d["workspace"] == want == lib.gptq_lora_backward_workspace_bytes(arr, 1, M), (K, N, r, M)
            assert d["wg_wgrad"] == -(-K // 64) * sa + -(-N // 64) * sb
            assert d["wg_sum"] == (-(-r * K // 256) if sa > 1 else 0) + (-(-N * r // 256) if sb > 1 else 0)
            assert d["launches"] == 3 + (1 if max(sa, sb) > 1 else 0)
            seen.add(min(sa, 3))
    assert seen == {1, 2, 3}
    d = _lib.describe_lora_backward_plan([_lora(4096, 11008, 16, dtype)], 4096)               # gate_proj of the 7B shapes
    assert d["S_dA"] == [8] and d["S_dB"] == [3], d
    d0 = _lib.describe_lora_backward_plan([_lora()], 0)
    assert d0["path"] == "lora_backward" and d0["launches"] == 0 and d0["wg_wgrad"] == 0 and d0["workspace"] == 0, d0


def test_plan_does_not_depend_on_the_device():
    """The query before and after gptq_init (which reads the device's properties where there is one): identical strings."""
    lib = _lib.load()
    cases = [([_lora(K, N, r)], M) for K, N, r in SHAPES for M in (1, 129, 1000, 4096)]
    before = [_lib.describe_lora_backward_plan(g, M) for g, M in cases]
    lib.gptq_init()                                                 # no device on a CPU box: an error code, and nothing may change
    assert [_lib.describe_lora_backward_plan(g, M) for g, M in cases] == before


def test_plan_of_a_group_is_the_sum_of_its_adapters():
    group = [_lora(4096, 4096, 64), _lora(4096, 1024, 24), _lora(4096, 1024, 8)]
    lib = _lib.load()
    for M in (1, 8, 9, 100, 1000, 4096):
        d = _lib.describe_lora_backward_plan(group, M)
        singles = [_lib.describe_lora_backward_plan([g], M) for g in group]
        assert d["path"] == "lora_backward", d
        for k in ("wg_down", "wg_wgrad", "wg_sum", "wg_up", "workspace"):
            assert d[k] == sum(s[k] for s in singles), (M, k)
        assert d["S_dA"] == [s["S_dA"][0] for s in singles] and d["S_dB"] == [s["S_dB"][0] for s in singles]
        assert d["launches"] == 2 * 3 + 1 + (1 if max(d["S_dA"] + d["S_dB"]) > 1 else 0)
        arr, _ = _arrs(group, [])
        assert lib.gptq_lora_backward_workspace_bytes(arr, 3, M) == d["workspace"]


@pytest.mark.parametrize("kw,n,frag", [
    (dict(r=4), 1, "r = 4"),
    (dict(r=72), 1, "r = 72"),
    (dict(r=12), 1, "r = 12"),
    (dict(dtype=_lib.GPTQ_F32), 1, "fp32"),
    (dict(), 5, "n = 5"),
    (dict(K=4112), 1, "K = 4112"),
    (dict(N=4112), 1, "N = 4112"),
    (dict(K=96, N=48), 1, "N = 48"),
])
def test_declines_with_a_reason_before_any_launch(kw, n, frag):
    lib = _lib.load()
    group = [_lora(**kw) for _ in range(n)]
    d = _lib.describe_lora_backward_plan(group, 4)
    assert d["path"] == "none" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
    la, ga = _arrs(group, [_grad() for _ in range(n)])
    assert lib.gptq_lora_backward(la, ga, n, 0x1000, 0x1000, 4, None, 0, None) == 3 and frag in lib.gptq_last_error().decode()
    assert lib.gptq_lora_backward_workspace_bytes(la, n, 4096) == 0


def test_the_forward_accepts_n_48_and_the_backward_declines_it():
    L = _lora(96, 48, 8)
    L.A = L.B = 0x1000
    assert _lib.describe_lora_plan([L], 4)["path"] == "lora"
    d = _lib.describe_lora_backward_plan([L], 4)
    assert d["path"] == "none" and "multiple_of_32" in d["reason"], d


def test_mixed_groups_misaligned_null_workspace_and_zero_rows():
    lib = _lib.load()
    d = _lib.describe_lora_backward_plan([_lora(K=4096), _lora(K=2048)], 4)
    assert d["path"] == "none" and "share_K_and_dtype" in d["reason"], d
    d = _lib.describe_lora_backward_plan([_lora(), _lora(dtype=_lib.GPTQ_BF16)], 4)
    assert d["path"] == "none" and "share_K_and_dtype" in d["reason"], d
    one = _lora()
    for f in FIELDS:                                                # every pointer of grads[] ...
        la, ga = _arrs([one], [_grad(**{f: 0x1008})])
        assert lib.gptq_lora_backward(la, ga, 1, 0x1000, 0x1000, 4, None, 0, None) == 3 and "16-byte aligned" in lib.gptq_last_error().decode(), f
    la, ga = _arrs([one], [_grad()])
    assert lib.gptq_lora_backward(la, ga, 1, 0x1008, 0x1000, 4, None, 0, None) == 3                # ... x, dX and the workspace
    assert lib.gptq_lora_backward(la, ga, 1, 0x1000, 0x1008, 4, None, 0, None) == 3
    assert lib.gptq_lora_backward(la, ga, 1, 0x1000, 0x1000, 4, 0x1008, 1 << 30, None) == 3
    for f in ("At", "Bt", "u", "dY", "du"):                         # GPTQ_ERR_NULL; dA / dB / dX NULL mean "skip"
        la1, ga1 = _arrs([one], [_grad(**{f: None})])
        assert lib.gptq_lora_backward(la1, ga1, 1, 0x1000, 0x1000, 4, None, 0, None) == 1, f
    assert lib.gptq_lora_backward(la, ga, 1, None, 0x1000, 4, None, 0, None) == 1
    assert lib.gptq_lora_backward(la, None, 1, 0x1000, 0x1000, 4, None, 0, None) == 1
    assert lib.gptq_lora_backward(None, ga, 1, 0x1000, 0x1000, 4, None, 0, None) == 1
    need = lib.gptq_lora_backward_workspace_bytes(la, 1, 4096)
    assert need > 0
    assert lib.gptq_lora_backward(la, ga, 1, 0x1000, 0x1000, 4096, 0x1000, need - 1, None) == 4    # GPTQ_ERR_WORKSPACE
    assert "workspace too small" in lib.gptq_last_error().decode()
    assert lib.gptq_lora_backward(la, ga, 1, 0x1000, 0x1000, 4096, None, 0, None) == 4
    assert lib.gptq_lora_backward(la, ga, 1, 0x1000, 0x1000, -1, None, 0, None) == 2               # GPTQ_ERR_SHAPE
    assert lib.gptq_lora_backward(la, ga, 1, 0x1000, 0x1000, 0, None, 0, None) == 0                # M = 0: nothing is launched, nothing is dereferenced


# ---------------------------------------------------------------- built code objects
def test_wgrad_kernels_are_the_three_intended_and_scratch_free():
    from test_kernel_resources import _kernels
    ks = _kernels()
    mine = {n: v for n, v in ks.items() if "wgrad" in n}
    assert len(mine) == 3 and all("gptq8adapters" in n for n in mine), sorted(mine)
    main = sorted(n for n in mine if "wgrad_kernel" in n)
    tail = [n for n in mine if "wgrad_sum_kernel" in n]
    assert len(main) == 2 and len(tail) == 1, sorted(mine)                                   # fp16 / bf16; orientation and slices are run-time branches
    for n, v in mine.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0), (n, v)
        assert not re.search(r"lora_\w*kernel", n) and "adapter_rows" not in n, n
    for n in main:                                                                           # the figures of DESIGN.md section 4.9
        assert mine[n]["vgpr"] == 60 and mine[n]["agpr"] == 16 and mine[n]["lds"] == 20480, (n, mine[n])
    assert mine[tail[0]]["vgpr"] == 6 and mine[tail[0]]["lds"] == 0, mine[tail[0]]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "60 VGPRs + 16 AGPRs" in design and "20,480 bytes of LDS" in design
    assert sum(1 for n in ks if re.search(r"lora_\w*kernel", n)) == 4
    assert len(ks) <= 1160, len(ks)


# ---------------------------------------------------------------- module logic without a kernel
def _stub_layer(fused_backward, seed=0):
    torch.manual_seed(seed)
    K, N, r = 64, 32, 8
    q = QuantLinear(4, 32, K, N, False, weight_dtype=torch.float32)
    W = torch.randn(K, N)
    q.forward = lambda x: x @ W                                      # stands in for the quantized product (no kernel on the CPU)
    lq = A.LoraQuantLinear(q, r, 16, fused_backward=fused_backward)
    with torch.no_grad():
        lq.lora_B.weight.normal_()
    return lq


def test_the_switch_defaults_off_and_the_helpers_set_it():
    q = QuantLinear(4, 32, 64, 32, False)
    assert A.LoraQuantLinear(q, 8, 16).fused_backward is False
    assert A.LoraQuantLinear(q, 8, 16, fused_backward=True).fused_backward is True

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj, self.k_proj = QuantLinear(4, 32, 64, 32, False), QuantLinear(4, 32, 64, 32, False)

    off = A.inject_lora(Net(), ["q_proj", "k_proj"], 8, 16)
    assert len(off) == 2 and not any(l.fused_backward for l in off.values())
    net = Net()
    on = A.inject_lora(net, ["q_proj", "k_proj"], 8, 16, fused_backward=True)
    assert len(on) == 2 and all(l.fused_backward for l in on.values())
    A.set_lora_fused_backward(net, False)
    assert not any(l.fused_backward for l in on.values())
    A.set_lora_fused_backward(net)
    assert all(l.fused_backward for l in on.values())
    assert "set_lora_fused_backward" in A.lora.__all__


def test_a_declined_layer_with_the_switch_on_computes_the_switch_off_gradients():
    grads = []
    for flag in (False, True):
        lq = _stub_layer(flag)
        assert not lq.fused_backward_ok()                           # fp32: gptq_lora_backward declines, the torch backward runs
        x = torch.randn(3, 5, 64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
        y = lq(x)
        y.backward(torch.randn(y.shape, generator=torch.Generator().manual_seed(2)))
        grads.append((y.detach(), x.grad, lq.lora_A.weight.grad, lq.lora_B.weight.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)
