"""CPU: the shared expert of Qwen-MoE blocks -- the C ABI (gptq_moe_shared_decode_* / gptq_moe_shared_combine: exports, plan arithmetic, the workspace
formula, one decline per reason) on host-built structs as tests/test_moe_decode_host.py builds them, and inject_shared_expert / remove_shared_expert on the
tiny Qwen2-MoE: the blocks are found, the module keeps its class and state-dict keys, and on CPU tensors the bound forward is the class formula bit for bit."""
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
from test_moe_decode_host import _a256, _layer, _moe  # noqa: E402

SHARED_SYMBOLS = ("gptq_moe_shared_decode_workspace_bytes", "gptq_moe_shared_decode_forward", "gptq_describe_moe_shared_decode_plan",
                  "gptq_moe_shared_combine")


def _shared(H=256, Is=1024, gate_kw=None, up_kw=None, down_kw=None, **kw):
    layers = [_layer(H, Is, **dict(kw, **(gate_kw or {}))), _layer(H, Is, **dict(kw, **(up_kw or {}))), _layer(Is, H, **dict(kw, **(down_kw or {})))]
    sh = _lib.GptqMoeShared()
    sh.gate, sh.up, sh.down = (ctypes.addressof(l) for l in layers)
    sh._keep = layers
    return sh


def test_shared_symbols_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in SHARED_SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and hasattr(lib, s), s
    assert "typedef struct gptq_moe_shared_t" in header
    import autogptq_amd
    for f in ("moe_shared_forward", "inject_shared_expert", "remove_shared_expert"):
        assert callable(getattr(autogptq_amd, f))


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("shape", [(8, 2, 256, 512, 1024, _lib.GPTQ_F16), (60, 4, 2048, 1408, 5632, _lib.GPTQ_BF16)], ids=["e8", "a2.7b"])
def test_plan_accepts_and_counts_the_workgroups(shape, bits, act):
    lib = _lib.load()
    E, topk, H, I, Is, dtype = shape
    m = _moe(E, H, I, bits=bits, dtype=dtype, act=act)
    sh = _shared(H, Is, bits=bits, dtype=dtype, act=act)
    for T in (1, 2, 3, 4):
        d = _lib.describe_moe_shared_decode_plan(m, sh, T, topk)
        base = _lib.describe_moe_decode_plan(m, T, topk)
        assert d["path"] == "decode_shared" and d["launches"] == 2, d
        assert d["wg_pair"] == T * topk * (I // 16) + T * (Is // 16), d
        assert d["wg_down"] == T * (H // 16), d
        assert d["waves_pair"] == base["waves_pair"] and d["waves_down"] >= base["waves_down"], (d, base)
        assert base["lds_pair"] <= d["lds_pair"] <= 160 * 1024 and d["lds_down"] <= 160 * 1024, (d, base)
        got = int(lib.gptq_moe_shared_decode_workspace_bytes(ctypes.byref(m), ctypes.byref(sh), T, topk))
        decode = int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), T, topk))
        assert decode == _lib.WS_HEADER_BYTES + _a256(T * topk * I * 2) + _a256(4 * T * topk)
        assert got == decode + _a256(T * Is * 2) + _a256(4 * T), (T, got)
    d0 = _lib.describe_moe_shared_decode_plan(m, sh, 0, topk)
    assert d0["path"] == "decode_shared" and d0["launches"] == 0, d0
    # T = 0: nothing is launched, nothing is dereferenced
    assert lib.gptq_moe_shared_decode_forward(ctypes.byref(m), ctypes.byref(sh), None, None, None, None, 0, topk, None, None, None, 0, None) == 0
    assert lib.gptq_moe_shared_combine(None, None, None, None, 0, H, dtype, None) == 0


def test_shared_narrower_than_routed_and_other_group_size():
    """I_s < I (one grid row per token, workgroups past I_s / 16 leave) and shared layers with a group size of their own."""
    m = _moe(8, 256, 512, gs=128)
    for gs in (32, 64):
        sh = _shared(256, 320, gs=gs)
        d = _lib.describe_moe_shared_decode_plan(m, sh, 4, 2)
        assert d["path"] == "decode_shared" and d["wg_pair"] == 4 * 2 * 32 + 4 * 20, d


@pytest.mark.parametrize("T,moe_kw,sh_kw,frag", [
    (5, dict(), dict(), "T = 5"),
    (1, dict(), dict(Is=1056), "I_s % 64"),
    (1, dict(), dict(bits=8), "8 bits"),
    (1, dict(), dict(down_kw=dict(bits=8)), "shared down has 8 bits"),
    (1, dict(), dict(dtype=_lib.GPTQ_BF16), "dtype"),
    (1, dict(), dict(up_kw=dict(copy=False)), "shared up carries no decode copy"),
    (1, dict(), dict(gs=48), "group_size"),
])
def test_plan_declines_with_a_reason(T, moe_kw, sh_kw, frag):
    lib = _lib.load()
    m, sh = _moe(**moe_kw), _shared(**sh_kw)
    d = _lib.describe_moe_shared_decode_plan(m, sh, T, 2)
    assert d["path"] == "none" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
    assert int(lib.gptq_moe_shared_decode_workspace_bytes(ctypes.byref(m), ctypes.byref(sh), T, 2)) == 0
    rc = lib.gptq_moe_shared_decode_forward(ctypes.byref(m), ctypes.byref(sh), 0x1000, 0x1000, 0x1000, 0x1000, T, 2, 0x1000, None, 0x1000, 1 << 30, None)
    assert rc == 3 and frag in lib.gptq_last_error().decode()


def test_a_bias_on_a_shared_layer_declines():
    lib = _lib.load()
    m, sh = _moe(), _shared()
    sh._keep[2].bias = 0x7000
    d = _lib.describe_moe_shared_decode_plan(m, sh, 1, 2)
    assert d["path"] == "none" and "shared_down" in d["reason"] and "no_bias" in d["reason"], d
    assert int(lib.gptq_moe_shared_decode_workspace_bytes(ctypes.byref(m), ctypes.byref(sh), 1, 2)) == 0


def test_validation_follows_the_decode_entry_point():
    lib = _lib.load()
    m, sh = _moe(), _shared()
    mp, sp = ctypes.byref(m), ctypes.byref(sh)
    need = int(lib.gptq_moe_shared_decode_workspace_bytes(mp, sp, 1, 2))
    assert lib.gptq_moe_shared_decode_forward(mp, None, 0x1000, 0x1000, 0x1000, 0x1000, 1, 2, 0x1000, None, 0x1000, need, None) == 1          # shared NULL
    assert lib.gptq_moe_shared_decode_forward(mp, sp, 0x1000, None, 0x1000, 0x1000, 1, 2, 0x1000, None, 0x1000, need, None) == 1             # x NULL
    assert lib.gptq_moe_shared_decode_forward(mp, sp, 0x1000, 0x1008, 0x1000, 0x1000, 1, 2, 0x1000, None, 0x1000, need, None) == 3           # x misaligned
    assert lib.gptq_moe_shared_decode_forward(mp, sp, 0x1000, 0x1000, 0x1000, 0x1000, 1, 2, 0x1000, None, 0x1000, need - 1, None) == 4       # workspace
    assert "workspace too small" in lib.gptq_last_error().decode()
    assert lib.gptq_moe_shared_decode_forward(mp, sp, 0x1000, 0x1000, 0x1000, 0x1000, 1, 9, 0x1000, None, 0x1000, need, None) == 3           # topk = 9
    sh.gate_w = 0x1008
    assert lib.gptq_moe_shared_decode_forward(mp, sp, 0x1000, 0x1000, 0x1000, 0x1000, 1, 2, 0x1000, None, 0x1000, need, None) == 3
    assert "gate_w" in lib.gptq_last_error().decode()
    # the combine entry point: dtype, H % 8, null and alignment, before any launch
    assert lib.gptq_moe_shared_combine(0x1000, 0x1000, 0x1000, 0x1000, 1, 256, _lib.GPTQ_F32, None) == 3
    assert lib.gptq_moe_shared_combine(0x1000, 0x1000, 0x1000, 0x1000, 1, 252, _lib.GPTQ_F16, None) == 3
    assert lib.gptq_moe_shared_combine(0x1000, 0x1000, None, 0x1000, 1, 256, _lib.GPTQ_F16, None) == 1
    assert lib.gptq_moe_shared_combine(0x1000, 0x1000, 0x1008, 0x1000, 1, 256, _lib.GPTQ_F16, None) == 3
    assert lib.gptq_moe_shared_combine(0x1000, 0x1000, 0x1000, 0x1000, -1, 256, _lib.GPTQ_F16, None) == 2


def test_the_routed_kernels_stay_eight_and_the_shared_form_is_one_kernel():
    from test_kernel_resources import _kernels
    ks = _kernels()
    assert len({n for n in ks if "moe_decode_kernel" in n}) == 8          # the routed kernels: not re-instantiated for the shared form
    mine = {n: v for n, v in ks.items() if "moe_shared" in n}
    assert len(mine) == 1 and "moe_shared_kernel" in next(iter(mine)), sorted(mine)
    for n, v in mine.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0) and (v["vgpr"] or 0) <= 128, (n, v)      # 16-wave workgroups: 4 waves per SIMD


# ---------------------------------------------------------------------------------------------------------------- the tiny model on the CPU
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    import _tiny_qwen2_moe as TQ
    model, _ = TQ.build(tmp_path_factory.mktemp("qwen2moe"))
    return TQ, model


def _cpu_stand_ins(monkeypatch, TQ):
    """QuantLinear and QuantMoEExperts have no CPU path: give both a deterministic one (the oracle's dequantised weights), so that the block's own formula
    -- what the injected forward must reproduce on CPU tensors -- can run."""
    from oracle import gptq_oracle as O
    from autogptq_amd.moe import QuantMoEExperts
    from autogptq_amd.qlinear_mi355x import QuantLinear
    mode = O.reference_zero_mode(False, TQ.BITS)

    def lin_forward(self, x):
        W = O.dequantize(self.qweight, self.qzeros, self.scales, self.g_idx, TQ.BITS, mode).to(x.dtype)
        return x @ W

    def experts_forward(self, x, idx, w):
        out = torch.zeros_like(x)
        for t in range(x.shape[0]):
            for j in range(idx.shape[1]):
                g, u, d = self[int(idx[t, j])].layers()
                out[t] += w[t, j].to(x.dtype) * d(torch.nn.functional.silu(g(x[t:t + 1])) * u(x[t:t + 1]))[0]
        return out

    monkeypatch.setattr(QuantLinear, "forward", lin_forward)
    monkeypatch.setattr(QuantMoEExperts, "forward", experts_forward)


def test_inject_and_remove_on_the_tiny_model(tiny, monkeypatch):
    TQ, model = tiny
    from autogptq_amd.moe import inject_fused_router, inject_shared_expert, remove_fused_router, remove_shared_expert
    _cpu_stand_ins(monkeypatch, TQ)
    blocks = [layer.mlp for layer in model.model.layers]
    keys = list(model.state_dict().keys())
    x = (torch.rand((1, 5, TQ.H), generator=torch.Generator().manual_seed(3)) - 0.5).half()
    with torch.no_grad():
        ref = [b(x) for b in blocks]
    assert inject_shared_expert(model) == 2
    assert inject_fused_router(model) == 2                          # the block calls self.gate(...) as before: a fused router composes
    try:
        assert all("forward" in b.__dict__ and type(b).__name__ == "Qwen2MoeSparseMoeBlock" for b in blocks)
        assert list(model.state_dict().keys()) == keys
        with torch.no_grad():
            got = [b(x) for b in blocks]
        for b, r, g in zip(blocks, ref, got):
            assert g.shape == r.shape and torch.equal(g, r)
            assert b.experts.last_plan["shared"] == "torch" and "cpu" in b.experts.last_plan["shared_reason"]
        assert inject_shared_expert(model) == 2                     # idempotent
    finally:
        assert remove_fused_router(model) == 2
        assert remove_shared_expert(model) == 2
    assert all("forward" not in b.__dict__ and "_shared_expert_injected" not in b.__dict__ for b in blocks)
    assert list(model.state_dict().keys()) == keys
    with torch.no_grad():
        for b, r in zip(blocks, ref):
            assert torch.equal(b(x), r)
    assert remove_shared_expert(model) == 0


def test_inject_leaves_other_blocks_alone(tiny):
    TQ, model = tiny
    from autogptq_amd.moe import inject_shared_expert, remove_shared_expert
    blk = model.model.layers[0].mlp
    gate = blk.shared_expert_gate
    blk.shared_expert_gate = torch.nn.Linear(TQ.H, 1, bias=True).half()      # a gate with a bias is not the block's formula: not bound
    try:
        assert inject_shared_expert(model) == 1
        assert "forward" not in blk.__dict__
    finally:
        blk.shared_expert_gate = gate
        remove_shared_expert(model)
    assert inject_shared_expert(torch.nn.Sequential(torch.nn.Linear(4, 4))) == 0
