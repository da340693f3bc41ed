"""CPU: the grouped-sigmoid router of DeepSeek-V3 / GLM-4 MoE blocks -- the C ABI (gptq_moe_router_grouped / gptq_describe_moe_router_grouped_plan: exports,
the plan string of either row regime, every decline reason before a launch, the pointer checks), the built code objects (still one router kernel per dtype,
scratch-free) and the module logic of autogptq_amd/moe.py that needs no kernel: moe_route_grouped's composition against transformers' DeepseekV3TopkRouter,
inject_fused_router / inject_shared_expert and their removal on a tiny DeepSeek-V3, and the ungated form of moe_shared_forward."""
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
from autogptq_amd import moe as M  # noqa: E402

GROUPED_SYMBOLS = ("gptq_moe_router_grouped", "gptq_describe_moe_router_grouped_plan")
P = 0x1000                                   # never dereferenced: every call below returns before a launch
UNSUPPORTED, NULL, SHAPE = 3, 1, 2
PLAN_SHAPES = [(16, 4, 2, 4, 256), (256, 8, 4, 8, 512), (64, 1, 1, 6, 320)]      # (E, G, kg, topk, H)


def _call(x=P, w=P, bias=P, T=4, H=256, E=16, topk=4, G=4, kg=2, scale=1.0, dtype=_lib.GPTQ_F16, flags=0, logits=P, scores=P, idx=P, wts=P):
    return _lib.load().gptq_moe_router_grouped(x, w, bias, T, H, E, topk, G, kg, scale, dtype, flags, logits, scores, idx, wts, None)


# ---------------------------------------------------------------- ABI
def test_grouped_router_symbols_exported_and_declared_abi_still_8():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in GROUPED_SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and hasattr(lib, s), s
    assert declared == set(_lib.EXPORTS)
    assert lib.gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert "#define GPTQ_MI355X_ABI_VERSION 8" in header
    assert A.moe_route_grouped is M.moe_route_grouped and A.router_grouped_plan is M.router_grouped_plan
    assert "moe_route_grouped" in M.__all__ and "router_grouped_plan" in M.__all__


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("dtype", [_lib.GPTQ_F16, _lib.GPTQ_BF16])
def test_plan_string_of_either_regime(dtype):
    lib = _lib.load()
    for E, G, kg, topk, H in PLAN_SHAPES:
        for flags in (0, _lib.ROUTER_RENORM):
            for T in range(1, 9):
                d = _lib.describe_moe_router_grouped_plan(T, H, E, topk, G, kg, dtype, flags)
                assert d == {"path": "router_grouped", "form": "rows", "wg": T, "waves": 8, "lds": 2 * H + (4 * E + 15) // 16 * 16, "groups": G,
                             "launches": 1}, (T, d)
            for T in (9, 16, 17, 64, 300, 2048):
                d = _lib.describe_moe_router_grouped_plan(T, H, E, topk, G, kg, dtype, flags)
                tiles = -(-E // 16)
                assert d == {"path": "router_grouped", "form": "tiles", "wg": -(-T // 16), "waves": 8, "lds": 32768 + 16 * 16 * tiles * 4, "groups": G,
                             "launches": 1}, (T, d)
                assert d["lds"] <= 65536
                # the grouped form runs in the softmax form's launch geometry
                s = _lib.describe_moe_router_plan(T, H, E, topk, dtype, flags)
                assert (s["form"], s["wg"], s["lds"]) == (d["form"], d["wg"], d["lds"])
    buf = ctypes.create_string_buffer(256)
    assert lib.gptq_describe_moe_router_grouped_plan(4, 256, 16, 4, 4, 2, dtype, 1, buf, len(buf)) == 0
    assert buf.value.decode() == "path=router_grouped form=rows wg=4 waves=8 lds=576 groups=4 launches=1"
    assert lib.gptq_describe_moe_router_grouped_plan(17, 512, 256, 8, 8, 4, dtype, 0, buf, len(buf)) == 0
    assert buf.value.decode() == "path=router_grouped form=tiles wg=2 waves=8 lds=49152 groups=8 launches=1"
    assert lib.gptq_describe_moe_router_grouped_plan(4, 256, 16, 4, 4, 2, dtype, 0, None, 0) == NULL
    d0 = _lib.describe_moe_router_grouped_plan(0, 256, 16, 4, 4, 2, dtype)
    assert d0["path"] == "router_grouped" and d0["wg"] == 0, d0
    # the limits themselves are taken
    assert _lib.describe_moe_router_grouped_plan(1, 64, 64, 8, 32, 32, dtype)["path"] == "router_grouped"      # G = 32, Eg = 2
    assert _lib.describe_moe_router_grouped_plan(1, 64, 4, 2, 2, 1, dtype)["path"] == "router_grouped"         # topk = kg Eg


@pytest.mark.parametrize("kw,frag", [
    (dict(dtype=_lib.GPTQ_F32), "fp32"),
    (dict(E=0), "E = 0"),
    (dict(E=257, G=1, kg=1), "E = 257"),
    (dict(topk=0), "topk = 0"),
    (dict(topk=9, E=64), "topk = 9"),
    (dict(H=96), "H = 96"),
    (dict(flags=2), "flags"),
    (dict(E=18), "not a multiple of n_group"),
    (dict(kg=5), "topk_group = 5"),
    (dict(kg=0), "topk_group = 0"),
    (dict(G=33, kg=1, E=66), "n_group = 33"),
    (dict(G=0), "n_group = 0"),
    (dict(E=4, topk=1), "E / n_group = 1"),
    (dict(topk=8, kg=1), "topk = 8 is more than the 4 experts"),
])
def test_every_decline_has_a_reason_and_launches_nothing(kw, frag):
    lib = _lib.load()
    full = dict(T=4, H=256, E=16, topk=4, G=4, kg=2, dtype=_lib.GPTQ_F16, flags=0)
    full.update(kw)
    for T in (4, 17, 0):
        full["T"] = T
        d = _lib.describe_moe_router_grouped_plan(full["T"], full["H"], full["E"], full["topk"], full["G"], full["kg"], full["dtype"], full["flags"])
        assert d["path"] == "none" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
        assert _call(**full) == UNSUPPORTED and frag in lib.gptq_last_error().decode()


@pytest.mark.parametrize("scale", [float("nan"), float("inf"), float("-inf")])
def test_a_scale_that_is_not_finite_declines(scale):
    lib = _lib.load()
    for T in (4, 17, 0):
        assert _call(T=T, scale=scale) == UNSUPPORTED and "scale must be finite" in lib.gptq_last_error().decode()
    assert _call(T=0, scale=2.5) == 0


@pytest.mark.parametrize("name", ["x", "w", "logits", "scores", "idx", "wts"])
def test_misaligned_pointers_decline(name):
    lib = _lib.load()
    assert _call(**{name: P + 8}) == UNSUPPORTED and "16-byte aligned" in lib.gptq_last_error().decode()
    assert _call(**{name: P + 4, "T": 17}) == UNSUPPORTED and "16-byte aligned" in lib.gptq_last_error().decode()


def test_bias_alignment_null_checks_and_zero_tokens():
    lib = _lib.load()
    assert _call(bias=P + 2) == UNSUPPORTED and "bias must be 4-byte aligned" in lib.gptq_last_error().decode()
    assert _call(bias=P + 4, T=0) == 0                                  # 4 bytes are enough for the bias
    for name in ("x", "w", "idx", "wts"):
        assert _call(**{name: None}) == NULL and "non-NULL" in lib.gptq_last_error().decode(), name
    assert _call(T=0) == 0 and _call(T=0, logits=None, scores=None, bias=None) == 0      # T = 0: nothing is launched, nothing is dereferenced
    assert _call(T=-1) == SHAPE
    assert _call(T=0, H=96) == UNSUPPORTED                              # ... but the call is still validated


def test_python_plan():
    assert M.router_grouped_plan(4, 256, 16, 4, 4, 2, torch.float16)["form"] == "rows"
    assert M.router_grouped_plan(9, 256, 16, 4, 4, 2, torch.bfloat16)["form"] == "tiles"
    d = M.router_grouped_plan(4, 256, 16, 4, 4, 2, torch.float32)
    assert d["path"] == "none" and "fp32" in d["reason"], d
    assert M.router_grouped_plan(4, 256, 16, 4, 4, 2, torch.float64)["path"] == "none"
    d = M.router_grouped_plan(4, 256, 16, 4, 8, 2, torch.float16)                            # Eg = 2: topk = kg Eg = 4 is the most it takes
    assert d["path"] == "router_grouped" and d["groups"] == 8 and d["reason"] == "", d
    d = M.router_grouped_plan(4, 256, 16, 5, 8, 2, torch.float16)
    assert d["path"] == "none" and "topk   5 is more than the 4 experts" in d["reason"], d
    # the one region declined for speed (profiles/moe_router_grouped_ab.log): DeepSeek-V3's router in the tiles form up to 64 tokens
    for T, path in ((8, "router_grouped"), (9, "none"), (64, "none"), (65, "router_grouped"), (512, "router_grouped")):
        d = M.router_grouped_plan(T, 7168, 256, 8, 8, 4, torch.float16)
        assert d["path"] == path and (path != "none" or "measured slower" in d["reason"]), (T, d)
    assert M.router_grouped_plan(16, 4096, 128, 8, 1, 1, torch.float16)["path"] == "router_grouped"
    assert _lib.describe_moe_router_grouped_plan(16, 7168, 256, 8, 8, 4, _lib.GPTQ_F16)["path"] == "router_grouped"      # the C plan says what the kernel takes
    # the softmax plan's strings are what they were
    assert M.router_plan(4, 256, 8, 2, torch.float16) == {"path": "router", "form": "rows", "wg": 4, "waves": 8, "lds": 544, "launches": 1, "reason": ""}


# ---------------------------------------------------------------- built code objects
def test_router_kernels_are_still_one_per_dtype_and_scratch_free():
    """The grouped form is a launch-uniform mode of the two router kernels: no kernel is added."""
    from test_kernel_resources import _kernels
    ks = _kernels()
    mine = {n: v for n, v in ks.items() if "moe_router_kernel" in n or "moe_route_grouped" in n}
    assert len(mine) == 2 and all("moe_router_kernel" in n for n in mine), sorted(mine)
    for n, v in mine.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0), (n, v)
        assert (v["vgpr"] or 0) <= 256 and (v["lds"] or 0) == 0, (n, v)
    assert len(ks) <= 1160, len(ks)


# ---------------------------------------------------------------- the composition against transformers' module
@pytest.fixture(scope="module")
def tiny():
    pytest.importorskip("transformers")
    import _tiny_deepseek_v3 as TD
    model = TD.fresh_model(0).float()
    ids = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(3))
    return TD, model, ids


def test_cpu_composition_equals_the_transformers_router(tiny):
    TD, model, _ = tiny
    from transformers.models.deepseek_v3.modeling_deepseek_v3 import DeepseekV3TopkRouter
    torch.manual_seed(5)
    for norm, scale in ((True, 2.5), (False, 1.0)):
        cfg = TD.tiny_config()
        cfg.norm_topk_prob, cfg.routed_scaling_factor = norm, scale
        r = DeepseekV3TopkRouter(cfg)
        r.weight.data.normal_(0, 0.05)
        r.e_score_correction_bias.data.normal_(0, 0.05)
        for dtype in (torch.float32, torch.float16):
            r = r.to(dtype)
            x = torch.randn((11, TD.H), generator=torch.Generator().manual_seed(1)).to(dtype)
            with torch.no_grad():
                ref = r(x)
                got = M.moe_route_grouped(x, r.weight, r.e_score_correction_bias, r.top_k, r.num_group, r.topk_group, renorm=norm, scale=scale)
            assert M.last_route_plan == {"path": "none", "reason": "cpu tensors"}
            assert len(got) == 3 and got[0].dtype == torch.float32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
            for a, b in zip(ref, got):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    assert M.moe_route_grouped(x, r.weight, None, 4, 4, 2, return_logits=False)[0] is None
    # router training keeps autograd
    wp = r.weight.detach().float().clone().requires_grad_(True)
    _, val, _ = M.moe_route_grouped(x.float(), wp, r.e_score_correction_bias.float(), 4, 4, 2, renorm=False)
    val.sum().backward()
    assert wp.grad is not None and torch.isfinite(wp.grad).all() and wp.grad.abs().sum() > 0


def test_bias_copy_is_cached_per_version():
    b = torch.randn(16).half()
    c1 = M._bias_f32(b)
    assert c1.dtype == torch.float32 and torch.equal(c1, b.float()) and M._bias_f32(b) is c1      # nothing is cast per call
    b.add_(1)                                                                                       # an in-place update is seen
    c2 = M._bias_f32(b)
    assert c2 is not c1 and torch.equal(c2, b.float())
    f = torch.randn(16)
    assert M._bias_f32(f) is f


# ---------------------------------------------------------------- injection on the tiny DeepSeek-V3 (CPU: the composition)
def _router_io(model, TD, ids):
    seen = []
    hooks = [b.gate.register_forward_hook(lambda m, args, out: seen.append((args[0].clone(), tuple(o.clone() for o in out)))) for b in TD.moe_blocks(model)]
    with torch.no_grad():
        res = model(ids)
    for h in hooks:
        h.remove()
    return seen, res


def test_inject_fused_router_on_tiny_deepseek_keeps_classes_keys_and_outputs(tiny):
    TD, model, ids = tiny
    n = len(TD.moe_blocks(model))
    assert n == 1
    classes = [type(m) for m in model.modules()]
    keys = list(model.state_dict().keys())
    before, res0 = _router_io(model, TD, ids)
    try:
        assert M.inject_fused_router(model) == n
        assert [type(m) for m in model.modules()] == classes and list(model.state_dict().keys()) == keys
        for b in TD.moe_blocks(model):
            g = b.gate
            assert type(g).__name__ == "DeepseekV3TopkRouter" and g.__dict__["_fused_router_kind"] == "grouped" and g.forward.__func__ is M._fused_router_forward
        after, res1 = _router_io(model, TD, ids)
        assert len(after) == len(before) == n
        for (xi, outs0), (xj, outs1) in zip(before, after):
            assert torch.equal(xi, xj) and len(outs1) == 3
            for a, b in zip(outs0, outs1):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
        assert torch.equal(res0.logits, res1.logits)
        assert M.inject_fused_router(model) == n                       # idempotent
    finally:
        removed = M.remove_fused_router(model)
    assert removed == n and M.remove_fused_router(model) == 0
    for b in TD.moe_blocks(model):
        assert "forward" not in b.gate.__dict__ and b.gate.forward.__func__ is type(b.gate).forward
    again, _ = _router_io(model, TD, ids)
    for (_, outs0), (_, outs2) in zip(before, again):
        assert all(torch.equal(a, b) for a, b in zip(outs0, outs2))


def test_a_grouped_router_without_its_attributes_is_left_alone():
    class DeepseekV3TopkRouter(torch.nn.Module):                       # the class name alone is not enough
        def __init__(self):
            super().__init__()
            self.top_k, self.num_experts = 2, 8
            self.weight = torch.nn.Parameter(torch.zeros(8, 64))

    class Glm4MoeTopkRouter(DeepseekV3TopkRouter):                     # ... the full attribute set under the config's spelling (n_group) is
        def __init__(self):
            super().__init__()
            self.n_group, self.topk_group, self.norm_topk_prob, self.routed_scaling_factor = 2, 1, True, 1.5
            self.register_buffer("e_score_correction_bias", torch.linspace(-0.1, 0.1, 8))

    net = torch.nn.ModuleList([DeepseekV3TopkRouter(), Glm4MoeTopkRouter()])
    torch.nn.init.normal_(net[1].weight, 0, 0.1)
    assert M.inject_fused_router(net) == 1 and "forward" not in net[0].__dict__
    x = torch.randn(3, 64, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        logits, w, idx = net[1](x)
        ref = M._route_grouped_composition(x, net[1].weight, net[1].e_score_correction_bias, 2, 2, 1, True, 1.5, True)
    assert all(torch.equal(a, b) for a, b in zip((logits, w, idx), ref))
    assert (idx // 4 == idx[:, :1] // 4).all()                          # one group stays: both experts come from it
    assert M.remove_fused_router(net) == 1


# ---------------------------------------------------------------- the shared experts on the tiny DeepSeek-V3 (CPU)
@pytest.fixture(scope="module")
def tiny_q(tmp_path_factory):
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    import _tiny_deepseek_v3 as TD
    model, _ = TD.build(tmp_path_factory.mktemp("deepseekv3"))
    return TD, model


def test_inject_shared_expert_binds_the_deepseek_blocks(tiny_q, monkeypatch):
    TD, model = tiny_q
    from test_moe_shared_host import _cpu_stand_ins
    _cpu_stand_ins(monkeypatch, TD)
    blocks = TD.moe_blocks(model)
    keys = list(model.state_dict().keys())
    x = (torch.rand((1, 5, TD.H), generator=torch.Generator().manual_seed(3)) - 0.5).half()
    with torch.no_grad():
        ref = [b(x) for b in blocks]
    assert M.inject_shared_expert(model) == len(blocks) == 1
    assert M.inject_fused_router(model) == 1                            # the block calls self.gate(...) as before: the fused router composes
    try:
        assert all("forward" in b.__dict__ and type(b).__name__ == "DeepseekV3MoE" for b in blocks)
        assert list(model.state_dict().keys()) == keys
        parts = M.injected_shared_blocks(model)
        assert len(parts) == 1 and parts[0][0] is blocks[0].experts and parts[0][1][0] is blocks[0].shared_experts.gate_proj
        with torch.no_grad():
            got = [b(x) for b in blocks]
        for b, r, g in zip(blocks, ref, got):
            assert g.shape == r.shape and torch.equal(g, r)
            assert b.experts.last_plan["shared"] == "torch" and "cpu" in b.experts.last_plan["shared_reason"]
        assert M.inject_shared_expert(model) == 1                       # idempotent
    finally:
        assert M.remove_fused_router(model) == 1
        assert M.remove_shared_expert(model) == 1
    assert all("forward" not in b.__dict__ and "_shared_expert_injected" not in b.__dict__ for b in blocks)
    with torch.no_grad():
        for b, r in zip(blocks, ref):
            assert torch.equal(b(x), r)


def test_ungated_torch_path_is_routed_plus_shared(tiny_q, monkeypatch):
    TD, model = tiny_q
    from test_moe_shared_host import _cpu_stand_ins
    _cpu_stand_ins(monkeypatch, TD)
    b = TD.moe_blocks(model)[0]
    se = b.shared_experts
    layers = (se.gate_proj, se.up_proj, se.down_proj)
    x = (torch.rand((5, TD.H), generator=torch.Generator().manual_seed(4)) - 0.5).half()
    with torch.no_grad():
        _, w, idx = b.gate(x)
        out = M.moe_shared_forward(b.experts, layers, None, x, idx, w)
        ref = b.experts(x, idx, w) + se.down_proj(torch.nn.functional.silu(se.gate_proj(x)) * se.up_proj(x))
    assert b.experts.last_plan["shared"] == "torch" and torch.equal(out, ref)


def test_blocks_with_a_gate_go_the_qwen_way_and_odd_blocks_are_left_alone(tiny_q):
    TD, model = tiny_q
    b = TD.moe_blocks(model)[0]
    try:
        b.shared_expert_gate = torch.nn.Linear(TD.H, 1, bias=False).half()      # a block with a gate is the Qwen form: it needs ``shared_expert``
        assert M._shared_block_parts(b) is None and M.inject_shared_expert(model) == 0
        b.shared_expert = b.shared_experts
        parts = M._shared_block_parts(b)
        assert parts is not None and parts[1][0] is b.shared_experts.gate_proj
        b.shared_expert_gate = torch.nn.Linear(TD.H, 1, bias=True).half()       # ... and the Qwen checks on the gate hold
        assert M._shared_block_parts(b) is None
    finally:
        del b.shared_expert_gate
        if "shared_expert" in b._modules:
            del b.shared_expert
    assert M._shared_block_parts(b) is not None
    down = b.shared_experts.down_proj
    try:
        b.shared_experts.down_proj = b.experts[0].down_proj                      # [I -> H] where [I_s -> H] belongs
        assert M._shared_block_parts(b) is None
    finally:
        b.shared_experts.down_proj = down
    assert M.inject_shared_expert(model) == 1 and M.remove_shared_expert(model) == 1
