"""CPU: the fused mixture-of-experts router -- the C ABI (gptq_moe_router / gptq_describe_moe_router_plan: exports, the plan string of either row regime,
every decline reason before a launch, the NULL checks), the built code objects (one kernel per dtype, scratch-free) and the module logic of
autogptq_amd/moe.py that needs no kernel: inject_fused_router / remove_fused_router on a tiny Mixtral, through moe_route's torch composition."""
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

ROUTER_SYMBOLS = ("gptq_moe_router", "gptq_describe_moe_router_plan")
P = 0x1000                                   # never dereferenced: every call below returns before a launch
UNSUPPORTED, NULL = 3, 1


def _call(x=P, w=P, T=4, H=256, E=8, topk=2, dtype=_lib.GPTQ_F16, flags=0, logits=P, idx=P, wts=P):
    return _lib.load().gptq_moe_router(x, w, T, H, E, topk, dtype, flags, logits, idx, wts, None)


# ---------------------------------------------------------------- ABI
def test_router_symbols_exported_and_declared_abi_still_8():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in ROUTER_SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and hasattr(lib, s), s
    assert declared == set(_lib.EXPORTS)
    assert lib.gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert "#define GPTQ_MI355X_ABI_VERSION 8" in header
    assert _lib.ROUTER_RENORM == int(re.search(r"#define GPTQ_ROUTER_RENORM (\d+)", header).group(1)) == 1
    assert A.moe_route is M.moe_route and A.inject_fused_router is M.inject_fused_router and A.remove_fused_router is M.remove_fused_router


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("dtype", [_lib.GPTQ_F16, _lib.GPTQ_BF16])
def test_plan_string_of_either_regime(dtype):
    lib = _lib.load()
    for E, topk, H in ((8, 2, 4096), (60, 4, 2048), (64, 8, 3584), (128, 8, 2048), (256, 8, 512), (3, 1, 64)):
        for flags in (0, _lib.ROUTER_RENORM):
            for T in range(1, 9):
                d = _lib.describe_moe_router_plan(T, H, E, topk, dtype, flags)
                assert d == {"path": "router", "form": "rows", "wg": T, "waves": 8, "lds": 2 * H + (4 * E + 15) // 16 * 16, "launches": 1}, (T, d)
            for T in (9, 16, 17, 64, 300, 2048):
                d = _lib.describe_moe_router_plan(T, H, E, topk, dtype, flags)
                tiles = -(-E // 16)
                # four tiles of 8 waves' partial sums at a time (32 KiB) + the 16 x (16 tiles') rounded logits
                assert d == {"path": "router", "form": "tiles", "wg": -(-T // 16), "waves": 8, "lds": 32768 + 16 * 16 * tiles * 4, "launches": 1}, (T, d)
                assert d["lds"] <= 65536
    import ctypes
    buf = ctypes.create_string_buffer(256)
    assert lib.gptq_describe_moe_router_plan(4, 256, 8, 2, dtype, 1, buf, len(buf)) == 0
    assert buf.value.decode() == "path=router form=rows wg=4 waves=8 lds=544 launches=1"
    assert lib.gptq_describe_moe_router_plan(17, 320, 60, 4, dtype, 0, buf, len(buf)) == 0
    assert buf.value.decode() == "path=router form=tiles wg=2 waves=8 lds=36864 launches=1"
    assert lib.gptq_describe_moe_router_plan(4, 256, 8, 2, dtype, 0, None, 0) == NULL
    d0 = _lib.describe_moe_router_plan(0, 256, 8, 2, dtype)
    assert d0["path"] == "router" and d0["wg"] == 0, d0


@pytest.mark.parametrize("kw,frag", [
    (dict(dtype=_lib.GPTQ_F32), "fp32"),
    (dict(E=0), "E = 0"),
    (dict(E=257, topk=8), "E = 257"),
    (dict(topk=0), "topk = 0"),
    (dict(topk=9, E=16), "topk = 9"),
    (dict(topk=4, E=3), "topk = 4"),
    (dict(H=96), "H = 96"),
    (dict(flags=2), "flags"),
    (dict(flags=5), "flags"),
])
def test_every_decline_has_a_reason_and_launches_nothing(kw, frag):
    lib = _lib.load()
    full = dict(T=4, H=256, E=8, topk=2, dtype=_lib.GPTQ_F16, flags=0)
    full.update(kw)
    for T in (4, 17, 0):
        full["T"] = T
        d = _lib.describe_moe_router_plan(**full)
        assert d["path"] == "none" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
        assert _call(**full) == UNSUPPORTED and frag in lib.gptq_last_error().decode()


@pytest.mark.parametrize("name", ["x", "w", "logits", "idx", "wts"])
def test_misaligned_pointers_decline(name):
    lib = _lib.load()
    assert _call(**{name: P + 8}) == UNSUPPORTED and "16-byte aligned" in lib.gptq_last_error().decode()
    assert _call(**{name: P + 2, "T": 17}) == UNSUPPORTED and "16-byte aligned" in lib.gptq_last_error().decode()


def test_null_checks_and_zero_tokens():
    lib = _lib.load()
    for name in ("x", "w", "idx", "wts"):
        assert _call(**{name: None}) == NULL and "non-NULL" in lib.gptq_last_error().decode(), name
    assert _call(T=0) == 0 and _call(T=0, logits=None) == 0           # T = 0: nothing is launched, nothing is dereferenced
    assert _call(T=-1) == 2                                           # GPTQ_ERR_SHAPE
    assert _call(T=0, H=96) == UNSUPPORTED                            # ... but the call is still validated


def test_python_plan_and_composition_reasons():
    assert M.router_plan(4, 256, 8, 2, torch.float16)["form"] == "rows" and M.router_plan(9, 256, 8, 2, torch.bfloat16)["form"] == "tiles"
    d = M.router_plan(4, 256, 8, 2, torch.float32)
    assert d["path"] == "none" and "fp32" in d["reason"], d
    assert M.router_plan(4, 256, 8, 2, torch.float64)["path"] == "none"
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn((5, 64), generator=g), torch.randn((6, 64), generator=g)
    for renorm in (False, True):
        logits, val, idx = M.moe_route(x, w, 3, renorm=renorm)
        assert M.last_route_plan == {"path": "none", "reason": "cpu tensors"}
        ref = torch.softmax((x @ w.t()).float(), -1)
        rv, ri = torch.topk(ref, 3, dim=-1)
        rv = rv / rv.sum(-1, keepdim=True) if renorm else rv
        assert torch.equal(idx, ri) and torch.equal(val, rv) and torch.equal(logits, torch.nn.functional.linear(x, w))
        assert val.dtype == torch.float32 and idx.dtype == torch.int64
    assert M.moe_route(x, w, 3, return_logits=False)[0] is None
    # router training keeps autograd
    wp = w.clone().requires_grad_(True)
    _, val, _ = M.moe_route(x, wp, 2)
    val.sum().backward()
    assert wp.grad is not None and torch.isfinite(wp.grad).all()


# ---------------------------------------------------------------- built code objects
def test_router_kernels_are_one_per_dtype_and_scratch_free():
    from test_kernel_resources import _kernels
    ks = _kernels()
    mine = {n: v for n, v in ks.items() if "moe_router_kernel" in n}
    assert len(mine) == 2, sorted(mine)                               # fp16 / bf16: the row regime is a run-time branch
    for n, v in mine.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0), (n, v)
        assert (v["vgpr"] or 0) <= 256 and (v["lds"] or 0) == 0, (n, v)       # 8 waves of 256 registers fit a CU; the LDS is dynamic (the plan's lds=)
    assert len(ks) <= 1160, len(ks)


# ---------------------------------------------------------------- injection on a tiny Mixtral (CPU: moe_route's composition)
@pytest.fixture(scope="module")
def tiny():
    pytest.importorskip("transformers")
    import _tiny_mixtral as TM
    model = TM.fresh_model(0).float()
    ids = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(3))
    return TM, model, ids


def _router_io(model, ids, **kw):
    seen = []
    hooks = [layer.mlp.gate.register_forward_hook(lambda m, args, out: seen.append((args[0].clone(), tuple(o.clone() for o in out))))
             for layer in model.model.layers]
    with torch.no_grad():
        res = model(ids, **kw)
    for h in hooks:
        h.remove()
    return seen, res


def test_inject_on_tiny_mixtral_keeps_classes_keys_outputs_and_recorders(tiny):
    TM, model, ids = tiny
    layers = len(model.model.layers)
    classes = [type(m) for m in model.modules()]
    keys = list(model.state_dict().keys())
    before, res0 = _router_io(model, ids)
    assert len(before) == layers
    try:
        assert M.inject_fused_router(model) == layers
        assert [type(m) for m in model.modules()] == classes and list(model.state_dict().keys()) == keys
        for layer in model.model.layers:
            g = layer.mlp.gate
            assert type(g).__name__ == "MixtralTopKRouter" and "forward" in g.__dict__ and g.forward.__func__ is M._fused_router_forward
        after, res1 = _router_io(model, ids, output_router_logits=True)
        assert len(after) == layers
        for (xi, outs0), (xj, outs1) in zip(before, after):
            assert torch.equal(xi, xj) and len(outs1) == 3
            for a, b in zip(outs0, outs1):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
        assert torch.equal(res0.logits, res1.logits)
        assert len(res1.router_logits) == layers
        for rl, (_, outs1) in zip(res1.router_logits, after):
            assert rl.shape == (ids.numel(), TM.E) and torch.equal(rl, outs1[0])
        assert M.inject_fused_router(model) == layers                  # idempotent
    finally:
        removed = M.remove_fused_router(model)
    assert removed == layers and M.remove_fused_router(model) == 0
    for layer in model.model.layers:
        g = layer.mlp.gate
        assert "forward" not in g.__dict__ and g.forward.__func__ is type(g).forward
    again, _ = _router_io(model, ids)
    for (_, outs0), (_, outs2) in zip(before, again):
        assert all(torch.equal(a, b) for a, b in zip(outs0, outs2))


def test_other_router_classes_are_left_alone_and_qwen_casts_its_scores():
    class Qwen3MoeTopKRouter(torch.nn.Module):
        def __init__(self, norm):
            super().__init__()
            self.top_k, self.num_experts, self.norm_topk_prob, self.hidden_dim = 2, 6, norm, 64
            self.weight = torch.nn.Parameter(torch.randn(6, 64, generator=torch.Generator().manual_seed(1)))

        def forward(self, hidden_states):                              # transformers' Qwen3MoeTopKRouter.forward
            hidden_states = hidden_states.reshape(-1, self.hidden_dim)
            router_logits = torch.nn.functional.linear(hidden_states, self.weight)
            router_probs = torch.nn.functional.softmax(router_logits, dtype=torch.float, dim=-1)
            router_top_value, router_indices = torch.topk(router_probs, self.top_k, dim=-1)
            if self.norm_topk_prob:
                router_top_value /= router_top_value.sum(dim=-1, keepdim=True)
            return router_logits, router_top_value.to(router_logits.dtype), router_indices

    class SigmoidRouter(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.top_k, self.num_experts = 2, 6
            self.weight = torch.nn.Parameter(torch.zeros(6, 64))

        def forward(self, x):
            return torch.sigmoid(x @ self.weight.t())

    net = torch.nn.ModuleList([Qwen3MoeTopKRouter(True), Qwen3MoeTopKRouter(False), SigmoidRouter()]).to(torch.bfloat16)
    x = torch.randn(2, 5, 64, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    with torch.no_grad():
        ref = [net[0](x), net[1](x)]
    assert M.inject_fused_router(net) == 2 and "forward" not in net[2].__dict__
    with torch.no_grad():
        got = [net[0](x), net[1](x)]
    for r, g in zip(ref, got):
        assert g[1].dtype == torch.bfloat16 and all(torch.equal(a, b) for a, b in zip(r, g))
    assert M.remove_fused_router(net) == 2
