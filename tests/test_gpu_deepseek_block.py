"""GPU: a tiny DeepSeek-V3 with the grouped-sigmoid router (inject_fused_router -> moe_route_grouped) and the ungated shared experts
(inject_shared_expert -> moe_shared_forward(gate_weight=None)) injected, after autogptq_post_init(expert_decode_copy=True).

The block against fp64: y64 = sum_j w_j (h64_j @ W2_e) + hs64 @ W2_s at the EMITTED routing, h64 = silu(g64) * u64 from x and the dequantised weights in
fp64.  The bound is the one test_gpu_moe_shared.py uses for the Qwen block, with the gate scalar s = 1 and the H rows' own bound (its _silu_mul_bound)
carried through the down projections:

    sum_j w_j (bound_h_j @ |W2_e|) + bound_hs @ |W2_s| + C 2^-24 (sqrt(I) A_routed + sqrt(I_s) A_shared) + (1/2 + 1/64) ulp(y64)

with C = 4 where the fused decode call runs (1..2 tokens: one fp32 sum, one rounding), and where the combine form runs (3 tokens and more) C = 16 -- the
project's constant for the matrix-core chains of the grouped path and of mlp_forward -- plus the two roundings that form adds: (1/2 + 1/64) (ulp(routed64) +
ulp(shared64)), the routed and the shared output each rounded to the layer dtype before the combine launch adds them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import moe as M  # noqa: E402
from test_gpu_moe import _ulp, _w64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    import _tiny_deepseek_v3 as TD
    from autogptq_amd.model_utils import autogptq_post_init
    model, twin = TD.build(tmp_path_factory.mktemp("deepseekv3"))
    model, twin = model.to(DEV), twin.to(DEV)
    n = len(TD.moe_blocks(model))
    assert n == 1
    assert M.inject_fused_router(model) == n and M.inject_shared_expert(model) == n
    autogptq_post_init(model, max_input_length=128, expert_decode_copy=True)
    return TD, model, twin


def _silu_mul(x64, W1, W3, K, dtype, C):
    """(h64, its bound): test_gpu_moe_shared._silu_mul_bound with the chain constant as an argument."""
    g64, u64 = x64 @ W1, x64 @ W3
    Eg = C * K ** 0.5 * 2.0 ** -24 * (x64.abs() @ W1.abs())
    Eu = C * K ** 0.5 * 2.0 ** -24 * (x64.abs() @ W3.abs())
    s64 = g64 * torch.sigmoid(g64)
    h64 = s64 * u64
    return h64, (0.5 + 1 / 64) * _ulp(h64, dtype) + 1.1 * Eg * (u64.abs() + Eu) + s64.abs() * Eu + 1e-6 * h64.abs() + 1e-30


@pytest.mark.parametrize("T", [1, 2, 3, 4, 7, 70])
def test_block_against_fp64_at_the_emitted_routing(tiny, T):
    TD, model, _ = tiny
    blk = TD.moe_blocks(model)[0]
    q, se = blk.experts, blk.shared_experts
    dtype = torch.float16
    x = ((torch.rand((1, T, TD.H), generator=torch.Generator().manual_seed(T)) - 0.5) * 2).to(dtype).to(DEV)
    seen = []
    h = blk.gate.register_forward_hook(lambda m, args, out: seen.append(out))
    with torch.no_grad():
        out = blk(x)
    h.remove()
    assert M.last_route_plan["path"] == "router_grouped" and M.last_route_plan["form"] == ("rows" if T <= 8 else "tiles")
    plan = q.last_plan
    assert plan["shared"] == ("decode" if T <= 2 else "combine"), plan
    assert plan["path"] == ("decode" if T <= 4 else "grouped"), plan
    logits, w, idx = seen[0]
    assert logits.dtype == torch.float32 and logits.shape == (T, TD.E) and w.dtype == torch.float32 and idx.shape == (T, TD.TOPK)
    # the routing is the router's contract on the block's own input (bias: the fp16 buffer read through its fp32 copy)
    ref = M._route_grouped_composition(x.reshape(T, TD.H), blk.gate.weight, blk.gate.e_score_correction_bias, TD.TOPK, TD.N_GROUP, TD.TOPK_GROUP, True,
                                       TD.SCALE, True)
    assert (logits - ref[0]).abs().max().item() <= 1e-4
    groups = idx // (TD.E // TD.N_GROUP)
    assert all(len(set(g.tolist())) <= TD.TOPK_GROUP for g in groups)                # group-limited
    assert ((w.sum(-1) - TD.SCALE).abs() <= 1e-5).all()                              # renormalised, then scaled
    C = 4.0 if T <= 2 else 16.0
    H, I, Is = TD.H, TD.I, TD.I_S
    x64 = x.reshape(T, H).double()
    y_r = torch.zeros((T, H), dtype=torch.float64, device=DEV)
    A_r, B_r = torch.zeros_like(y_r), torch.zeros_like(y_r)
    for e in sorted(set(idx.flatten().tolist())):
        tok, j = torch.where(idx == e)
        gate, up, down = q[e].layers()
        h64, bound_h = _silu_mul(x64[tok], _w64(gate), _w64(up), H, dtype, C)
        W2 = _w64(down)
        wj = w[tok, j].double()[:, None]
        y_r.index_add_(0, tok, wj * (h64 @ W2))
        A_r.index_add_(0, tok, wj * (h64.abs() @ W2.abs()))
        B_r.index_add_(0, tok, wj * (bound_h @ W2.abs()))
    h64, bound_h = _silu_mul(x64, _w64(se.gate_proj), _w64(se.up_proj), H, dtype, C)
    W2s = _w64(se.down_proj)
    y_s = h64 @ W2s
    A_s, B_s = h64.abs() @ W2s.abs(), bound_h @ W2s.abs()
    y64 = y_r + y_s
    bound = B_r + B_s + C * 2.0 ** -24 * (I ** 0.5 * A_r + Is ** 0.5 * A_s) + (0.5 + 1 / 64) * _ulp(y64, dtype) + 1e-30
    if T > 2:
        bound = bound + (0.5 + 1 / 64) * (_ulp(y_r, dtype) + _ulp(y_s, dtype))
    err = (out.reshape(T, H).double() - y64).abs()
    print(f"deepseek block T={T} [{plan['shared']} / {plan['path']}]: worst err/bound {float((err / bound).max()):.3f}")
    assert out.shape == x.shape and out.dtype == dtype and bool((err <= bound).all()), float((err / bound).max())


def test_model_against_the_fp16_twin_and_greedy_generation(tiny):
    TD, model, twin = tiny
    blocks = TD.moe_blocks(model)
    seen = []
    hooks = [b.register_forward_hook(lambda m, args, out: seen.append((m, args[0], out, dict(m.experts.last_plan)))) for b in blocks]
    ids = torch.randint(0, 512, (1, 12), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        logits = model(ids).logits.float()
        ref = twin(ids).logits.float()
    for h in hooks:
        h.remove()
    err = (logits - ref).abs().max().item()
    print(f"tiny deepseek-v3 logits against the twin: max err {err:.3e}, scale {ref.abs().max().item():.2f}")
    assert torch.isfinite(logits).all() and err <= 1e-2 * max(1.0, ref.abs().max().item()), err
    assert len(seen) == 1 and seen[0][3]["shared"] == "combine"
    for m, hs, out, _ in seen:                      # per block, on the SAME hidden states, at the tolerance of test_tiny_qwen2_moe_end_to_end
        with torch.no_grad():
            r = TD.moe_blocks(twin)[blocks.index(m)](hs)
        e = (out.float() - r.float()).abs().max().item()
        assert out.shape == r.shape and e <= 1e-2 * max(1.0, r.abs().max().item()), e
    ids = torch.randint(0, 512, (1, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        ga = model.generate(ids, max_new_tokens=8, do_sample=False)
        gb = twin.generate(ids, max_new_tokens=8, do_sample=False)
    assert ga.shape == (1, 16) and torch.equal(ga, gb), (ga.tolist(), gb.tolist())
    assert blocks[0].experts.last_plan["shared"] == "decode" and blocks[0].experts.last_plan["path"] == "decode"      # the decode steps ran the fused call


def test_capture_decode_step_replays_bit_equal_to_eager(tiny):
    from transformers import StaticCache
    from autogptq_amd.model_utils import capture_decode_step
    TD, model, _ = tiny
    ids = torch.randint(0, 512, (1, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    caches = [StaticCache(config=model.config, max_cache_len=64) for _ in range(2)]
    with torch.no_grad():
        first = [model(ids, past_key_values=c, use_cache=True).logits for c in caches]
    assert torch.equal(first[0], first[1])
    tok = first[0][:, -1].argmax(-1)
    step = capture_decode_step(model, caches[0])
    blk = TD.moe_blocks(model)[0]
    assert blk.experts.last_plan["shared"] == "decode" and M.last_route_plan["path"] == "router_grouped"
    for _ in range(7):
        got = step(tok.view(1, 1)).clone()
        with torch.no_grad():
            eager = model(tok.view(1, 1), past_key_values=caches[1], use_cache=True).logits
        assert torch.equal(got, eager)
        tok = got[:, -1].argmax(-1)


def test_remove_restores_the_class_forwards(tiny):
    """Last in the file: the module-scoped model loses its injected forwards here (and gets them back)."""
    TD, model, _ = tiny
    blk = TD.moe_blocks(model)[0]
    x = ((torch.rand((1, 3, TD.H), generator=torch.Generator().manual_seed(9)) - 0.5) * 2).half().to(DEV)
    with torch.no_grad():
        fused = blk(x)
    assert M.remove_shared_expert(model) == 1 and M.remove_fused_router(model) == 1
    try:
        assert "forward" not in blk.__dict__ and blk.forward.__func__ is type(blk).forward
        assert "forward" not in blk.gate.__dict__ and blk.gate.forward.__func__ is type(blk.gate).forward
        assert M.injected_shared_blocks(model) == []
        with torch.no_grad():
            plain = blk(x)                          # the class forward on the quantised modules: transformers' router, experts, shared MLP, add
        assert (plain.float() - fused.float()).abs().max().item() <= 1e-2 * max(1.0, plain.float().abs().max().item())
    finally:
        assert M.inject_fused_router(model) == 1 and M.inject_shared_expert(model) == 1
