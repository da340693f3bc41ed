"""GPU: routed mixture-of-experts layers (gptq_moe_forward through QuantMoEExperts / moe_forward) against fp64 oracles of the formulas in
include/gptq_mi355x.h, with the per-output error model of test_gpu_error_model.py (C = 16: the matrix core chains a whole K range per wave):

    |y - y64|  <=  (1/2 + 1/64) ulp(y64)  +  C sqrt(K) 2^-24 A,      A = |a| @ |W|

H_sorted is checked against silu(g64) * u64 with the bound propagated through silu * mul; out against the fp64 product of the kernel's OWN H rows."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd.moe import QuantMoEExperts, moe_forward  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 16.0


def _ulp(y64, dtype):
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(y64.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=y64.device), e - mant)


def _fill(lin, gen, act):
    K, N, bits, gs = lin.infeatures, lin.outfeatures, lin.bits, lin.group_size
    lin.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qweight.shape, generator=gen, dtype=torch.int64).to(torch.int32)
    lin.qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qzeros.shape, generator=gen, dtype=torch.int64).to(torch.int32)
    lin.scales = (torch.rand(lin.scales.shape, generator=gen) * 0.004 + 0.001).to(lin.scales.dtype) * (16.0 / (1 << bits))
    gi = torch.arange(K, dtype=torch.int32) // gs
    lin.g_idx = gi[torch.randperm(K, generator=gen)].contiguous() if act else gi


def make_experts(E, H, I, bits, gs, act, dtype, seed=0, top_k=2):
    gen = torch.Generator().manual_seed(seed)
    q = QuantMoEExperts(E, H, I, bits, gs, top_k=top_k, weight_dtype=dtype)
    for e in range(E):
        for l in q[e].layers():
            _fill(l, gen, act)
    q = q.to(DEV)
    q.post_init()
    return q


def _routing(T, E, topk, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]) if T else torch.zeros((0, topk), dtype=torch.int64)
    w = torch.rand((T, topk), generator=g) + 0.1
    w = w / w.sum(-1, keepdim=True)
    return idx.to(DEV), w.to(DEV).float()


def _w64(q):
    return q.dequantize().double()           # [K, N]: the weights the kernels must use, bit for bit


def check(q, x, idx, w, dtype):
    """Run the grouped path with its intermediate and check H and out against the fp64 oracles; returns (out, H, pos)."""
    assert q.plan(x.shape[0], idx.shape[1])["path"] == "grouped"
    with torch.no_grad():
        out, hs, pos = moe_forward(q, x, idx, w, return_intermediate=True)
    T, topk = idx.shape
    H, I = q.hidden_dim, q.intermediate_dim
    assert out.shape == (T, H) and out.dtype == dtype
    if T == 0:
        return out, hs, pos
    x64 = x.double()
    y64 = torch.zeros((T, H), dtype=torch.float64, device=DEV)
    A = torch.zeros_like(y64)
    valid = (idx >= 0) & (idx < q.num_experts)
    assert torch.equal(pos >= 0, valid)
    for e in range(q.num_experts):
        tok, j = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        gate, up, down = q[e].layers()
        W1, W3, W2 = _w64(gate), _w64(up), _w64(down)
        xe = x64[tok]
        g64, u64 = xe @ W1, xe @ W3
        Eg = C * H ** 0.5 * 2.0 ** -24 * (xe.abs() @ W1.abs())
        Eu = C * H ** 0.5 * 2.0 ** -24 * (xe.abs() @ W3.abs())
        s64 = g64 * torch.sigmoid(g64)
        h64 = s64 * u64
        bound_h = (0.5 + 1 / 64) * _ulp(h64, dtype) + 1.1 * Eg * (u64.abs() + Eu) + s64.abs() * Eu + 1e-6 * h64.abs() + 1e-30
        rows = pos[tok, j].long()
        hk = hs[rows].double()
        err = (hk - h64).abs()
        assert bool((err <= bound_h).all()), f"H expert {e}: worst err/bound {float((err / bound_h).max()):.3f}"
        wj = w[tok, j].double()[:, None]
        y64.index_add_(0, tok, wj * (hk @ W2))
        A.index_add_(0, tok, wj.abs() * (hk.abs() @ W2.abs()))
    bound = (0.5 + 1 / 64) * _ulp(y64, dtype) + C * I ** 0.5 * 2.0 ** -24 * A + 1e-30
    err = (out.double() - y64).abs()
    assert bool((err <= bound).all()), f"out: worst err/bound {float((err / bound).max()):.3f}"
    return out, hs, pos


SHAPES = [(8, 2, 256, 512), (60, 4, 2048, 1408)]
TS = (0, 1, 2, 3, 7, 64, 300)
_CACHE = {}


@pytest.mark.parametrize("shape", SHAPES, ids=["e8", "e60"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [32, 128, -1])
@pytest.mark.parametrize("bits", [4, 8])
def test_parity_grid(bits, gs, act, dtype, shape):
    E, topk, H, I = shape
    q = make_experts(E, H, I, bits, gs, act, dtype, seed=bits + gs + E, top_k=topk)
    for T in TS:
        x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).to(dtype).to(DEV)
        idx, w = _routing(T, E, topk, T + E)
        check(q, x, idx, w, dtype)


def test_routing_edge_cases():
    dtype = torch.float16
    q = make_experts(8, 256, 512, 4, 128, False, dtype, seed=3)
    T = 50
    x = (torch.rand((T, 256), generator=torch.Generator().manual_seed(1)) - 0.5).to(dtype).to(DEV)
    w = torch.full((T, 2), 0.5, device=DEV)
    # every token to one expert (most experts get no rows)
    idx = torch.full((T, 2), 5, dtype=torch.int64, device=DEV)
    idx[:, 1] = 2
    check(q, x, idx, w, dtype)
    # indices == E and -1 are dropped; a token with none left gets 0
    idx = torch.randint(0, 8, (T, 2), generator=torch.Generator().manual_seed(2)).to(DEV)
    idx[::3, 0] = 8
    idx[1::4, 1] = -1
    idx[7] = torch.tensor([8, -1])
    out, _, pos = check(q, x, idx, w, dtype)
    assert bool((pos[7] == -1).all()) and bool((out[7] == 0).all())
    # a repeated expert within a token's top-k counts twice
    idx = torch.randint(0, 8, (T, 1), generator=torch.Generator().manual_seed(3)).to(DEV).repeat(1, 2)
    out2, _, pos2 = check(q, x, idx, w, dtype)
    assert bool((pos2[:, 0] != pos2[:, 1]).all())
    with torch.no_grad():
        single = moe_forward(q, x, idx[:, :1], torch.ones((T, 1), device=DEV))
    assert torch.allclose(out2.float(), single.float(), rtol=1e-2, atol=1e-3)
    # T = 0: nothing launched, an empty result
    out0, _, _ = check(q, x[:0], idx[:0], w[:0], dtype)
    assert out0.shape == (0, 256)


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
def test_mixtral_8x7b_block(act):
    """H 4096, I 14336, E 8, topk 2, 4-bit g128 fp16: every output against the fp64 product on the device."""
    dtype = torch.float16
    q = make_experts(8, 4096, 14336, 4, 128, act, dtype, seed=11)
    for T in (1, 4, 64, 2048):
        x = (torch.rand((T, 4096), generator=torch.Generator().manual_seed(T)) - 0.5).to(dtype).to(DEV)
        idx, w = _routing(T, 8, 2, T)
        check(q, x, idx, w, dtype)


def test_reproducible_and_permutation_invariant():
    dtype = torch.bfloat16
    q = make_experts(60, 2048, 1408, 4, 128, True, dtype, seed=5, top_k=4)
    T = 300
    x = (torch.rand((T, 2048), generator=torch.Generator().manual_seed(9)) - 0.5).to(dtype).to(DEV)
    idx, w = _routing(T, 60, 4, 9)
    with torch.no_grad():
        a = moe_forward(q, x, idx, w)
        b = moe_forward(q, x, idx, w)
        p = torch.randperm(T, generator=torch.Generator().manual_seed(4)).to(DEV)
        c = moe_forward(q, x[p], idx[p], w[p])
    assert torch.equal(a, b)
    assert torch.equal(a[p], c)


def test_grouped_matches_per_expert_and_allocates_nothing():
    from autogptq_amd.moe import _per_expert
    from autogptq_amd.model_utils import autogptq_post_init
    dtype = torch.float16
    q = make_experts(8, 256, 512, 4, 64, False, dtype, seed=8)
    model = torch.nn.Sequential(q)
    autogptq_post_init(model, max_input_length=64)
    for T in (1, 7, 64):
        x = (torch.rand((T, 256), generator=torch.Generator().manual_seed(T)) - 0.5).to(dtype).to(DEV)
        idx, w = _routing(T, 8, 2, T)
        with torch.no_grad():
            ref = _per_expert(q, x, idx, w)
            moe_forward(q, x, idx, w)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            out = moe_forward(q, x, idx, w)
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated() - before
        assert grown <= out.numel() * out.element_size() + 512, grown
        assert torch.allclose(out.float(), ref.float(), rtol=2e-2, atol=2e-3), float((out.float() - ref.float()).abs().max())


def test_graph_capture_replays_with_new_inputs():
    dtype = torch.float16
    q = make_experts(8, 256, 512, 8, 32, True, dtype, seed=4)
    T = 4
    x = torch.zeros((T, 256), dtype=dtype, device=DEV)
    idx = torch.zeros((T, 2), dtype=torch.int64, device=DEV)
    w = torch.zeros((T, 2), dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        moe_forward(q, x, idx, w)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = moe_forward(q, x, idx, w)
    for r in range(3):
        xn = (torch.rand((T, 256), generator=torch.Generator().manual_seed(r)) - 0.5).to(dtype).to(DEV)
        idn, wn = _routing(T, 8, 2, 100 + r)
        x.copy_(xn), idx.copy_(idn), w.copy_(wn)
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = moe_forward(q, xn, idn, wn)
        assert torch.equal(out, eager), r


def _tiny(tmp_path, desc_act):
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    import _tiny_mixtral as TM
    from autogptq_amd.model_utils import autogptq_post_init
    src = TM.fresh_model(0)
    twin_w = TM.quantize_and_pack(src, desc_act)
    TM.save_checkpoint(src, str(tmp_path), desc_act)
    model, _, _ = TM.load_checkpoint(str(tmp_path))
    twin = TM.make_twin(model.state_dict(), twin_w).to(DEV)
    model = model.to(DEV)
    autogptq_post_init(model, max_input_length=64)
    return TM, model, twin


@pytest.mark.parametrize("desc_act", [False, True])
def test_tiny_mixtral_end_to_end(tmp_path, desc_act):
    """Loaded from the checkpoint and post-initialised, every MoE layer of the quantised model agrees with the fp16 twin's MixtralExperts on the SAME
    inputs (hidden states, routing), and the model generates.  (Whole-model logits are not compared with the twin's: a router near-tie flips an expert
    choice between the two models -- observed with desc_act = False at T = 12 -- and then one token's output differs by design, not by error.)"""
    TM, model, twin = _tiny(tmp_path, desc_act)
    seen = []
    hooks = [layer.mlp.experts.register_forward_hook(lambda m, args, out: seen.append((m, args, out))) for layer in model.model.layers]
    ids = torch.randint(0, 512, (1, 12), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        logits = model(ids).logits.float()
    for h in hooks:
        h.remove()
    assert torch.isfinite(logits).all() and len(seen) == 2
    assert model.model.layers[0].mlp.experts.last_plan["path"] == "grouped"
    for li, (m, (hs, idx, w), out) in enumerate(seen):
        with torch.no_grad():
            ref = twin.model.layers[li].mlp.experts(hs, idx, w)
        err = (out.float() - ref.float()).abs().max().item()
        assert err <= 1e-2 * max(1.0, ref.abs().max().item()), (li, err)
    with torch.no_grad():
        ga = model.generate(ids, max_new_tokens=16, do_sample=False)
    assert ga.shape == (1, 28)


def test_tiny_mixtral_decode_step_capture(tmp_path):
    from transformers import StaticCache
    from autogptq_amd.model_utils import capture_decode_step
    TM, model, _ = _tiny(tmp_path, False)
    ids = torch.randint(0, 512, (1, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        ref = model.generate(ids, max_new_tokens=8, do_sample=False)[0, 8:]
    cache = StaticCache(config=model.config, max_cache_len=64)
    with torch.no_grad():
        logits = model(ids, past_key_values=cache, use_cache=True).logits
    tok = logits[:, -1].argmax(-1)
    step = capture_decode_step(model, cache)
    got = [tok.item()]
    for _ in range(7):
        tok = step(tok.view(1, 1))[:, -1].argmax(-1)
        got.append(tok.item())
    assert got == ref.tolist()


def test_gradients_through_the_experts():
    dtype = torch.float16
    q = make_experts(8, 256, 512, 4, 128, False, dtype, seed=6)
    T = 16
    x = ((torch.rand((T, 256), generator=torch.Generator().manual_seed(0)) - 0.5).to(dtype).to(DEV)).requires_grad_(True)
    idx, w = _routing(T, 8, 2, 0)
    w = w.clone().requires_grad_(True)
    out = moe_forward(q, x, idx, w)
    assert "grad" in q.last_plan["reason"]
    gy = torch.randn((T, 256), generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
    out.backward(gy)
    # twin: the same arithmetic on the dequantised weights in fp32 autograd
    x2 = x.detach().float().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    ref = torch.zeros((T, 256), device=DEV)
    for e in range(8):
        tok, j = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        gate, up, down = q[e].layers()
        W1, W3, W2 = (l.dequantize().float() for l in (gate, up, down))
        h = F.silu(x2[tok] @ W1) * (x2[tok] @ W3)
        ref = ref.index_add(0, tok, (h @ W2) * w2[tok, j, None])
    ref.backward(gy.float())
    assert torch.allclose(x.grad.float(), x2.grad, rtol=3e-2, atol=3e-3), float((x.grad.float() - x2.grad).abs().max())
    assert torch.allclose(w.grad, w2.grad, rtol=3e-2, atol=3e-3), float((w.grad - w2.grad).abs().max())
