"""GPU: the decode path of the routed mixture-of-experts layers (gptq_moe_decode_forward through QuantMoEExperts.post_init(decode_copy=True) / moe_forward):
1..4 tokens on the experts' decode copy, two launches, the expert chosen on the device.

Its arithmetic is that of the dense decode-copy kernel -- w - z exact in the layer dtype, products exact in fp32, fp32 sums per run of 32 (8 bits: 16) k,
the group's scale applied to the fp32 sum; W is never rounded -- so every output is checked with the error model of that family (test_gpu_error_model.py):

    |y - y64|  <=  (1/2 + 1/64) ulp(y64)  +  C sqrt(K) 2^-24 A,      A = |a| @ |W64|,   C = 4,   W64 = scales (w - z) in fp64, UNROUNDED

C = 4 is the project's constant for the decode kernels (4x4x4 matrix-core steps into per-run fp32 sums, then swaps / LDS in a fixed order).  bf16: this kernel
decodes w - z in fp16 and converts the pair to bf16 (exact: |w - z| <= 256); it carries no biased weights, so A is taken on |W64| itself for both dtypes.
H is checked against silu(g64) * u64 with the bound propagated through silu * mul as test_gpu_moe.check does, out against the fp64 product of the
kernel's OWN H rows (the combine adds topk products in fp32: inside the same term)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.moe import QuantMoEExperts, moe_forward  # noqa: E402
from test_gpu_moe import _fill, _routing, _ulp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 4.0


def make_experts(E, H, I, bits, gs, act, dtype, seed=0, top_k=2, decode_copy=True):
    gen = torch.Generator().manual_seed(seed)
    q = QuantMoEExperts(E, H, I, bits, gs, top_k=top_k, weight_dtype=dtype)
    for e in range(E):
        for l in q[e].layers():
            _fill(l, gen, act)
    q = q.to(DEV)
    q.post_init(decode_copy=decode_copy)
    return q


def _w64(lin):
    """scales[g(k)] * (w[k] - z[g(k)]) in fp64, unrounded, [K, N] -- from the checkpoint tensors (4 / 8 bits: whole fields per word)."""
    bits, K, N = lin.bits, lin.infeatures, lin.outfeatures
    per, maxq = 32 // bits, (1 << bits) - 1
    sh = (torch.arange(per, device=DEV, dtype=torch.int32) * bits)
    w = ((lin.qweight.unsqueeze(1) >> sh.view(1, -1, 1)) & maxq).reshape(K, N)
    z = ((lin.qzeros.unsqueeze(2) >> sh.view(1, 1, -1)) & maxq).reshape(lin.qzeros.shape[0], N) + 1
    if lin.resolved_zero_mode() == _lib.ZERO_WRAP:
        z = z & maxq
    g = lin.g_idx.long()
    return lin.scales.double()[g] * (w - z[g]).double()


def check(q, x, idx, w, dtype):
    """Run the decode path with its intermediate and check H and out against the fp64 oracles; returns (out, H, pos)."""
    T, topk = idx.shape
    plan = q.plan(T, topk)
    assert plan["path"] == "decode" and plan["launches"] == 2, plan
    with torch.no_grad():
        out, hs, pos = moe_forward(q, x, idx, w, return_intermediate=True)
    assert q.last_plan["path"] == "decode"
    H, I = q.hidden_dim, q.intermediate_dim
    assert out.shape == (T, H) and out.dtype == dtype and hs.shape == (T * topk, I)
    x64 = x.double()
    y64 = torch.zeros((T, H), dtype=torch.float64, device=DEV)
    A = torch.zeros_like(y64)
    valid = (idx >= 0) & (idx < q.num_experts)
    want_pos = torch.where(valid, torch.arange(T * topk, device=DEV, dtype=torch.int32).view(T, topk), torch.full_like(pos, -1))
    assert torch.equal(pos, want_pos)
    worst_h = worst_o = 0.0
    for e in sorted(set(idx[valid].tolist())):
        tok, j = torch.where(idx == e)
        gate, up, down = q[e].layers()
        W1, W3, W2 = _w64(gate), _w64(up), _w64(down)
        xe = x64[tok]
        g64, u64 = xe @ W1, xe @ W3
        Eg = C * H ** 0.5 * 2.0 ** -24 * (xe.abs() @ W1.abs())
        Eu = C * H ** 0.5 * 2.0 ** -24 * (xe.abs() @ W3.abs())
        s64 = g64 * torch.sigmoid(g64)
        h64 = s64 * u64
        bound_h = (0.5 + 1 / 64) * _ulp(h64, dtype) + 1.1 * Eg * (u64.abs() + Eu) + s64.abs() * Eu + 1e-6 * h64.abs() + 1e-30
        hk = hs[pos[tok, j].long()].double()
        err = (hk - h64).abs()
        worst_h = max(worst_h, float((err / bound_h).max()))
        assert bool((err <= bound_h).all()), f"H expert {e}: worst err/bound {float((err / bound_h).max()):.3f}"
        wj = w[tok, j].double()[:, None]
        y64.index_add_(0, tok, wj * (hk @ W2))
        A.index_add_(0, tok, wj.abs() * (hk.abs() @ W2.abs()))
    bound = (0.5 + 1 / 64) * _ulp(y64, dtype) + C * I ** 0.5 * 2.0 ** -24 * A + 1e-30
    err = (out.double() - y64).abs()
    worst_o = float((err / bound).max())
    print(f"moe decode T={T} bits={q.bits} {str(dtype)[6:]}: worst err/bound H {worst_h:.3f} out {worst_o:.3f}")
    assert bool((err <= bound).all()), f"out: worst err/bound {worst_o:.3f}"
    return out, hs, pos


def _x(T, H, dtype, seed):
    return (torch.rand((T, H), generator=torch.Generator().manual_seed(seed)) - 0.5).to(dtype).to(DEV)


SHAPES = [(8, 2, 256, 512), (60, 4, 2048, 1408)]


@pytest.mark.parametrize("shape", SHAPES, ids=["e8", "e60"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [32, 128, -1])
@pytest.mark.parametrize("bits", [4, 8])
def test_parity_grid(bits, gs, act, dtype, shape):
    E, topk, H, I = shape
    q = make_experts(E, H, I, bits, gs, act, dtype, seed=bits + gs + E, top_k=topk)
    for T in (1, 2, 3, 4):
        idx, w = _routing(T, E, topk, T + E)
        check(q, _x(T, H, dtype, T), idx, w, dtype)


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
def test_mixtral_8x7b_block(act):
    """H 4096, I 14336, E 8, topk 2, 4-bit g128 fp16."""
    dtype = torch.float16
    q = make_experts(8, 4096, 14336, 4, 128, act, dtype, seed=11)
    for T in (1, 4):
        idx, w = _routing(T, 8, 2, T)
        check(q, _x(T, 4096, dtype, T), idx, w, dtype)


def test_routing_edge_cases():
    dtype = torch.float16
    q = make_experts(8, 256, 512, 4, 128, False, dtype, seed=3)
    T = 4
    x = _x(T, 256, dtype, 1)
    w = torch.full((T, 2), 0.5, device=DEV)
    # all tokens on one expert: every assignment of the call reads the same table entry and the same strips
    idx = torch.full((T, 2), 5, dtype=torch.int64, device=DEV)
    check(q, x, idx, w, dtype)
    check(q, x, idx[:, :1].contiguous(), torch.ones((T, 1), device=DEV), dtype)
    # indices == E and -1 are dropped; a token with none left gets exactly 0
    idx = torch.tensor([[8, 3], [1, -1], [8, -1], [6, 0]], dtype=torch.int64, device=DEV)
    out, _, pos = check(q, x, idx, w, dtype)
    assert pos.tolist() == [[-1, 1], [2, -1], [-1, -1], [6, 7]]
    assert bool((out[2] == 0).all()) and bool((out[0] != 0).any())
    # a repeated expert within a token's top-k counts twice
    idx = torch.tensor([[4, 4], [1, 1], [7, 7], [0, 0]], dtype=torch.int64, device=DEV)
    out2, _, pos2 = check(q, x, idx, w, dtype)
    assert bool((pos2[:, 0] != pos2[:, 1]).all())
    with torch.no_grad():
        single = moe_forward(q, x, idx[:, :1], torch.ones((T, 1), device=DEV))
    assert torch.allclose(out2.float(), single.float(), rtol=1e-2, atol=1e-3)
    # T = 0: nothing launched, an empty result
    with torch.no_grad():
        out0 = moe_forward(q, x[:0], idx[:0], w[:0])
    assert out0.shape == (0, 256)


def test_reproducible_permutation_invariant_and_row_independent():
    dtype = torch.bfloat16
    q = make_experts(60, 2048, 1408, 4, 128, True, dtype, seed=5, top_k=4)
    T = 4
    x = _x(T, 2048, dtype, 9)
    idx, w = _routing(T, 60, 4, 9)
    with torch.no_grad():
        a = moe_forward(q, x, idx, w)
        b = moe_forward(q, x, idx, w)
        p = torch.tensor([2, 0, 3, 1], device=DEV)
        c = moe_forward(q, x[p], idx[p], w[p])
        rows = [moe_forward(q, x[t:t + 1], idx[t:t + 1], w[t:t + 1]) for t in range(T)]
    assert q.last_plan["path"] == "decode"
    assert torch.equal(a, b)
    assert torch.equal(a[p], c)
    for t in range(T):
        assert torch.equal(a[t:t + 1], rows[t]), t


def test_decode_agrees_with_grouped_and_per_expert_and_allocates_nothing():
    from autogptq_amd.moe import _per_expert
    from autogptq_amd.model_utils import autogptq_post_init
    dtype = torch.float16
    q = make_experts(8, 256, 512, 4, 64, False, dtype, seed=8)
    plain = make_experts(8, 256, 512, 4, 64, False, dtype, seed=8, decode_copy=False)
    autogptq_post_init(torch.nn.Sequential(q), max_input_length=64, expert_decode_copy=True)
    autogptq_post_init(torch.nn.Sequential(plain), max_input_length=64)
    for T in (1, 2, 3, 4):
        x = _x(T, 256, dtype, T)
        idx, w = _routing(T, 8, 2, T)
        assert q.plan(T)["path"] == "decode" and plain.plan(T)["path"] == "grouped"
        with torch.no_grad():
            ref = _per_expert(plain, x, idx, w)
            grouped = moe_forward(plain, x, idx, w)
            moe_forward(q, x, idx, w)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            out = moe_forward(q, x, idx, w)
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated() - before
        assert q.last_plan["path"] == "decode" and plain.last_plan["path"] == "grouped"
        assert grown <= out.numel() * out.element_size() + 512, grown
        assert torch.allclose(out.float(), grouped.float(), rtol=2e-2, atol=2e-3), float((out.float() - grouped.float()).abs().max())
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
    assert q.last_plan["path"] == "decode"
    for r in range(3):
        xn = _x(T, 256, dtype, r)
        idn, wn = _routing(T, 8, 2, 100 + r)
        x.copy_(xn), idx.copy_(idn), w.copy_(wn)
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = moe_forward(q, xn, idn, wn)
        assert torch.equal(out, eager), r


def test_default_is_unchanged_and_the_copy_is_reported():
    dtype = torch.float16
    plain = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, decode_copy=False)
    plain2 = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, decode_copy=False)
    plain2.post_init()                                            # the call existing callers make
    copy = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7)
    for T in (1, 2, 3, 4):
        for p in (plain, plain2):
            d = p.plan(T)
            assert d["path"] == "grouped" and d["launches"] == 4, d
        assert copy.plan(T)["path"] == "decode"
    assert plain.decode_copy_bytes == 0 and plain2.decode_copy_bytes == 0
    packed = sum(l.qweight.numel() * 4 for e in range(8) for l in copy[e].layers())
    assert packed <= copy.decode_copy_bytes <= 1.2 * packed, (copy.decode_copy_bytes, packed)      # the weights once more + the constants records
    T = 64
    x = _x(T, 256, dtype, 2)
    idx, w = _routing(T, 8, 2, 2)
    assert plain.plan(T)["path"] == "grouped" and copy.plan(T)["path"] == "grouped"
    with torch.no_grad():
        assert torch.equal(moe_forward(plain, x, idx, w), moe_forward(copy, x, idx, w))


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
    autogptq_post_init(model, max_input_length=64, expert_decode_copy=True)
    return TM, model, twin


@pytest.mark.parametrize("desc_act", [False, True])
def test_tiny_mixtral_end_to_end(tmp_path, desc_act):
    """A prompt of 12 tokens runs the grouped path, the decode steps of generate the decode path; hooked during one decode step, every MoE layer agrees with
    the fp16 twin's MixtralExperts on the same inputs at the tolerance of test_gpu_moe.test_tiny_mixtral_end_to_end."""
    TM, model, twin = _tiny(tmp_path, desc_act)
    experts = [layer.mlp.experts for layer in model.model.layers]
    ids = torch.randint(0, 512, (1, 12), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        logits = model(ids).logits.float()
    assert torch.isfinite(logits).all()
    assert all(ex.last_plan["path"] == "grouped" for ex in experts)
    seen = []
    hooks = [ex.register_forward_hook(lambda m, args, out: seen.append((m, args, out, dict(m.last_plan)))) for ex in experts]
    with torch.no_grad():
        ga = model.generate(ids, max_new_tokens=4, do_sample=False)
    for h in hooks:
        h.remove()
    assert ga.shape == (1, 16)
    steps = [s for s in seen if s[1][0].reshape(-1, s[1][0].shape[-1]).shape[0] == 1]
    assert len(steps) >= 2 * 3 and all(s[3]["path"] == "decode" for s in steps), [s[3] for s in seen]
    for m, (hs, idx, w), out, _ in steps[:2]:
        li = experts.index(m)
        with torch.no_grad():
            ref = twin.model.layers[li].mlp.experts(hs, idx, w)
        err = (out.float() - ref.float()).abs().max().item()
        assert err <= 1e-2 * max(1.0, ref.abs().max().item()), (li, err)


def test_tiny_mixtral_decode_step_capture(tmp_path):
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
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
    assert all(layer.mlp.experts.last_plan["path"] == "decode" for layer in model.model.layers)
    got = [tok.item()]
    for _ in range(7):
        tok = step(tok.view(1, 1))[:, -1].argmax(-1)
        got.append(tok.item())
    assert got == ref.tolist()
