"""GPU: the batch path of the routed mixture-of-experts layers (gptq_moe_batch_forward through QuantMoEExperts.post_init(batch=True) / moe_forward):
5..64 tokens on the experts' decode copy, 16-row tiles of one expert over the whole K, four launches (six for act-order experts).

Its arithmetic contract is the grouped path's (every W bit-exact to dequantize(), fp32 products and sums on the matrix core, h rounded once), so every output
is checked as tests/test_gpu_moe.py checks the grouped path, with the error model of test_gpu_error_model.py:

    |y - y64|  <=  (1/2 + 1/64) ulp(y64)  +  C sqrt(K) 2^-24 A,      A = |a| @ |W|,   W = dequantize(),   C = 16

C = 16 is the project's constant for matrix-core chains over a whole K.  H is checked against silu(g64) * u64 with the bound propagated through silu * mul,
out against the fp64 product of the kernel's OWN H rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd.moe import QuantMoEExperts, moe_forward  # noqa: E402
from test_gpu_moe import _fill, _routing, _ulp, _w64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 16.0


def make_experts(E, H, I, bits, gs, act, dtype, seed=0, top_k=2, decode_copy=False, batch=True):
    gen = torch.Generator().manual_seed(seed)
    q = QuantMoEExperts(E, H, I, bits, gs, top_k=top_k, weight_dtype=dtype)
    for e in range(E):
        for l in q[e].layers():
            _fill(l, gen, act)
    q = q.to(DEV)
    q.post_init(decode_copy=decode_copy, batch=batch)
    return q


def _x(T, H, dtype, seed):
    return (torch.rand((T, H), generator=torch.Generator().manual_seed(seed)) - 0.5).to(dtype).to(DEV)


def check(q, x, idx, w, dtype, act=False):
    """Run the batch path with its intermediate and check H and out against the fp64 oracles; returns (out, H, pos)."""
    T, topk = idx.shape
    plan = q.plan(T, topk)
    # act-order experts: one row gather through perm in front of either GEMM whose experts carry one (a shuffled g_idx of ONE group is sequential: no perm)
    gate, up, down = q.projections()
    launches = 4 + int(any(l._layer.perm for l in gate + up)) + int(any(l._layer.perm for l in down))
    assert launches == (6 if act and q[0].layers()[0].group_size < q.hidden_dim else 4), launches
    assert plan["path"] == "batch" and plan["bm"] == 16 and plan["launches"] == launches, plan
    with torch.no_grad():
        out, hs, pos = moe_forward(q, x, idx, w, return_intermediate=True)
    assert q.last_plan["path"] == "batch"
    H, I = q.hidden_dim, q.intermediate_dim
    assert out.shape == (T, H) and out.dtype == dtype and hs.shape == (T * topk, I)
    x64 = x.double()
    y64 = torch.zeros((T, H), dtype=torch.float64, device=DEV)
    A = torch.zeros_like(y64)
    valid = (idx >= 0) & (idx < q.num_experts)
    assert torch.equal(pos >= 0, valid)
    assert sorted(pos[valid].tolist()) == list(range(int(valid.sum())))           # the sorted rows in use are 0 .. count - 1, each once
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
    print(f"moe batch T={T} bits={q.bits} {str(dtype)[6:]}: worst err/bound H {worst_h:.3f} out {worst_o:.3f}")
    assert bool((err <= bound).all()), f"out: worst err/bound {worst_o:.3f}"
    return out, hs, pos


SHAPES = [(8, 2, 256, 512), (60, 4, 2048, 1408)]
TS = (5, 7, 16, 33, 64)


@pytest.mark.parametrize("shape", SHAPES, ids=["e8", "e60"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [32, 128, -1])
@pytest.mark.parametrize("bits", [4, 8])
def test_parity_grid(bits, gs, act, dtype, shape):
    E, topk, H, I = shape
    q = make_experts(E, H, I, bits, gs, act, dtype, seed=bits + gs + E, top_k=topk)
    for T in TS:
        idx, w = _routing(T, E, topk, T + E)
        check(q, _x(T, H, dtype, T), idx, w, dtype, act)


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
def test_mixtral_8x7b_block(act):
    """H 4096, I 14336, E 8, topk 2, 4-bit g128 fp16."""
    dtype = torch.float16
    q = make_experts(8, 4096, 14336, 4, 128, act, dtype, seed=11)
    for T in (8, 64):
        idx, w = _routing(T, 8, 2, T)
        check(q, _x(T, 4096, dtype, T), idx, w, dtype, act)


def test_routing_edge_cases():
    dtype = torch.float16
    q = make_experts(8, 256, 512, 4, 128, False, dtype, seed=3)
    T = 50
    x = _x(T, 256, dtype, 1)
    w = torch.full((T, 2), 0.5, device=DEV)
    # every token to the same two experts: each gets 50 rows = tiles of 16, 16, 16 and 2
    idx = torch.tensor([[5, 2]] * T, dtype=torch.int64, device=DEV)
    check(q, x, idx, w, dtype)
    # an expert with exactly 16 rows and one with 17 (a full tile; a full tile and a tile of one row)
    first = [3] * 16 + [6] * 17 + [0] * 17
    idx = torch.tensor([[a, 7] for a in first], dtype=torch.int64, device=DEV)
    check(q, x, idx, w, dtype)
    # indices == E and -1 are dropped; a token with none left gets exactly 0 and pos == -1
    T = 6
    x, w = x[:T], w[:T]
    idx = torch.tensor([[8, 3], [1, -1], [8, -1], [6, 0], [2, 2], [3, 1]], dtype=torch.int64, device=DEV)
    out, _, pos = check(q, x, idx, w, dtype)
    assert pos[2].tolist() == [-1, -1] and pos[0, 0].item() == -1 and pos[1, 1].item() == -1
    assert bool((out[2] == 0).all()) and bool((out[0] != 0).any())
    # a repeated expert within a token's top-k counts twice
    idx = torch.tensor([[4, 4], [1, 1], [7, 7], [0, 0], [5, 5], [2, 2]], dtype=torch.int64, device=DEV)
    out2, _, pos2 = check(q, x, idx, w, dtype)
    assert bool((pos2[:, 0] != pos2[:, 1]).all())
    with torch.no_grad():
        single = moe_forward(q, x, idx[:, :1], torch.ones((T, 1), device=DEV))
    assert q.last_plan["path"] == "batch"
    assert torch.allclose(out2.float(), single.float(), rtol=1e-2, atol=1e-3)


def test_reproducible_permutation_invariant_and_row_independent():
    dtype = torch.bfloat16
    q = make_experts(60, 2048, 1408, 4, 128, True, dtype, seed=5, top_k=4)
    T = 40
    x = _x(T, 2048, dtype, 9)
    idx, w = _routing(T, 60, 4, 9)
    with torch.no_grad():
        a = moe_forward(q, x, idx, w)
        b = moe_forward(q, x, idx, w)
        p = torch.randperm(T, generator=torch.Generator().manual_seed(4)).to(DEV)
        c = moe_forward(q, x[p], idx[p], w[p])
        five = moe_forward(q, x[:5], idx[:5], w[:5])
    assert q.last_plan["path"] == "batch"
    assert torch.equal(a, b)
    assert torch.equal(a[p], c)
    assert torch.equal(a[:5], five)


def test_batch_agrees_with_grouped_and_per_expert_and_allocates_nothing():
    from autogptq_amd.moe import _per_expert
    from autogptq_amd.model_utils import autogptq_post_init
    dtype = torch.float16
    q = make_experts(8, 256, 512, 4, 64, False, dtype, seed=8)
    plain = make_experts(8, 256, 512, 4, 64, False, dtype, seed=8, batch=False)
    autogptq_post_init(torch.nn.Sequential(q), max_input_length=64, expert_batched_decode=True)
    autogptq_post_init(torch.nn.Sequential(plain), max_input_length=64)
    for T in (5, 16, 64):
        x = _x(T, 256, dtype, T)
        idx, w = _routing(T, 8, 2, T)
        assert q.plan(T)["path"] == "batch" and plain.plan(T)["path"] == "grouped"
        with torch.no_grad():
            ref = _per_expert(plain, x, idx, w)
            grouped = moe_forward(plain, x, idx, w)
            moe_forward(q, x, idx, w)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            out = moe_forward(q, x, idx, w)
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated() - before
        assert q.last_plan["path"] == "batch" and plain.last_plan["path"] == "grouped"
        assert grown <= out.numel() * out.element_size() + 512, grown
        assert torch.allclose(out.float(), grouped.float(), rtol=2e-2, atol=2e-3), float((out.float() - grouped.float()).abs().max())
        assert torch.allclose(out.float(), ref.float(), rtol=2e-2, atol=2e-3), float((out.float() - ref.float()).abs().max())


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
def test_graph_capture_replays_with_new_inputs(act):
    dtype = torch.float16
    q = make_experts(8, 256, 512, 8 if act else 4, 32, act, dtype, seed=4)
    T = 24
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
    assert q.last_plan["path"] == "batch"
    for r in range(3):
        xn = _x(T, 256, dtype, r)
        idn, wn = _routing(T, 8, 2, 100 + r)
        x.copy_(xn), idx.copy_(idn), w.copy_(wn)
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = moe_forward(q, xn, idn, wn)
        assert torch.equal(out, eager), r


def test_defaults_are_unchanged_and_decode_keeps_its_band():
    dtype = torch.float16
    plain = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, batch=False)
    copy = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, decode_copy=True, batch=False)
    both = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, decode_copy=False, batch=True)      # batch builds the copy and its table
    T = 64
    x = _x(T, 256, dtype, 2)
    idx, w = _routing(T, 8, 2, 2)
    assert plain.plan(T)["path"] == "grouped" and copy.plan(T)["path"] == "grouped" and both.plan(T)["path"] == "batch"
    assert copy.plan(5)["path"] == "grouped" and both.plan(5)["path"] == "batch"
    with torch.no_grad():
        assert torch.equal(moe_forward(plain, x, idx, w), moe_forward(copy, x, idx, w))
    assert copy.last_plan["path"] == "grouped"
    for t in (1, 2, 3, 4):
        assert both.plan(t)["path"] == "decode" and copy.plan(t)["path"] == "decode"
    assert both.plan(65)["path"] == "grouped"
    assert both.decode_copy_bytes == copy.decode_copy_bytes > 0
    both.batch_max_tokens = 16                                       # the band can be narrowed per module
    assert both.plan(16)["path"] == "batch" and both.plan(17)["path"] == "grouped"
    # experts the batch plan declines behave as without the flag
    odd = make_experts(8, 256, 192, 4, 64, False, dtype, seed=1, batch=True)       # I = 192 is not a multiple of 128
    assert odd.plan(16)["path"] == "grouped" and odd.decode_copy_bytes == 0


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
    autogptq_post_init(model, max_input_length=64, expert_batched_decode=True)
    return TM, model, twin


@pytest.mark.parametrize("desc_act", [False, True])
def test_tiny_mixtral_end_to_end(tmp_path, desc_act):
    """A prompt of 12 tokens runs the batch path in every MoE layer and each layer agrees with the fp16 twin's MixtralExperts on the same inputs at the
    tolerance of test_gpu_moe.test_tiny_mixtral_end_to_end; the decode steps of generate still run the decode path."""
    TM, model, twin = _tiny(tmp_path, desc_act)
    experts = [layer.mlp.experts for layer in model.model.layers]
    ids = torch.randint(0, 512, (1, 12), generator=torch.Generator().manual_seed(0)).to(DEV)
    seen = []
    hooks = [ex.register_forward_hook(lambda m, args, out: seen.append((m, args, out, dict(m.last_plan)))) for ex in experts]
    with torch.no_grad():
        logits = model(ids).logits.float()
    assert torch.isfinite(logits).all()
    assert len(seen) == len(experts) and all(s[3]["path"] == "batch" for s in seen), [s[3] for s in seen]
    for m, (hs, idx, w), out, _ in seen:
        li = experts.index(m)
        with torch.no_grad():
            ref = twin.model.layers[li].mlp.experts(hs, idx, w)
        err = (out.float() - ref.float()).abs().max().item()
        assert err <= 1e-2 * max(1.0, ref.abs().max().item()), (li, err)
    del seen[:]
    with torch.no_grad():
        ga = model.generate(ids, max_new_tokens=4, do_sample=False)
    for h in hooks:
        h.remove()
    assert ga.shape == (1, 16)
    steps = [s for s in seen if s[1][0].reshape(-1, s[1][0].shape[-1]).shape[0] == 1]
    assert len(steps) >= 2 * 3 and all(s[3]["path"] == "decode" for s in steps), [s[3] for s in seen]
