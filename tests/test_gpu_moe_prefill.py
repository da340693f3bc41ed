"""GPU: the prefill path of the routed mixture-of-experts layers (gptq_moe_prefill_forward through QuantMoEExperts.post_init(prefill=True) / moe_forward):
65 tokens and more on the experts' decode copy, 64-row panels of one expert over the whole K, five launches (six with act-order down projections).

Its arithmetic contract is the grouped path's (every W bit-exact to dequantize(), fp32 products and sums on the matrix core, h rounded once), so every output
is checked as tests/test_gpu_moe_batch.py checks the batch path, with the error model of test_gpu_error_model.py and no new constant:

    |y - y64|  <=  (1/2 + 1/64) ulp(y64)  +  C sqrt(K) 2^-24 A,      A = |a| @ |W|,   W = dequantize(),   C = 16

C = 16 is the project's constant for matrix-core chains over a whole K.  H is checked against silu(g64) * u64 with the bound propagated through silu * mul,
out against the fp64 product of the kernel's OWN H rows.  Every output is checked.

Shapes (E, topk, H, I): (8, 2, 256, 512) -- 4 k-steps for the pair stage's waves (waves run empty), exactly one per wave in the down stage;
(60, 4, 512, 384) -- every tile partial, 6 down steps; (4, 2, 2048, 768) -- several steps per wave, 12 down steps (the last two waves empty), group
boundaries inside a wave's range at g64 / g128."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _guarded as G  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.moe import QuantMoEExperts, moe_forward  # noqa: E402
from test_gpu_moe import _fill, _routing, _ulp, _w64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 16.0
SHAPES = [(8, 2, 256, 512), (60, 4, 512, 384), (4, 2, 2048, 768)]
WORST = {"H": 0.0, "out": 0.0}


def make_experts(E, H, I, bits, gs, act, dtype, seed=0, top_k=2, prefill=True, **kw):
    gen = torch.Generator().manual_seed(seed)
    q = QuantMoEExperts(E, H, I, bits, gs, top_k=top_k, weight_dtype=dtype)
    for e in range(E):
        for l in q[e].layers():
            _fill(l, gen, act)
    q = q.to(DEV)
    q.post_init(prefill=prefill, **kw)
    return q


def _x(T, H, dtype, seed):
    return (torch.rand((T, H), generator=torch.Generator().manual_seed(seed)) - 0.5).to(dtype).to(DEV)


def _weights(q, e):
    """The fp64 weights of expert e, computed once per experts object."""
    cache = q.__dict__.setdefault("_w64_cache", {})
    if e not in cache:
        cache[e] = tuple(_w64(l) for l in q[e].layers())
    return cache[e]


def verify(q, x, idx, w, dtype, out, hs, pos, tag="prefill"):
    """H and out of one call against the fp64 oracles: every output, the bounds of the module docstring."""
    T, topk = idx.shape
    H, I = q.hidden_dim, q.intermediate_dim
    assert out.shape == (T, H) and out.dtype == dtype and hs.shape == (T * topk, I)
    x64 = x.double()
    y64 = torch.zeros((T, H), dtype=torch.float64, device=DEV)
    A = torch.zeros_like(y64)
    valid = (idx >= 0) & (idx < q.num_experts)
    assert torch.equal(pos >= 0, valid)
    assert sorted(pos[valid].tolist()) == list(range(int(valid.sum())))           # the sorted rows in use are 0 .. count - 1, each once
    worst_h = 0.0
    for e in sorted(set(idx[valid].tolist())):
        tok, j = torch.where(idx == e)
        W1, W3, W2 = _weights(q, e)
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
    WORST["H"], WORST["out"] = max(WORST["H"], worst_h), max(WORST["out"], worst_o)
    print(f"moe {tag} T={T} bits={q.bits} {str(dtype)[6:]}: worst err/bound H {worst_h:.3f} out {worst_o:.3f}  (so far: H {WORST['H']:.3f} out {WORST['out']:.3f})")
    assert bool((err <= bound).all()), f"out: worst err/bound {worst_o:.3f}"


def check(q, x, idx, w, dtype):
    """Run the prefill path with its intermediate and check H and out against the fp64 oracles; returns (out, H, pos)."""
    T, topk = idx.shape
    plan = q.plan(T, topk)
    gate, up, down = q.projections()
    launches = 5 + int(any(l._layer.perm for l in down))       # (a shuffled g_idx of ONE group is sequential: no perm)
    R = T * topk
    assert plan["path"] == "prefill" and plan["bm"] == 64 and plan["launches"] == launches, plan
    assert plan["tiles"] == R // 64 + min(q.num_experts, R) and plan["waves"] == 8, plan
    assert plan["waves_pair"] == (4 if any(l._layer.perm for l in gate + up) else 8), plan
    with torch.no_grad():
        out, hs, pos = moe_forward(q, x, idx, w, return_intermediate=True)
    assert q.last_plan["path"] == "prefill"
    verify(q, x, idx, w, dtype, out, hs, pos)
    return out, hs, pos


@pytest.mark.parametrize("shape", SHAPES, ids=["e8", "e60", "e4"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [64, 128, -1])
@pytest.mark.parametrize("bits", [4, 8])
def test_parity_grid(bits, gs, act, dtype, shape):
    E, topk, H, I = shape
    q = make_experts(E, H, I, bits, gs, act, dtype, seed=bits + gs + E, top_k=topk)
    for T in (65, 100, 129, 300) + ((520,) if E == 4 else ()):      # 520 on four experts: four full tiles plus a short one per expert
        idx, w = _routing(T, E, topk, T + E)
        check(q, _x(T, H, dtype, T), idx, w, dtype)


def test_routing_edge_cases():
    dtype = torch.float16
    E, topk, H, I = SHAPES[0]
    q = make_experts(E, H, I, 4, 128, False, dtype, seed=3)
    T = 130
    x = _x(T, H, dtype, 1)
    w = torch.full((T, 2), 0.5, device=DEV)
    # every token to the same two experts: each gets 130 rows = tiles of 64, 64 and 2; six experts nobody picks
    idx = torch.tensor([[5, 2]] * T, dtype=torch.int64, device=DEV)
    check(q, x, idx, w, dtype)
    # an expert with exactly 64 rows and one with 65 (a full tile; a full tile and a tile of one row); expert 4 is picked by nobody
    first = [3] * 64 + [6] * 65 + [0]
    idx = torch.tensor([[a, 7] for a in first], dtype=torch.int64, device=DEV)
    check(q, x, idx, w, dtype)
    # indices == E and -1 are dropped; a token with none left gets exactly 0 and pos == -1
    idx, _ = _routing(T, E, topk, 17)
    idx[0] = torch.tensor([8, 3], device=DEV)
    idx[1] = torch.tensor([1, -1], device=DEV)
    idx[2] = torch.tensor([8, -1], device=DEV)
    idx[3::7, 0] = E
    out, _, pos = check(q, x, idx, w, dtype)
    assert pos[2].tolist() == [-1, -1] and pos[0, 0].item() == -1 and pos[1, 1].item() == -1
    assert bool((out[2] == 0).all()) and bool((out[0] != 0).any())
    # a repeated expert within a token's top-k counts twice
    idx = torch.tensor([[t % E, t % E] for t in range(T)], dtype=torch.int64, device=DEV)
    out2, _, pos2 = check(q, x, idx, w, dtype)
    assert bool((pos2[:, 0] != pos2[:, 1]).all())
    with torch.no_grad():
        single = moe_forward(q, x, idx[:, :1], torch.ones((T, 1), device=DEV))
    assert q.last_plan["path"] == "prefill"
    assert torch.allclose(out2.float(), single.float(), rtol=1e-2, atol=1e-3)


def _direct(q, x, idx, w, dtype, guarded=False):
    """One gptq_moe_prefill_forward call on the C ABI (any T); guarded: every buffer inside guard bands, the workspace exactly its query."""
    lib = _lib.load()
    T, topk = idx.shape
    H, I = q.hidden_dim, q.intermediate_dim
    es, R = x.element_size(), T * topk
    m = ctypes.byref(q._moe)
    need = int(lib.gptq_moe_prefill_workspace_bytes(m, T, topk))
    assert need > 0
    st = torch.cuda.current_stream(DEV).cuda_stream
    if not guarded:
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        out = torch.empty((T, H), dtype=dtype, device=DEV)
        hb = torch.empty(R * I * es + 4 * R, dtype=torch.uint8, device=DEV)
        _lib.check(lib.gptq_moe_prefill_forward(m, q._decode_table.data_ptr(), x.data_ptr(), idx.data_ptr(), w.data_ptr(), T, topk, out.data_ptr(), hb.data_ptr(),
                                                ws.data_ptr(), need, st))
        body = hb
    else:
        gx, _ = G.guarded_like(x, G.guard_for(H * es))
        gi, _ = G.guarded_like(idx, G.guard_for(topk * 8))
        gw, _ = G.guarded_like(w, G.guard_for(topk * 4))
        ws = G.Guarded(need, max(64 << 10, (need + 255) // 256 * 256), 0x00, G.OUT_GUARD, DEV)
        go = G.Guarded(T * H * es, G.guard_for(H * es), 0xFF, G.OUT_GUARD, DEV)
        gh = G.Guarded(R * I * es + 4 * R, G.guard_for(I * es), 0xFF, G.OUT_GUARD, DEV)
        _lib.check(lib.gptq_moe_prefill_forward(m, q._decode_table.data_ptr(), gx.ptr, gi.ptr, gw.ptr, T, topk, go.ptr, gh.ptr, ws.ptr, need, st))
        for g, nm in ((gx, "x"), (gi, "topk_idx"), (gw, "topk_w"), (go, "out"), (gh, "h_out"), (ws, f"workspace ({need} bytes = its query)")):
            g.assert_intact(f"gptq_moe_prefill_forward T={T}: {nm}")
        out, body = go.view(dtype, (T, H)), gh.body
    hs = body[:R * I * es].view(dtype).view(R, I)
    pos = body[R * I * es:].view(torch.int32).view(T, topk)
    return out, hs, pos


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
def test_c_abi_takes_any_token_count(act):
    dtype = torch.float16
    E, topk, H, I = SHAPES[0]
    q = make_experts(E, H, I, 4, 64, act, dtype, seed=12)
    lib = _lib.load()
    for T in (1, 7):
        x = _x(T, H, dtype, T)
        idx, w = _routing(T, E, topk, T)
        out, hs, pos = _direct(q, x, idx, w, dtype)
        verify(q, x, idx, w, dtype, out, hs, pos, tag="prefill (C ABI)")
    # T = 0: success, nothing written
    canary = torch.full((64,), 0x5A, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(q._moe), 1, topk)), dtype=torch.uint8, device=DEV)
    rc = lib.gptq_moe_prefill_forward(ctypes.byref(q._moe), q._decode_table.data_ptr(), canary.data_ptr(), canary.data_ptr(), canary.data_ptr(), 0, topk,
                                      canary.data_ptr(), None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool((canary == 0x5A).all()) and not bool(ws.any())


def test_row_independence_and_reproducibility():
    """A token's output bits depend only on its own x, indices and weights: 200 tokens in one call = the same tokens in two calls of 100."""
    dtype = torch.bfloat16
    E, topk, H, I = SHAPES[2]
    q = make_experts(E, H, I, 4, 128, True, dtype, seed=5, top_k=topk)
    T = 200
    x = _x(T, H, dtype, 9)
    idx, w = _routing(T, E, topk, 9)
    with torch.no_grad():
        a = moe_forward(q, x, idx, w)
        b = moe_forward(q, x, idx, w)
        lo = moe_forward(q, x[:100], idx[:100], w[:100])
        hi = moe_forward(q, x[100:].contiguous(), idx[100:].contiguous(), w[100:].contiguous())
    assert q.last_plan["path"] == "prefill"
    assert torch.equal(a, b)
    assert torch.equal(a[:100], lo) and torch.equal(a[100:], hi)


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
def test_graph_capture_replays_bit_equal(act):
    dtype = torch.float16
    E, topk, H, I = SHAPES[0]
    q = make_experts(E, H, I, 8 if act else 4, 64, act, dtype, seed=4)
    T = 100
    x = torch.zeros((T, H), dtype=dtype, device=DEV)
    idx = torch.zeros((T, topk), dtype=torch.int64, device=DEV)
    w = torch.zeros((T, topk), dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        moe_forward(q, x, idx, w)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = moe_forward(q, x, idx, w)
    assert q.last_plan["path"] == "prefill"
    for r in range(2):                                     # new inputs and a new routing per replay: the grid is a bound, the tile table is rebuilt on the device
        xn = _x(T, H, dtype, r)
        idn, wn = _routing(T, E, topk, 100 + r)
        x.copy_(xn), idx.copy_(idn), w.copy_(wn)
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = moe_forward(q, xn, idn, wn)
        assert torch.equal(out, eager), r


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
def test_memory_contract(act):
    """x, topk_idx, topk_w, out, h_out and a workspace of exactly gptq_moe_prefill_workspace_bytes inside guard bands: all guards intact, same bits as moe_forward."""
    dtype = torch.float16
    E, topk, H, I = SHAPES[0]
    q = make_experts(E, H, I, 4, 128, act, dtype, seed=6)
    for T in (65, 129):
        x = _x(T, H, dtype, T)
        idx, w = _routing(T, E, topk, T)
        idx[::5, 0] = E                                    # dropped assignments: sorted rows past the count stay unwritten and unread
        with torch.no_grad():
            y_mod, hs_mod, pos_mod = moe_forward(q, x, idx, w, return_intermediate=True)
        assert q.last_plan["path"] == "prefill"
        out, hs, pos = _direct(q, x, idx, w, dtype, guarded=True)
        valid = pos_mod >= 0
        assert torch.equal(out, y_mod) and torch.equal(pos, pos_mod)
        assert torch.equal(hs[pos[valid].long()], hs_mod[pos_mod[valid].long()])


def test_defaults_are_unchanged_and_the_lower_bands_keep_their_paths():
    from autogptq_amd.model_utils import autogptq_post_init
    dtype = torch.float16
    E, topk, H, I = SHAPES[0]
    plain = make_experts(E, H, I, 4, 128, False, dtype, seed=7, prefill=False)
    pre = make_experts(E, H, I, 4, 128, False, dtype, seed=7)                     # prefill builds the copy and its table
    both = make_experts(E, H, I, 4, 128, False, dtype, seed=7, batch=True)
    assert plain.plan(300)["path"] == "grouped" and plain.decode_copy_bytes == 0
    assert pre.plan(300)["path"] == "prefill" and pre.plan(65)["path"] == "prefill" and pre.decode_copy_bytes > 0
    for t in (1, 4):
        assert pre.plan(t)["path"] == "decode" and both.plan(t)["path"] == "decode"
    for t in (5, 64):
        assert pre.plan(t)["path"] == "grouped" and both.plan(t)["path"] == "batch"
    assert both.plan(65)["path"] == "prefill"
    assert pre.workspace_bytes(300) == int(_lib.load().gptq_moe_prefill_workspace_bytes(ctypes.byref(pre._moe), 300, topk))
    # agrees with the grouped path of the same weights; under grad nothing changes
    T = 150
    x = _x(T, H, dtype, 2)
    idx, w = _routing(T, E, topk, 2)
    with torch.no_grad():
        a, b = moe_forward(pre, x, idx, w), moe_forward(plain, x, idx, w)
    assert pre.last_plan["path"] == "prefill" and plain.last_plan["path"] == "grouped"
    assert torch.allclose(a.float(), b.float(), rtol=2e-2, atol=2e-3), float((a.float() - b.float()).abs().max())
    xg = x.clone().requires_grad_(True)
    moe_forward(pre, xg, idx, w)
    assert pre.last_plan["path"] == "per_expert"
    # experts the prefill plan declines behave as without the flag
    odd = make_experts(E, H, 192, 4, 64, False, dtype, seed=1)                    # I = 192 is not a multiple of 128
    assert odd.plan(300)["path"] == "grouped" and odd.decode_copy_bytes == 0
    g32 = make_experts(E, H, I, 4, 32, False, dtype, seed=1)                      # 32-wide groups
    assert g32.plan(300)["path"] == "grouped" and g32.decode_copy_bytes == 0
    # the model-level switch reserves the path's scratch: the call allocates nothing but its output
    autogptq_post_init(torch.nn.Sequential(pre), max_input_length=300, expert_prefill=True)
    assert pre.plan(300)["path"] == "prefill"
    x, (idx, w) = _x(300, H, dtype, 3), _routing(300, E, topk, 3)
    with torch.no_grad():
        moe_forward(pre, x, idx, w)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = moe_forward(pre, x, idx, w)
        torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - before <= out.numel() * out.element_size() + 512
