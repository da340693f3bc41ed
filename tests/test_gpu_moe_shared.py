"""GPU: the shared expert of a Qwen-MoE block fused into the two decode launches (gptq_moe_shared_decode_forward through moe_shared_forward), the any-T tail
(gptq_moe_shared_combine), and both behind inject_shared_expert on a tiny Qwen2-MoE.

The fused call keeps the arithmetic of the decode path, so it is checked with that path's error model (test_gpu_moe_decode.py):

    |y - y64|  <=  (1/2 + 1/64) ulp(y64)  +  C sqrt(K) 2^-24 A,      A = |a| @ |W64|,   C = 4,   W64 = scales (w - z) in fp64, UNROUNDED

* routed H rows and the shared Hs rows against silu(g64) * u64, with the bound test_gpu_moe_decode.check propagates through silu * mul;
* the gate scalar: l = T(x . w_g) carries (1/2 + 1/64) ulp_T(l64) + C sqrt(H) 2^-24 sum|x||w_g|; the sigmoid's Lipschitz constant is 1/4, and 1e-6 is the
  slack the silu check already gives the fast exponential:   |s - sigmoid(l64)| <= 1/4 ((1/2 + 1/64) ulp_T(l64) + C sqrt(H) 2^-24 sum|x||w_g|) + 1e-6;
* out against the fp64 value built from the kernel's OWN H, Hs and s:  y64 = sum_j w_j (H_j @ W2_e) + s (Hs @ W2_s),
  bound (1/2 + 1/64) ulp(y64) + C 2^-24 (sqrt(I) A_routed + sqrt(I_s) A_shared)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _guarded as G  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.moe import _shared_state, moe_forward, moe_shared_forward, shared_plan, shared_workspace_bytes  # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear  # noqa: E402
from test_gpu_moe import _fill, _routing, _ulp  # noqa: E402
from test_gpu_moe_decode import C, _w64, _x, make_experts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGE = (8, 2, 256, 512, 320)


def make_block(E, topk, H, I, Is, bits, gs, act, dtype, seed=0, zero_shared_down=False):
    """(routed experts with their decode copy, the shared (gate, up, down) QuantLinears, the gate vector [1, H])."""
    q = make_experts(E, H, I, bits, gs, act, dtype, seed=seed, top_k=topk)
    q.shared_decode_max_tokens = 4      # the kernels' whole range (moe_shared_forward's default stops where the fused call was measured the fastest form)
    gen = torch.Generator().manual_seed(seed + 1000)
    layers = []
    for k, n in ((H, Is), (H, Is), (Is, H)):
        l = QuantLinear(bits, gs, k, n, False, weight_dtype=dtype)
        _fill(l, gen, act)
        layers.append(l)
    if zero_shared_down:
        layers[2].scales = torch.zeros_like(layers[2].scales)
    layers = tuple(l.to(DEV) for l in layers)
    for l in layers:
        l.post_init()
    gw = ((torch.rand((1, H), generator=gen) - 0.5) * 0.25).to(dtype).to(DEV)
    return q, layers, gw


def _silu_mul_bound(x64, W1, W3, K, dtype):
    g64, u64 = x64 @ W1, x64 @ W3
    Eg = C * K ** 0.5 * 2.0 ** -24 * (x64.abs() @ W1.abs())
    Eu = C * K ** 0.5 * 2.0 ** -24 * (x64.abs() @ W3.abs())
    s64 = g64 * torch.sigmoid(g64)
    h64 = s64 * u64
    return h64, (0.5 + 1 / 64) * _ulp(h64, dtype) + 1.1 * Eg * (u64.abs() + Eu) + s64.abs() * Eu + 1e-6 * h64.abs() + 1e-30


def _gate_bound(x64, gw64, H, dtype):
    """(sigmoid(l64), the bound on |s - sigmoid(l64)|)."""
    l64 = x64 @ gw64
    bound = 0.25 * ((0.5 + 1 / 64) * _ulp(l64, dtype) + C * H ** 0.5 * 2.0 ** -24 * (x64.abs() @ gw64.abs())) + 1e-6
    return torch.sigmoid(l64), bound


def check(q, layers, gw, x, idx, w, dtype):
    """Run the fused call with its intermediates and check H, Hs, s and out against the fp64 oracles; returns (out, H, pos, Hs, s)."""
    T, topk = idx.shape
    plan = shared_plan(q, layers, T, topk)
    assert plan["path"] == "decode_shared" and plan["launches"] == 2, plan
    with torch.no_grad():
        out, hs, pos, hss, s = moe_shared_forward(q, layers, gw, x, idx, w, return_intermediate=True)
    assert q.last_plan["path"] == "decode" and q.last_plan["shared"] == "decode"
    H, I, Is = q.hidden_dim, q.intermediate_dim, layers[0].outfeatures
    assert out.shape == (T, H) and out.dtype == dtype and hs.shape == (T * topk, I) and hss.shape == (T, Is) and s.shape == (T,) and s.dtype == torch.float32
    x64 = x.double()
    y64 = torch.zeros((T, H), dtype=torch.float64, device=DEV)
    A_r = torch.zeros_like(y64)
    valid = (idx >= 0) & (idx < q.num_experts)
    want_pos = torch.where(valid, torch.arange(T * topk, device=DEV, dtype=torch.int32).view(T, topk), torch.full_like(pos, -1))
    assert torch.equal(pos, want_pos)
    worst = {"H": 0.0, "Hs": 0.0, "s": 0.0, "out": 0.0}
    for e in sorted(set(idx[valid].tolist())):
        tok, j = torch.where(idx == e)
        gate, up, down = q[e].layers()
        h64, bound_h = _silu_mul_bound(x64[tok], _w64(gate), _w64(up), H, dtype)
        hk = hs[pos[tok, j].long()].double()
        err = (hk - h64).abs()
        worst["H"] = max(worst["H"], float((err / bound_h).max()))
        assert bool((err <= bound_h).all()), f"H expert {e}: worst err/bound {float((err / bound_h).max()):.3f}"
        W2 = _w64(down)
        wj = w[tok, j].double()[:, None]
        y64.index_add_(0, tok, wj * (hk @ W2))
        A_r.index_add_(0, tok, wj.abs() * (hk.abs() @ W2.abs()))
    # the shared expert's rows
    h64, bound_h = _silu_mul_bound(x64, _w64(layers[0]), _w64(layers[1]), H, dtype)
    err = (hss.double() - h64).abs()
    worst["Hs"] = float((err / bound_h).max())
    assert bool((err <= bound_h).all()), f"Hs: worst err/bound {worst['Hs']:.3f}"
    # the gate scalar
    s_ref, bound_s = _gate_bound(x64, gw.double().reshape(-1), H, dtype)
    err = (s.double() - s_ref).abs()
    worst["s"] = float((err / bound_s).max())
    assert bool((err <= bound_s).all()), f"s: worst err/bound {worst['s']:.3f}"
    # out from the kernel's own H, Hs and s
    W2s = _w64(layers[2])
    s64 = s.double()[:, None]
    y64 = y64 + s64 * (hss.double() @ W2s)
    A_s = s64.abs() * (hss.double().abs() @ W2s.abs())
    bound = (0.5 + 1 / 64) * _ulp(y64, dtype) + C * 2.0 ** -24 * (I ** 0.5 * A_r + Is ** 0.5 * A_s) + 1e-30
    err = (out.double() - y64).abs()
    worst["out"] = float((err / bound).max())
    print(f"moe shared T={T} bits={q.bits} {str(dtype)[6:]} I_s={Is}: worst err/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert bool((err <= bound).all()), f"out: worst err/bound {worst['out']:.3f}"
    return out, hs, pos, hss, s


SHAPES = [(8, 2, 256, 512, 1024, 128), (8, 2, 256, 512, 1024, -1), (8, 2, 256, 512, 320, 32), (8, 2, 256, 512, 320, 64), (60, 4, 2048, 1408, 5632, 128)]


@pytest.mark.parametrize("shape", SHAPES, ids=["is1024-g128", "is1024-gfull", "is320-g32", "is320-g64", "a2.7b"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("bits", [4, 8])
def test_decode_parity_grid(bits, act, dtype, shape):
    E, topk, H, I, Is, gs = shape
    q, layers, gw = make_block(E, topk, H, I, Is, bits, gs, act, dtype, seed=bits + gs + E)
    for T in (1, 2, 3, 4):
        idx, w = _routing(T, E, topk, T + E)
        check(q, layers, gw, _x(T, H, dtype, T), idx, w, dtype)


def _c_call(q, layers, gate_ptr, x, idx, w, guarded=False):
    """gptq_moe_shared_decode_forward through the C ABI (gate_ptr: a device pointer or None); returns (out, Hs, s) -- with ``guarded`` every buffer sits
    between guard bands and the workspace has exactly the queried size."""
    lib = _lib.load()
    T, topk = idx.shape
    H, I, Is = q.hidden_dim, q.intermediate_dim, layers[0].outfeatures
    dtype = x.dtype
    es, R = x.element_size(), T * topk
    sh, _ = _shared_state(q, layers)
    sh.gate_w = gate_ptr
    mp, sp = ctypes.byref(q._moe), ctypes.byref(sh)
    need = int(lib.gptq_moe_shared_decode_workspace_bytes(mp, sp, T, topk))
    assert need > 0
    hb = R * I * es + 4 * R + T * Is * es + 4 * T
    stream = torch.cuda.current_stream(DEV).cuda_stream
    if guarded:
        gx, _ = G.guarded_like(x, G.guard_for(H * es))
        gi, _ = G.guarded_like(idx, G.guard_for(topk * 8))
        gwt, _ = G.guarded_like(w, G.guard_for(topk * 4))
        go = G.Guarded(T * H * es, G.guard_for(H * es), 0xFF, G.OUT_GUARD, DEV)
        gh = G.Guarded(hb, G.guard_for(Is * es), 0xFF, G.OUT_GUARD, DEV)
        ws = G.Guarded(need, max(64 << 10, (need + 255) // 256 * 256), 0x00, G.OUT_GUARD, DEV)
        _lib.check(lib.gptq_moe_shared_decode_forward(mp, sp, q._decode_table.data_ptr(), gx.ptr, gi.ptr, gwt.ptr, T, topk, go.ptr, gh.ptr, ws.ptr, need, stream))
        for g, nm in ((gx, "x"), (gi, "topk_idx"), (gwt, "topk_w"), (go, "out"), (gh, "h_out"), (ws, f"workspace ({need} bytes = its query)")):
            g.assert_intact(f"gptq_moe_shared_decode_forward T={T}: {nm}")
        out, body = go.view(dtype, (T, H)).clone(), gh.body.clone()
    else:
        out = torch.empty((T, H), dtype=dtype, device=DEV)
        body = torch.empty(hb, dtype=torch.uint8, device=DEV)
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        _lib.check(lib.gptq_moe_shared_decode_forward(mp, sp, q._decode_table.data_ptr(), x.data_ptr(), idx.data_ptr(), w.data_ptr(), T, topk, out.data_ptr(),
                                                      body.data_ptr(), ws.data_ptr(), need, stream))
    torch.cuda.synchronize()
    o2 = R * I * es + 4 * R
    return out, body[o2:o2 + T * Is * es].view(dtype).view(T, Is), body[o2 + T * Is * es:].view(torch.float32)


def test_edge_cases():
    dtype = torch.float16
    E, topk, H, I, Is = EDGE
    q, layers, gw = make_block(E, topk, H, I, Is, 4, 64, False, dtype, seed=3)
    T = 4
    x = _x(T, H, dtype, 1)
    idx, w = _routing(T, E, topk, 5)
    # every routed index dropped: each token gets exactly T(s * y_s) -- the bits of a call whose routed terms are exact zeros
    dropped = torch.tensor([[E, -1]] * T, dtype=torch.int64, device=DEV)
    out_d, _, pos, hss, s = check(q, layers, gw, x, dropped, w, dtype)
    assert bool((pos == -1).all()) and bool((out_d != 0).any())
    with torch.no_grad():
        out_z = moe_shared_forward(q, layers, gw, x, idx, torch.zeros_like(w))
    assert torch.equal(out_d, out_z)
    # ... and the value: y_s = hs . W2_s exists only as an fp32 register of the kernel, so T(s * y_s) cannot be rebuilt bit for bit from outside; with
    # gate_w = NULL the same call returns T(y_s), which pins y_s to half an ulp, and T(s * y_s) must lie within its own half ulp of s * T(y_s) +- s ulp / 2
    out_1, _, s_1 = _c_call(q, layers, None, x, dropped, w)
    assert bool((s_1 == 1.0).all())
    y1, s64 = out_1.double(), s.double()[:, None]
    # (the ulp of the larger of the two: s * y and s * T(y) may sit on either side of a power of two; 1.001: s * y is rounded to fp32 first)
    slack = 0.5 * _ulp(torch.maximum((s64 * y1).abs(), out_d.double().abs()), dtype) * 1.001 + s64 * 0.5 * _ulp(y1, dtype)
    assert bool(((out_d.double() - s64 * y1).abs() <= slack).all())
    # a mixed routing: dropped and valid assignments next to the shared term
    mixed = torch.tensor([[E, 3], [1, -1], [E, -1], [6, 0]], dtype=torch.int64, device=DEV)
    check(q, layers, gw, x, mixed, w, dtype)
    # gate_w = NULL through the C ABI: s == 1 exactly, and the rest of the call as with a gate
    out_n, hss_n, s_n = _c_call(q, layers, None, x, idx, w)
    assert bool((s_n == 1.0).all())
    with torch.no_grad():
        _, _, _, hss_g, _ = moe_shared_forward(q, layers, gw, x, idx, w, return_intermediate=True)
    assert torch.equal(hss_n, hss_g)
    # row t of a T = 4 call is bit-equal to the same token alone; two runs are bit-equal
    with torch.no_grad():
        a = moe_shared_forward(q, layers, gw, x, idx, w)
        b = moe_shared_forward(q, layers, gw, x, idx, w)
        rows = [moe_shared_forward(q, layers, gw, x[t:t + 1], idx[t:t + 1], w[t:t + 1]) for t in range(T)]
    assert torch.equal(a, b)
    for t in range(T):
        assert torch.equal(a[t:t + 1], rows[t]), t
    # T = 0: nothing launched, an empty result
    with torch.no_grad():
        out0 = moe_shared_forward(q, layers, gw, x[:0], idx[:0], w[:0])
    assert out0.shape == (0, H)


@pytest.mark.parametrize("Is", [320, 1024], ids=["is320", "is1024"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("bits", [4, 8])
def test_routed_part_is_bit_equal_to_the_decode_path(bits, act, Is):
    """A shared W2 with zero scales makes the shared term an exact zero: the fused call must then return the bits of gptq_moe_decode_forward, whatever the
    wave count the shared segment brings to the workgroup (I_s = 1024: more waves than the routed K = 512 asks for)."""
    dtype = torch.float16
    E, topk, H, I = EDGE[:4]
    q, layers, gw = make_block(E, topk, H, I, Is, bits, 64, act, dtype, seed=7 + bits, zero_shared_down=True)
    for T in (1, 4):
        x = _x(T, H, dtype, T)
        idx, w = _routing(T, E, topk, T + 3)
        with torch.no_grad():
            fused = moe_shared_forward(q, layers, gw, x, idx, w)
            assert q.last_plan["shared"] == "decode"
            routed = moe_forward(q, x, idx, w)
            assert q.last_plan["path"] == "decode"
        assert torch.equal(fused, routed), int((fused != routed).sum())


def _combine(x, gw, ys, out):
    T, H = x.shape
    _lib.check(_lib.load().gptq_moe_shared_combine(x.data_ptr(), gw.data_ptr(), ys.data_ptr(), out.data_ptr(), T, H, _lib.DTYPE_ENUM[x.dtype],
                                                   torch.cuda.current_stream(DEV).cuda_stream))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("H", [256, 2048])
def test_combine_kernel(H, dtype):
    gen = torch.Generator().manual_seed(H)
    gw = ((torch.rand((1, H), generator=gen) - 0.5) * 0.25).to(dtype).to(DEV)
    for T in (1, 5, 64, 65):
        x = _x(T, H, dtype, T)
        ys = ((torch.rand((T, H), generator=gen) - 0.5) * 4).to(dtype).to(DEV)
        out_in = ((torch.rand((T, H), generator=gen) - 0.5) * 4).to(dtype).to(DEV)
        a, b = out_in.clone(), out_in.clone()
        _combine(x, gw, ys, a)
        _combine(x, gw, ys, b)
        assert torch.equal(a, b)
        s_ref, bound_s = _gate_bound(x.double(), gw.double().reshape(-1), H, dtype)
        y64 = out_in.double() + s_ref[:, None] * ys.double()
        bound = (0.5 + 1 / 64) * _ulp(y64, dtype) + bound_s[:, None] * ys.double().abs() + 1e-30
        err = (a.double() - y64).abs()
        print(f"shared combine T={T} H={H} {str(dtype)[6:]}: worst err/bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), float((err / bound).max())
    # T = 0: a no-op that dereferences nothing
    assert _lib.load().gptq_moe_shared_combine(None, None, None, None, 0, H, _lib.DTYPE_ENUM[dtype], None) == 0


def test_combine_and_decode_compute_the_same_gate_scalar():
    """One formula, one order in both kernels: the combine kernel on out = 0, ys = 1 returns T(s), and that is the s the fused call reports, rounded."""
    dtype = torch.bfloat16
    E, topk, H, I, Is = EDGE
    q, layers, gw = make_block(E, topk, H, I, Is, 4, 64, False, dtype, seed=11)
    T = 4
    x = _x(T, H, dtype, 2)
    idx, w = _routing(T, E, topk, 2)
    with torch.no_grad():
        _, _, _, _, s = moe_shared_forward(q, layers, gw, x, idx, w, return_intermediate=True)
    out = torch.zeros((T, H), dtype=dtype, device=DEV)
    _combine(x, gw, torch.ones_like(out), out)
    assert torch.equal(out[:, 0], s.to(dtype)) and bool((out == out[:, :1]).all())


def test_guard_bands():
    dtype = torch.float16
    E, topk, H, I, Is = EDGE
    for bits, act in ((4, True), (8, False)):
        q, layers, gw = make_block(E, topk, H, I, Is, bits, 64, act, dtype, seed=13 + bits)
        ggw, _ = G.guarded_like(gw, G.guard_for(H * 2))
        for T in (1, 4):
            x = _x(T, H, dtype, T)
            idx, w = _routing(T, E, topk, T)
            out_g, _, _ = _c_call(q, layers, ggw.ptr, x, idx, w, guarded=True)
            ggw.assert_intact("gate_w")
            with torch.no_grad():
                assert torch.equal(out_g, moe_shared_forward(q, layers, gw, x, idx, w))
    for T, Hc in ((1, 256), (65, 2048)):
        x = _x(T, Hc, dtype, T)
        ys = _x(T, Hc, dtype, T + 1)
        gwc = _x(1, Hc, dtype, T + 2)
        gx, _ = G.guarded_like(x, G.guard_for(Hc * 2))
        gy, _ = G.guarded_like(ys, G.guard_for(Hc * 2))
        gg, _ = G.guarded_like(gwc, G.guard_for(Hc * 2))
        go, ov = G.guarded_like(ys, G.guard_for(Hc * 2), G.OUT_GUARD)
        _lib.check(_lib.load().gptq_moe_shared_combine(gx.ptr, gg.ptr, gy.ptr, go.ptr, T, Hc, _lib.GPTQ_F16, torch.cuda.current_stream(DEV).cuda_stream))
        for g, nm in ((gx, "x"), (gy, "ys"), (gg, "gate_w"), (go, "out")):
            g.assert_intact(f"gptq_moe_shared_combine T={T}: {nm}")
        ref = ys.clone()
        _combine(x, gwc, ys, ref)
        assert torch.equal(ov, ref)


def test_combine_path_above_four_tokens_and_workspace_is_reserved():
    dtype = torch.float16
    E, topk, H, I, Is = EDGE
    q, layers, gw = make_block(E, topk, H, I, Is, 4, 64, False, dtype, seed=17)
    assert shared_workspace_bytes(q, layers, 4) > q.workspace_bytes(4) and shared_workspace_bytes(q, layers, 5) == 0
    # the default policy: the fused call up to SHARED_DECODE_MAX_TOKENS tokens, the combine form above
    from autogptq_amd.moe import SHARED_DECODE_MAX_TOKENS
    del q.shared_decode_max_tokens
    assert 1 <= SHARED_DECODE_MAX_TOKENS <= 4
    for T in (1, 2, 3, 4):
        idx, w = _routing(T, E, topk, T)
        with torch.no_grad():
            moe_shared_forward(q, layers, gw, _x(T, H, dtype, T), idx, w)
        assert q.last_plan["shared"] == ("decode" if T <= SHARED_DECODE_MAX_TOKENS else "combine") and q.last_plan["path"] == "decode", (T, q.last_plan)
    T = 7
    x = _x(T, H, dtype, 3)
    idx, w = _routing(T, E, topk, 3)
    with torch.no_grad():
        out = moe_shared_forward(q, layers, gw, x, idx, w)
        assert q.last_plan["shared"] == "combine" and q.last_plan["path"] == "grouped"
        routed = moe_forward(q, x, idx, w)
        ys = layers[2](torch.nn.functional.silu(layers[0](x)) * layers[1](x))
    ref = routed.double() + torch.sigmoid((x.double() @ gw.double().t())) * ys.double()
    assert float((out.double() - ref).abs().max()) <= 2e-2 * max(1.0, float(ref.abs().max()))
    # under grad: the torch formula, differentiable in x
    xg = x.clone().requires_grad_(True)
    y = moe_shared_forward(q, layers, gw, xg, idx, w)
    assert q.last_plan["shared"] == "torch" and y.requires_grad
    assert float((y.detach().double() - ref).abs().max()) <= 2e-2 * max(1.0, float(ref.abs().max()))


def test_graph_capture_replays_with_new_inputs():
    dtype = torch.float16
    E, topk, H, I, Is = EDGE
    q, layers, gw = make_block(E, topk, H, I, Is, 8, 32, True, dtype, seed=4)
    T = 1
    x = torch.zeros((T, H), dtype=dtype, device=DEV)
    idx = torch.zeros((T, topk), dtype=torch.int64, device=DEV)
    w = torch.zeros((T, topk), dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        moe_shared_forward(q, layers, gw, x, idx, w)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = moe_shared_forward(q, layers, gw, x, idx, w)
    assert q.last_plan["shared"] == "decode"
    for r in range(3):
        xn = _x(T, H, dtype, r)
        idn, wn = _routing(T, E, topk, 100 + r)
        x.copy_(xn), idx.copy_(idn), w.copy_(wn)
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = moe_shared_forward(q, layers, gw, xn, idn, wn)
        assert torch.equal(out, eager), r


# ---------------------------------------------------------------------------------------------------------------- the tiny model
def _tiny(tmp_path):
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    import _tiny_qwen2_moe as TQ
    from autogptq_amd.model_utils import autogptq_post_init
    from autogptq_amd.moe import inject_fused_router, inject_shared_expert
    model, twin = TQ.build(tmp_path)
    model, twin = model.to(DEV), twin.to(DEV)
    assert inject_shared_expert(model) == 2 and inject_fused_router(model) == 2
    autogptq_post_init(model, max_input_length=64, expert_decode_copy=True)
    return TQ, model, twin


def test_tiny_qwen2_moe_end_to_end(tmp_path):
    """A prompt of 12 tokens runs the combine tail, the decode steps of generate the fused call; every hooked block agrees with the fp16 twin's class forward
    on the SAME hidden states at the tolerance of test_tiny_mixtral_end_to_end (per block: the models' hidden states drift apart layer by layer)."""
    TQ, model, twin = _tiny(tmp_path)
    blocks = [layer.mlp for layer in model.model.layers]
    seen = []
    hooks = [b.register_forward_hook(lambda m, args, out: seen.append((m, args[0], out, dict(m.experts.last_plan)))) for b in blocks]
    ids = torch.randint(0, 512, (1, 12), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        logits = model(ids).logits.float()
        assert torch.isfinite(logits).all()
        prompt = list(seen)
        ga = model.generate(ids, max_new_tokens=4, do_sample=False)
    for h in hooks:
        h.remove()
    assert ga.shape == (1, 16)
    assert len(prompt) == 2 and all(p[3]["shared"] == "combine" for p in prompt), [p[3] for p in prompt]
    steps = [s for s in seen if s[1].reshape(-1, s[1].shape[-1]).shape[0] == 1]
    assert len(steps) >= 2 * 3 and all(s[3]["shared"] == "decode" and s[3]["path"] == "decode" for s in steps), [s[3] for s in seen]
    for m, hs, out, _ in prompt + steps[:2]:
        li = blocks.index(m)
        with torch.no_grad():
            ref = twin.model.layers[li].mlp(hs)
        err = (out.float() - ref.float()).abs().max().item()
        assert out.shape == ref.shape and err <= 1e-2 * max(1.0, ref.abs().max().item()), (li, err)


def test_tiny_qwen2_moe_decode_step_capture(tmp_path):
    from transformers import StaticCache
    from autogptq_amd.model_utils import capture_decode_step
    TQ, model, _ = _tiny(tmp_path)
    ids = torch.randint(0, 512, (1, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        ref = model.generate(ids, max_new_tokens=8, do_sample=False)[0, 8:]
    cache = StaticCache(config=model.config, max_cache_len=64)
    with torch.no_grad():
        logits = model(ids, past_key_values=cache, use_cache=True).logits
    tok = logits[:, -1].argmax(-1)
    step = capture_decode_step(model, cache)
    assert all(layer.mlp.experts.last_plan["shared"] == "decode" for layer in model.model.layers)
    got = [tok.item()]
    for _ in range(7):
        tok = step(tok.view(1, 1))[:, -1].argmax(-1)
        got.append(tok.item())
    assert got == ref.tolist()
