"""GPU: the grouped backward of the mixture-of-experts layers (gptq_moe_backward; QuantMoEExperts.post_init(backward=True)) against the fp64 oracle of the
formulas in include/gptq_mi355x.h (tests/_moe_backward_oracle.py on the dequantised weights), with the project's per-output error model
(test_gpu_moe.py / test_gpu_error_model.py, C = 16):

    |y - y64|  <=  (1/2 + 1/64) ulp_T(y64)  +  C sqrt(K) 2^-24 (|a| @ |W|)      per GEMM

propagated to first order through the formulas (second-order terms: the factor 1.1 that test_gpu_moe.check uses; |silu'| <= 1.1, |silu''| <= 0.5):

    E_d = C sqrt(H) 2^-24 |dOut| |W2^T|                         d is kept in fp32: no rounding term
    D_g = C sqrt(H) 2^-24 |x| |W1| + (1/2 + 1/64) ulp_T(g)      the recomputed g (u alike): the GEMM term plus its one rounding to T
    dg:  (1/2 + 1/64) ulp_T(dg) + 1.1 |w| (1.1 E_d |u| + 1.1 |d| D_u + 0.5 |d| |u| D_g) + 1e-6 |dg|        (1e-6: the fp32 epilogue, as check's H bound)
    du:  (1/2 + 1/64) ulp_T(du) + 1.1 |w| (E_d |silu(g)| + 1.1 |d| D_g) + 1e-6 |du|
    dX:  against the fp64 product of the kernel's OWN dg / du rows with W1^T, W3^T summed over j:  (1/2 + 1/64) ulp_T + C sqrt(2 I) 2^-24 A
    dw:  sum_i 1.1 (E_d |h| + |d| B_h) + C sqrt(I) 2^-24 sum_i |d| |h|,   B_h = check's H bound with D_g, D_u in the place of E_g, E_u
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _guarded as G  # noqa: E402
from _moe_backward_oracle import oracle  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.moe import QuantMoEExperts, moe_forward  # noqa: E402
from test_gpu_moe import C, DEV, _routing, _ulp, make_experts  # noqa: E402

pytestmark = pytest.mark.gpu
EPS, HALF = 2.0 ** -24, 0.5 + 1 / 64


def _es(dtype):
    return torch.tensor([], dtype=dtype).element_size()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _rand(T, H, dtype, seed):
    return (torch.rand((T, H), generator=torch.Generator().manual_seed(seed)) - 0.5).to(dtype).to(DEV)


def make_backward_experts(*args, **kw):
    q = make_experts(*args, **kw)
    q.post_init(backward=True)
    assert q._grad_table is not None
    return q


def _dense(q):
    """([W1_e], [W3_e], [W2_e]) in fp64: the weights the kernels must use, bit for bit (computed once per module)."""
    d = getattr(q, "_dense64", None)
    if d is None:
        d = q._dense64 = tuple([l.dequantize().double() for l in ls] for ls in q.projections())
    return d


def run_backward(q, x, idx, w, dout, want_dx=True, want_dw=True, want_dgu=True, ws=None):
    """One gptq_moe_backward call through the C ABI: (dx [T, H] | None, dw [T, topk] | None, dg rows, du rows, pos) of the kernel."""
    lib = _lib.load()
    T, topk = idx.shape
    H, I, dtype = q.hidden_dim, q.intermediate_dim, x.dtype
    R, es = T * topk, _es(x.dtype)
    need = int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(q._moe), T, topk))
    assert need > 0
    if ws is None:
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    dx = torch.full((T, H), float("nan"), dtype=dtype, device=DEV) if want_dx else None
    dw = torch.full((T, topk), float("nan"), dtype=torch.float32, device=DEV) if want_dw else None
    dgu = torch.zeros(2 * R * I * es + 4 * R, dtype=torch.uint8, device=DEV) if want_dgu else None
    _lib.check(lib.gptq_moe_backward(ctypes.byref(q._moe), q._table.data_ptr(), q._grad_table.data_ptr(), x.data_ptr(), idx.data_ptr(), w.data_ptr(),
                                     dout.data_ptr(), T, topk, _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(dgu), ws.data_ptr(), ws.numel(), _stream()))
    if not want_dgu:
        return dx, dw, None, None, None
    gb = R * I * es
    return (dx, dw, dgu[:gb].view(dtype).view(R, I), dgu[gb:2 * gb].view(dtype).view(R, I), dgu[2 * gb:].view(torch.int32).view(T, topk))


def _assert_within(err, bound, what):
    assert bool((err <= bound).all()), f"{what}: worst err/bound {float((err / bound).max()):.3f}"


def check_backward(q, x, idx, w, dout):
    """The kernel's dg / du / dX / dw against the fp64 oracle with the propagated bounds of the module docstring; returns (dx, dw)."""
    dtype = x.dtype
    T, topk = idx.shape
    H, I, E = q.hidden_dim, q.intermediate_dim, q.num_experts
    dx, dw, dgr, dur, pos = run_backward(q, x, idx, w, dout)
    assert dx.shape == (T, H) and dx.dtype == dtype and dw.shape == (T, topk) and dw.dtype == torch.float32
    if T == 0:
        return dx, dw
    W1, W3, W2 = _dense(q)
    o = oracle(x, idx, w, dout, W1, W3, W2)
    valid = o.valid
    assert torch.equal(pos >= 0, valid)
    rows = pos.clamp_min(0).long()
    dgk = torch.where(valid[:, :, None], dgr[rows].double(), 0.0)          # the kernel's rows per assignment [T, topk, I]
    duk = torch.where(valid[:, :, None], dur[rows].double(), 0.0)
    Ed = C * H ** 0.5 * EPS * o.Ad
    Dg = C * H ** 0.5 * EPS * o.Ag + HALF * _ulp(o.g, dtype)
    Du = C * H ** 0.5 * EPS * o.Au + HALF * _ulp(o.u, dtype)
    wa = w.double().abs()[:, :, None]
    silu = o.g * torch.sigmoid(o.g)
    d, u = o.d.abs(), o.u.abs()
    bound_dg = HALF * _ulp(o.dg, dtype) + 1.1 * wa * (1.1 * Ed * u + 1.1 * d * Du + 0.5 * d * u * Dg) + 1e-6 * o.dg.abs() + 1e-30
    bound_du = HALF * _ulp(o.du, dtype) + 1.1 * wa * (Ed * silu.abs() + 1.1 * d * Dg) + 1e-6 * o.du.abs() + 1e-30
    v3 = valid[:, :, None].expand_as(o.dg)
    _assert_within((dgk - o.dg).abs()[v3], bound_dg[v3], "dg")
    _assert_within((duk - o.du).abs()[v3], bound_du[v3], "du")
    # dX against the fp64 product of the kernel's own dg / du rows
    y64 = torch.zeros((T, H), dtype=torch.float64, device=DEV)
    A = torch.zeros_like(y64)
    for e in range(E):
        tok, j = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        y64.index_add_(0, tok, dgk[tok, j] @ W1[e].t() + duk[tok, j] @ W3[e].t())
        A.index_add_(0, tok, dgk[tok, j].abs() @ W1[e].abs().t() + duk[tok, j].abs() @ W3[e].abs().t())
    _assert_within((dx.double() - y64).abs(), HALF * _ulp(y64, dtype) + C * (2 * I) ** 0.5 * EPS * A + 1e-30, "dX")
    # dw against <d64, h64>
    bound_h = HALF * _ulp(o.h, dtype) + 1.1 * Dg * (u + Du) + silu.abs() * Du + 1e-6 * o.h.abs() + 1e-30
    bound_dw = (1.1 * (Ed * o.h.abs() + d * bound_h)).sum(-1) + C * I ** 0.5 * EPS * (d * o.h.abs()).sum(-1) + 1e-30
    _assert_within((dw.double() - o.dw).abs()[valid], bound_dw[valid], "dw")
    # dropped assignments: dw exactly 0; a token without a valid expert: a zero dX row
    assert not bool(dw[~valid].any())
    none = ~valid.any(-1)
    assert not bool(dx[none].any())
    return dx, dw


TS = (0, 1, 3, 17, 70)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [32, 128, -1])
@pytest.mark.parametrize("bits", [4, 8])
def test_parity_grid(bits, gs, act, dtype):
    E, topk, H, I = 8, 2, 256, 512
    q = make_backward_experts(E, H, I, bits, gs, act, dtype, seed=bits + gs + E, top_k=topk)
    for T in TS:
        x, dout = _rand(T, H, dtype, T), _rand(T, H, dtype, 100 + T)
        idx, w = _routing(T, E, topk, T + E)
        check_backward(q, x, idx, w, dout)


def test_partial_128_column_tiles_of_both_stages():
    """H = 320, I = 448: multiples of 64 but not of 128 -- the last output tile of the down stage (I) and of the up stage (H) is half a tile."""
    for dtype, act in ((torch.float16, False), (torch.bfloat16, True)):
        q = make_backward_experts(8, 320, 448, 4, 64, act, dtype, seed=21)
        for T in (3, 70):
            idx, w = _routing(T, 8, 2, T)
            check_backward(q, _rand(T, 320, dtype, T), idx, w, _rand(T, 320, dtype, 50 + T))


def test_skewed_routing_one_full_tile_and_a_short_one():
    dtype = torch.float16
    q = make_backward_experts(8, 256, 512, 4, 128, False, dtype, seed=3, top_k=1)
    T = 70
    idx = torch.zeros((T, 1), dtype=torch.int64, device=DEV)              # every token to expert 0: a 64-row tile and a 6-row tile
    w = (torch.rand((T, 1), generator=torch.Generator().manual_seed(1)) + 0.5).to(DEV)
    check_backward(q, _rand(T, 256, dtype, 1), idx, w, _rand(T, 256, dtype, 2))


def test_topk_8_of_8_experts():
    dtype = torch.bfloat16
    q = make_backward_experts(8, 256, 512, 8, 128, True, dtype, seed=4, top_k=8)
    for T in (1, 9):
        idx, w = _routing(T, 8, 8, T)
        check_backward(q, _rand(T, 256, dtype, T), idx, w, _rand(T, 256, dtype, 30 + T))


def test_dropped_assignments_give_exact_zeros():
    dtype = torch.float16
    q = make_backward_experts(8, 256, 512, 4, 128, False, dtype, seed=3)
    T = 50
    idx = torch.randint(0, 8, (T, 2), generator=torch.Generator().manual_seed(2)).to(DEV)
    idx[::3, 0] = 8
    idx[1::4, 1] = -1
    idx[7] = torch.tensor([8, -1])
    w = torch.full((T, 2), 0.5, device=DEV)
    dx, dw = check_backward(q, _rand(T, 256, dtype, 1), idx, w, _rand(T, 256, dtype, 2))
    assert not bool(dw[7].any()) and not bool(dx[7].any())
    assert not bool(dw[0, 0]) and not bool(dw[1, 1]) and bool(dx[0].any())


def test_qwen_moe_like_block():
    """E = 60, topk = 4, H = 2048, I = 1408 (a multiple of 128), T = 64, int4 g128 fp16."""
    dtype = torch.float16
    q = make_backward_experts(60, 2048, 1408, 4, 128, False, dtype, seed=5, top_k=4)
    idx, w = _routing(64, 60, 4, 9)
    check_backward(q, _rand(64, 2048, dtype, 9), idx, w, _rand(64, 2048, dtype, 10))


def _per_expert_grads(q_ref, x, idx, w, gy):
    xr, wr = x.detach().clone().requires_grad_(x.requires_grad), w.detach().clone().requires_grad_(w.requires_grad)
    out = moe_forward(q_ref, xr, idx, wr)
    assert q_ref.last_plan["path"] == "per_expert"
    out.backward(gy.to(out.dtype))
    return xr.grad, wr.grad


def test_autograd_node_matches_the_per_expert_composition():
    dtype = torch.float16
    E, H, I, T = 8, 256, 512, 16
    q = make_backward_experts(E, H, I, 4, 128, False, dtype, seed=6)
    ref = make_experts(E, H, I, 4, 128, False, dtype, seed=6)             # the same weights without the flag: the composition under grad
    idx, w0 = _routing(T, E, 2, 0)
    gy = torch.randn((T, H), generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
    x0 = _rand(T, H, dtype, 0)
    with torch.no_grad():
        plain = moe_forward(q, x0, idx, w0)
    for need_x, need_w, xdt in ((True, True, dtype), (True, False, dtype), (False, True, dtype), (True, True, torch.float32)):
        x = x0.to(xdt).clone().requires_grad_(need_x)
        w = w0.clone().requires_grad_(need_w)
        out = moe_forward(q, x, idx, w)
        assert q.last_plan["path"] == "grouped" and q.last_plan["backward"] == "grouped", q.last_plan
        assert out.dtype == xdt and torch.equal(out.to(dtype), plain)      # the ordinary no-grad path's values, bit for bit
        assert out.grad_fn is not None and "MoEBackward" in type(out.grad_fn).__name__
        out.backward(gy.to(xdt))
        gx_ref, gw_ref = _per_expert_grads(ref, x, idx, w, gy)
        if need_x:
            assert x.grad.dtype == xdt and x.grad.shape == x.shape
            assert torch.allclose(x.grad.float(), gx_ref.float(), rtol=3e-2, atol=3e-3), float((x.grad.float() - gx_ref.float()).abs().max())
        else:
            assert x.grad is None
        if need_w:
            assert w.grad.dtype == w.dtype and w.grad.shape == w.shape
            assert torch.allclose(w.grad, gw_ref, rtol=3e-2, atol=3e-3), float((w.grad - gw_ref).abs().max())
        else:
            assert w.grad is None
    # without the flag nothing changes: the composition, as test_gpu_moe.test_gradients_through_the_experts sees it
    out = moe_forward(ref, x0.clone().requires_grad_(True), idx, w0)
    assert ref.last_plan["path"] == "per_expert" and "backward" not in ref.last_plan
    # leading dimensions and the module's forward
    x3 = x0.reshape(2, 8, H).clone().requires_grad_(True)
    out3 = q(x3, idx, w0)
    out3.backward(gy.reshape(2, 8, H))
    assert out3.shape == (2, 8, H) and x3.grad.shape == (2, 8, H)


def test_reproducible_graph_capturable_and_allocation_free():
    dtype = torch.bfloat16
    E, H, I, T, topk = 8, 256, 512, 70, 2
    q = make_backward_experts(E, H, I, 4, 32, True, dtype, seed=7)
    lib = _lib.load()
    x, dout = _rand(T, H, dtype, 1), _rand(T, H, dtype, 2)
    idx, w = _routing(T, E, topk, 3)
    need = int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(q._moe), T, topk))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)                  # reserved before the capture
    dx = torch.empty((T, H), dtype=dtype, device=DEV)
    dw = torch.empty((T, topk), dtype=torch.float32, device=DEV)

    def call():
        _lib.check(lib.gptq_moe_backward(ctypes.byref(q._moe), q._table.data_ptr(), q._grad_table.data_ptr(), x.data_ptr(), idx.data_ptr(), w.data_ptr(),
                                         dout.data_ptr(), T, topk, dx.data_ptr(), dw.data_ptr(), None, ws.data_ptr(), need, _stream()))

    call()
    torch.cuda.synchronize()
    a = (dx.clone(), dw.clone())
    before = torch.cuda.memory_allocated()
    call()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before                         # nothing is allocated by the call
    assert torch.equal(dx, a[0]) and torch.equal(dw, a[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    dx.zero_(), dw.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(dx, a[0]) and torch.equal(dw, a[1])
    # only one output asked for: the other is not touched, the one asked for has the same bits
    dx1, _, _, _, _ = run_backward(q, x, idx, w, dout, want_dw=False, want_dgu=False)
    _, dw1, _, _, _ = run_backward(q, x, idx, w, dout, want_dx=False, want_dgu=False)
    assert torch.equal(dx1, a[0]) and torch.equal(dw1, a[1])


@pytest.mark.parametrize("shape", [(256, 512, 1, "skew"), (320, 448, 2, "random")], ids=["t70-skewed", "h320-i448"])
def test_every_buffer_stays_inside_its_guards(shape):
    """dx, dw, dgu_out and the workspace sized exactly by the header's formulas inside guard bands; the inputs followed by poisoned guards."""
    H, I, topk, routing = shape
    dtype, E, T = torch.float16, 8, 70
    q = make_backward_experts(E, H, I, 4, 64, False, dtype, seed=9, top_k=topk)
    lib = _lib.load()
    es, R = _es(dtype), T * topk
    if routing == "skew":
        idx = torch.zeros((T, topk), dtype=torch.int64, device=DEV)
        w = torch.full((T, topk), 0.75, device=DEV)
    else:
        idx, w = _routing(T, E, topk, 5)
        idx[3, 0], idx[9, 1] = E, -1
    x, dout = _rand(T, H, dtype, 1), _rand(T, H, dtype, 2)
    ref = run_backward(q, x, idx, w, dout)
    need = int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(q._moe), T, topk))
    a256 = lambda b: (b + 255) // 256 * 256
    tiles = R // 64 + min(E, R)
    assert need == (_lib.WS_HEADER_BYTES + a256(4 * (E + 1)) + 256 + a256(16 * tiles) + 2 * a256(4 * R) + 2 * a256(R * I * es)
                    + a256(4 * R * ((I + 127) // 128)) + a256(4 * R * H))
    gx, _ = G.guarded_like(x, G.guard_for(H * es))
    gd, _ = G.guarded_like(dout, G.guard_for(H * es))
    gi, _ = G.guarded_like(idx, G.guard_for(topk * 8))
    gw, _ = G.guarded_like(w, G.guard_for(topk * 4))
    ws = G.Guarded(need, max(64 << 10, a256(need)), 0x00, G.OUT_GUARD, DEV)
    for launch in (1, 2):
        gdx = G.Guarded(T * H * es, G.guard_for(H * es), 0xFF, G.OUT_GUARD, DEV)
        gdw = G.Guarded(T * topk * 4, G.guard_for(topk * 4), 0xFF, G.OUT_GUARD, DEV)
        gdgu = G.Guarded(2 * R * I * es + 4 * R, G.guard_for(I * es), 0xFF, G.OUT_GUARD, DEV)
        _lib.check(lib.gptq_moe_backward(ctypes.byref(q._moe), q._table.data_ptr(), q._grad_table.data_ptr(), gx.ptr, gi.ptr, gw.ptr, gd.ptr, T, topk,
                                         gdx.ptr, gdw.ptr, gdgu.ptr, ws.ptr, need, _stream()))
        for g, nm in ((gx, "x"), (gd, "dout"), (gi, "topk_idx"), (gw, "topk_w"), (gdx, "dx"), (gdw, "dw"), (gdgu, "dgu_out"),
                      (ws, f"workspace ({need} bytes = its query)")):
            g.assert_intact(f"gptq_moe_backward H={H} I={I} routing={routing}: {nm} (launch {launch})")
        assert torch.equal(gdx.view(dtype, (T, H)), ref[0]) and torch.equal(gdw.view(torch.float32, (T, topk)), ref[1])
        assert torch.equal(gdgu.body[2 * R * I * es:].view(torch.int32).view(T, topk), ref[4])


def test_tiny_mixtral_lora_fine_tuning_step(tmp_path):
    """Adapters on the attention projections, frozen experts: one forward + loss.backward() in train mode with the grouped backward against the same model
    on the per-expert composition.

    The tolerance is test_gpu_moe.test_gradients_through_the_experts' (rtol 3e-2, atol 3e-3), which that test applies to gradients of magnitude 0.1 .. 1.
    Both models here are fp16 pipelines that round at every autograd node (2^-11 relative), the composition at 3 E more nodes than the grouped backward,
    so two correct runs differ by about 1e-3 of the LARGEST entry of a gradient matrix in every entry of it (an fp16 composition of ONE experts layer is
    already 6e-4 of the largest entry away from its fp64 value) -- an absolute difference that atol only covers while the gradients stay of order 1.
    The adapter values (0.01 randn) are therefore chosen so that the compared gradients are of that order: with 0.05 randn the lora_B gradients reach 3.6
    and the two runs differ by 5e-3 in entries near zero."""
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    import _tiny_mixtral as TM
    from autogptq_amd import lora as A
    from autogptq_amd.model_utils import autogptq_post_init
    src = TM.fresh_model(0)
    TM.quantize_and_pack(src, False)
    TM.save_checkpoint(src, str(tmp_path), False)
    ids = torch.randint(0, 512, (1, 12), generator=torch.Generator().manual_seed(0)).to(DEV)
    grads, plans = [], []
    for flag in (True, False):
        model, _, _ = TM.load_checkpoint(str(tmp_path))
        model = model.to(DEV)
        layers = A.inject_lora(model, ["q_proj", "k_proj", "v_proj", "o_proj"], r=8, lora_alpha=16)
        assert len(layers) == 8
        autogptq_post_init(model, max_input_length=64, expert_backward=flag)
        A.mark_only_lora_trainable(model)
        gen = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for n in sorted(layers):
                layers[n].lora_A.weight.copy_(torch.randn(layers[n].lora_A.weight.shape, generator=gen) * 0.01)
                layers[n].lora_B.weight.copy_(torch.randn(layers[n].lora_B.weight.shape, generator=gen) * 0.01)
        model.train()
        logits = model(ids).logits.float()
        loss = torch.nn.functional.cross_entropy(logits[0, :-1], ids[0, 1:])
        loss.backward()
        experts = [m for m in model.modules() if isinstance(m, QuantMoEExperts)]
        plans.append([m.last_plan for m in experts])
        grads.append({n: (layers[n].lora_A.weight.grad.clone(), layers[n].lora_B.weight.grad.clone()) for n in sorted(layers) if ".layers.0." in n})
    assert len(plans[0]) == 2 and all(p["backward"] == "grouped" for p in plans[0]), plans[0]
    assert all(p["path"] == "per_expert" for p in plans[1]), plans[1]
    assert len(grads[0]) == 4
    for n, (ga, gb) in grads[0].items():
        ra, rb = grads[1][n]
        assert bool(ga.any()) and bool(gb.any()), n
        for nm, g, r in (("lora_A", ga.float(), ra.float()), ("lora_B", gb.float(), rb.float())):
            print(f"{n}.{nm}: max|grad| {float(r.abs().max()):.4f}  max|diff| {float((g - r).abs().max()):.5f}  "
                  f"worst diff/(atol + rtol |ref|) {float(((g - r).abs() / (3e-3 + 3e-2 * r.abs())).max()):.3f}")
        assert torch.allclose(ga.float(), ra.float(), rtol=3e-2, atol=3e-3), (n, float((ga - ra).abs().max()))
        assert torch.allclose(gb.float(), rb.float(), rtol=3e-2, atol=3e-3), (n, float((gb - rb).abs().max()))
