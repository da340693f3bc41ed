"""GPU: 2- and 3-bit routed experts on the grouped path (QuantMoEExperts.post_init(low_bit=True) -> GPTQ_MOE_LOW_BIT): gptq_moe_forward at any T and
gptq_moe_backward.  The oracles and bounds are those of the 4- / 8-bit tests: test_gpu_moe.check (fp64 product of dequantize(), C = 16 -- a wrong field,
pair order or zero point misses it by orders of magnitude) and test_gpu_moe_backward.check_backward (tests/_moe_backward_oracle.py).

Shapes are the smallest that reach each hazard: H = 256 is 8 k-steps (every k-slot window; both straddling 3-bit zero quads in every 64-column block),
T = 130 gives full and short 64-row tiles, (192, 320) uneven steps per wave and odd counts of 64-column blocks, I = 2048 at T = 1 the
K-slice form of the down GEMM."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _guarded as G  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.moe import QuantMoEExperts, moe_forward  # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear  # noqa: E402
from test_gpu_moe import DEV, _fill, _routing, check, make_experts  # noqa: E402
from test_gpu_moe_backward import check_backward, run_backward  # noqa: E402

pytestmark = pytest.mark.gpu
E, TOPK, H, I = 8, 2, 256, 512
_CACHE = {}


def _rand(T, K, dtype, seed):
    return (torch.rand((T, K), generator=torch.Generator().manual_seed(seed)) - 0.5).to(dtype).to(DEV)


def _es(dtype):
    return torch.tensor([], dtype=dtype).element_size()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def low_bit_experts(*args, backward=False, **kw):
    q = make_experts(*args, **kw)
    assert q.plan(1)["path"] == "per_expert"                      # without the switch: as before
    q.post_init(backward=backward, low_bit=True)
    assert q.plan(1)["path"] == "grouped" and q._moe.flags == _lib.MOE_LOW_BIT
    return q


def shared(bits, dtype=torch.float16, act=False, backward=False):
    """One set of (8, 2, 256, 512) g128 experts per (bits, dtype, act, backward), shared by the tests that only read them."""
    key = (bits, dtype, act, backward)
    if key not in _CACHE:
        _CACHE[key] = low_bit_experts(E, H, I, bits, 128, act, dtype, seed=40 + bits, backward=backward)
    return _CACHE[key]


def custom_experts(E_, H_, I_, bits, gs, act, dtype, seed, down_bits=None, zero_mode="auto"):
    """As make_experts, with a zero_mode and (down_bits) a down projection of another width than gate | up."""
    gen = torch.Generator().manual_seed(seed)
    q = QuantMoEExperts(E_, H_, I_, bits, gs, top_k=TOPK, weight_dtype=dtype, zero_mode=zero_mode)
    for e in range(E_):
        if down_bits is not None:
            setattr(q[e], "w2", QuantLinear(down_bits, gs, I_, H_, False, weight_dtype=dtype, zero_mode=zero_mode))
        for l in q[e].layers():
            _fill(l, gen, act)
    q = q.to(DEV)
    q.post_init(low_bit=True)
    return q


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [32, 128, -1])
@pytest.mark.parametrize("bits", [2, 3])
def test_parity_grid(bits, gs, act, dtype):
    q = low_bit_experts(E, H, I, bits, gs, act, dtype, seed=bits + gs + E, top_k=TOPK)
    for T in (0, 1, 3, 7, 64, 130):
        idx, w = _routing(T, E, TOPK, T + E)
        check(q, _rand(T, H, dtype, T), idx, w, dtype)


@pytest.mark.parametrize("gs", [32, 64])
@pytest.mark.parametrize("bits", [2, 3])
def test_uneven_steps_per_wave_and_an_odd_last_column_block(bits, gs):
    """(E, topk, H, I) = (4, 2, 192, 320): 6 steps over the 4 waves of gate | up and 10 over those of down, and 5 / 3 column blocks -- an odd count, so the
    last block's zero points start mid-way through the qzeros row's 6-word period at 3 bits."""
    for dtype, act in ((torch.float16, True), (torch.bfloat16, False)):
        q = low_bit_experts(4, 192, 320, bits, gs, act, dtype, seed=bits + gs, top_k=TOPK)
        for T in (3, 70):
            idx, w = _routing(T, 4, TOPK, T)
            check(q, _rand(T, 192, dtype, T), idx, w, dtype)


@pytest.mark.parametrize("bits", [2, 3])
def test_k_slices_of_the_down_gemm(bits):
    q = low_bit_experts(2, 128, 2048, bits, 128, False, torch.float16, seed=bits, top_k=2)
    assert q.plan(1)["ksplit"] == 2, q.plan(1)
    idx, w = _routing(1, 2, 2, 1)
    check(q, _rand(1, 128, torch.float16, 1), idx, w, torch.float16)


@pytest.mark.parametrize("bits,down_bits", [(3, 4), (4, 2)], ids=["gu3-d4", "gu4-d2"])
def test_mixed_widths(bits, down_bits):
    for dtype, act in ((torch.float16, False), (torch.bfloat16, True)):
        q = custom_experts(E, H, I, bits, 64, act, dtype, seed=bits + down_bits, down_bits=down_bits)
        assert {l.bits for l in q[0].layers()} == {bits, down_bits}
        for T in (1, 70):
            idx, w = _routing(T, E, TOPK, T)
            check(q, _rand(T, H, dtype, T), idx, w, dtype)


@pytest.mark.parametrize("zero_mode", ["wrap", "nowrap"])
def test_both_zero_point_conventions_at_3_bits(zero_mode):
    """Random qzeros: fields equal to maxq occur (wrap: zero point 0; nowrap: 8)."""
    q = custom_experts(E, H, I, 3, 32, False, torch.float16, seed=17, zero_mode=zero_mode)
    gate = q[0].layers()[0]
    assert gate.zero_mode == zero_mode
    from oracle import gptq_oracle as O
    z = O.unpack_zeros(gate.qzeros.cpu(), 3, zero_mode)
    assert (z == (0 if zero_mode == "wrap" else 8)).any()
    for T in (3, 70):
        idx, w = _routing(T, E, TOPK, T)
        check(q, _rand(T, H, torch.float16, T), idx, w, torch.float16)


def test_reproducible_and_permutation_invariant():
    dtype = torch.bfloat16
    q = shared(3, dtype, act=True)
    T = 300
    x = _rand(T, H, dtype, 9)
    idx, w = _routing(T, E, TOPK, 9)
    with torch.no_grad():
        a = moe_forward(q, x, idx, w)
        b = moe_forward(q, x, idx, w)
        p = torch.randperm(T, generator=torch.Generator().manual_seed(4)).to(DEV)
        c = moe_forward(q, x[p], idx[p], w[p])
    assert torch.equal(a, b)
    assert torch.equal(a[p], c)


def test_graph_capture_replays_with_new_inputs():
    """Not possible on the per-expert composition (torch.where syncs the host once per expert)."""
    dtype = torch.float16
    q = shared(3, dtype, act=True)
    T = 4
    x = torch.zeros((T, H), dtype=dtype, device=DEV)
    idx = torch.zeros((T, TOPK), dtype=torch.int64, device=DEV)
    w = torch.zeros((T, TOPK), dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        moe_forward(q, x, idx, w)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = moe_forward(q, x, idx, w)
    assert q.last_plan["path"] == "grouped"
    for r in range(3):
        xn = _rand(T, H, dtype, r)
        idn, wn = _routing(T, E, TOPK, 100 + r)
        x.copy_(xn), idx.copy_(idn), w.copy_(wn)
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = moe_forward(q, xn, idn, wn)
        assert torch.equal(out, eager), r


@pytest.mark.parametrize("bits", [2, 3])
def test_the_switch_is_opt_in_and_survives_a_re_init(bits, caplog):
    dtype = torch.float16
    off = make_experts(E, H, I, bits, 128, False, dtype, seed=40 + bits)      # the weights of shared(bits)
    on = shared(bits, dtype)
    for T in (1, 7, 70):
        assert off.plan(T)["path"] == "per_expert" and f"{bits}-bit" in off.plan(T)["reason"]
        assert on.plan(T)["path"] == "grouped"
        idx, w = _routing(T, E, TOPK, T)
        x = _rand(T, H, dtype, T)
        with torch.no_grad():
            a, b = moe_forward(off, x, idx, w), moe_forward(on, x, idx, w)
        assert off.last_plan["path"] == "per_expert" and on.last_plan["path"] == "grouped"
        assert torch.allclose(a.float(), b.float(), rtol=1e-2, atol=1e-3), float((a.float() - b.float()).abs().max())
    # the tables are rebuilt with the remembered choice
    q = low_bit_experts(E, H, I, bits, 128, False, dtype, seed=1, backward=True)
    q._invalidate()
    assert q.plan(1)["path"] == "grouped" and q._grad_table is not None and q._moe.flags == _lib.MOE_LOW_BIT
    # the decode copy and the batch path keep declining these widths; the grouped path stays
    q.post_init(decode_copy=True, batch=True, low_bit=True)
    assert q._decode_table is None and q.decode_copy_bytes == 0
    assert "has no effect" in caplog.text and f"{bits}-bit" in caplog.text
    assert [q.plan(T)["path"] for T in (1, 4, 5, 64, 65)] == ["grouped"] * 5
    q.post_init()
    assert q.plan(1)["path"] == "per_expert" and q._moe.flags == 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("bits", [2, 3])
def test_backward_parity(bits, act, dtype):
    q = shared(bits, dtype, act, backward=True)
    assert q._grad_table is not None
    for T in (3, 70):
        idx, w = _routing(T, E, TOPK, T + E)
        check_backward(q, _rand(T, H, dtype, T), idx, w, _rand(T, H, dtype, 100 + T))


def test_autograd_node_matches_the_per_expert_composition():
    dtype, T = torch.float16, 16
    q = shared(3, dtype, backward=True)
    ref = make_experts(E, H, I, 3, 128, False, dtype, seed=43)                # the same weights without the switches: the composition under grad
    idx, w0 = _routing(T, E, TOPK, 0)
    gy = torch.randn((T, H), generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
    x0 = _rand(T, H, dtype, 0)
    with torch.no_grad():
        plain = moe_forward(q, x0, idx, w0)
    for need_x, need_w in ((True, True), (True, False), (False, True)):
        x = x0.clone().requires_grad_(need_x)
        w = w0.clone().requires_grad_(need_w)
        out = moe_forward(q, x, idx, w)
        assert q.last_plan["path"] == "grouped" and q.last_plan["backward"] == "grouped", q.last_plan
        assert torch.equal(out, plain)
        assert out.grad_fn is not None and "MoEBackward" in type(out.grad_fn).__name__
        out.backward(gy)
        xr, wr = x0.clone().requires_grad_(need_x), w0.clone().requires_grad_(need_w)
        outr = moe_forward(ref, xr, idx, wr)
        assert ref.last_plan["path"] == "per_expert" and "backward" not in ref.last_plan
        outr.backward(gy)
        if need_x:
            assert torch.allclose(x.grad.float(), xr.grad.float(), rtol=3e-2, atol=3e-3), float((x.grad.float() - xr.grad.float()).abs().max())
        else:
            assert x.grad is None
        if need_w:
            assert torch.allclose(w.grad, wr.grad, rtol=3e-2, atol=3e-3), float((w.grad - wr.grad).abs().max())
        else:
            assert w.grad is None


def _edge_routing(T):
    idx, w = _routing(T, E, TOPK, T + E)
    idx[::3, 0] = E
    idx[1::4, 1] = -1
    idx[7] = torch.tensor([E, -1], device=DEV)
    return idx, w


@pytest.mark.parametrize("bits", [2, 3])
def test_forward_stays_inside_guarded_buffers(bits):
    """x, topk_idx, topk_w, out, h_out and a workspace of exactly gptq_moe_workspace_bytes inside guard bands; bit-identical to moe_forward."""
    dtype, T = torch.float16, 70
    q = shared(bits, dtype, act=True)
    lib = _lib.load()
    es, R = _es(dtype), T * TOPK
    m = ctypes.byref(q._moe)
    need = int(lib.gptq_moe_workspace_bytes(m, T, TOPK))
    assert need > 0
    x = _rand(T, H, dtype, T)
    for name, (idx, w) in (("random", _routing(T, E, TOPK, T)), ("E-and-minus-1", _edge_routing(T))):
        with torch.no_grad():
            y_mod, hs_mod, pos_mod = moe_forward(q, x, idx, w, return_intermediate=True)
        gx, _ = G.guarded_like(x, G.guard_for(H * es))
        gi, _ = G.guarded_like(idx, G.guard_for(TOPK * 8))
        gw, _ = G.guarded_like(w, G.guard_for(TOPK * 4))
        ws = G.Guarded(need, max(64 << 10, (need + 255) // 256 * 256), 0x00, G.OUT_GUARD, DEV)
        valid = pos_mod >= 0
        for launch in (1, 2):
            go = G.Guarded(T * H * es, G.guard_for(H * es), 0xFF, G.OUT_GUARD, DEV)
            gh = G.Guarded(R * I * es + 4 * R, G.guard_for(I * es), 0xFF, G.OUT_GUARD, DEV)
            _lib.check(lib.gptq_moe_forward(m, q._table.data_ptr(), gx.ptr, gi.ptr, gw.ptr, T, TOPK, go.ptr, gh.ptr, ws.ptr, need, _stream()))
            for g, nm in ((gx, "x"), (gi, "topk_idx"), (gw, "topk_w"), (go, "out"), (gh, "h_out"), (ws, f"workspace ({need} bytes = its query)")):
                g.assert_intact(f"gptq_moe_forward int{bits} routing={name}: {nm} (launch {launch})")
            assert torch.equal(go.view(dtype, (T, H)), y_mod), (name, launch)
            pos = gh.body[R * I * es:].view(torch.int32).view(T, TOPK)
            hs = gh.body[:R * I * es].view(dtype).view(R, I)
            assert torch.equal(pos, pos_mod)
            assert torch.equal(hs[pos[valid].long()], hs_mod[pos_mod[valid].long()])


@pytest.mark.parametrize("bits", [2, 3])
def test_backward_stays_inside_guarded_buffers(bits):
    dtype, T = torch.float16, 70
    q = shared(bits, dtype, act=True, backward=True)
    lib = _lib.load()
    es, R = _es(dtype), T * TOPK
    idx, w = _edge_routing(T)
    x, dout = _rand(T, H, dtype, 1), _rand(T, H, dtype, 2)
    ref = run_backward(q, x, idx, w, dout)
    need = int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(q._moe), T, TOPK))
    assert need > 0
    gx, _ = G.guarded_like(x, G.guard_for(H * es))
    gd, _ = G.guarded_like(dout, G.guard_for(H * es))
    gi, _ = G.guarded_like(idx, G.guard_for(TOPK * 8))
    gw, _ = G.guarded_like(w, G.guard_for(TOPK * 4))
    ws = G.Guarded(need, max(64 << 10, (need + 255) // 256 * 256), 0x00, G.OUT_GUARD, DEV)
    for launch in (1, 2):
        gdx = G.Guarded(T * H * es, G.guard_for(H * es), 0xFF, G.OUT_GUARD, DEV)
        gdw = G.Guarded(T * TOPK * 4, G.guard_for(TOPK * 4), 0xFF, G.OUT_GUARD, DEV)
        gdgu = G.Guarded(2 * R * I * es + 4 * R, G.guard_for(I * es), 0xFF, G.OUT_GUARD, DEV)
        _lib.check(lib.gptq_moe_backward(ctypes.byref(q._moe), q._table.data_ptr(), q._grad_table.data_ptr(), gx.ptr, gi.ptr, gw.ptr, gd.ptr, T, TOPK,
                                         gdx.ptr, gdw.ptr, gdgu.ptr, ws.ptr, need, _stream()))
        for g, nm in ((gx, "x"), (gd, "dout"), (gi, "topk_idx"), (gw, "topk_w"), (gdx, "dx"), (gdw, "dw"), (gdgu, "dgu_out"),
                      (ws, f"workspace ({need} bytes = its query)")):
            g.assert_intact(f"gptq_moe_backward int{bits}: {nm} (launch {launch})")
        assert torch.equal(gdx.view(dtype, (T, H)), ref[0]) and torch.equal(gdw.view(torch.float32, (T, TOPK)), ref[1])
        assert torch.equal(gdgu.body[2 * R * I * es:].view(torch.int32).view(T, TOPK), ref[4])


def _tiny3(tmp_path, monkeypatch, desc_act):
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    import _tiny_mixtral as TM
    from autogptq_amd.model_utils import autogptq_post_init
    monkeypatch.setattr(TM, "BITS", 3)
    src = TM.fresh_model(0)
    twin_w = TM.quantize_and_pack(src, desc_act)
    TM.save_checkpoint(src, str(tmp_path), desc_act)
    model, _, qc = TM.load_checkpoint(str(tmp_path))
    assert qc["bits"] == 3
    twin = TM.make_twin(model.state_dict(), twin_w).to(DEV)
    model = model.to(DEV)
    autogptq_post_init(model, max_input_length=64, expert_low_bit=True)
    return TM, model, twin


@pytest.mark.parametrize("desc_act", [False, True])
def test_tiny_mixtral_at_3_bits_end_to_end(tmp_path, monkeypatch, desc_act):
    """quantise -> pack -> save -> load -> autogptq_post_init(expert_low_bit=True): the logits against the dequantised fp16 twin, and every MoE layer against
    the twin's MixtralExperts on the same inputs, both at test_gpu_moe.test_tiny_mixtral_end_to_end's tolerance (1e-2 of max(1, |ref|))."""
    TM, model, twin = _tiny3(tmp_path, monkeypatch, desc_act)
    seen = []
    hooks = [layer.mlp.experts.register_forward_hook(lambda m, args, out: seen.append((m, args, out))) for layer in model.model.layers]
    ids = torch.randint(0, 512, (1, 12), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        logits = model(ids).logits.float()
        ref_logits = twin(ids).logits.float()
    for h in hooks:
        h.remove()
    assert torch.isfinite(logits).all() and len(seen) == 2
    for layer in model.model.layers:
        ex = layer.mlp.experts
        assert isinstance(ex, QuantMoEExperts) and ex.bits == 3 and ex.last_plan["path"] == "grouped", ex.last_plan
    for li, (m, (hs, idx, w), out) in enumerate(seen):
        with torch.no_grad():
            ref = twin.model.layers[li].mlp.experts(hs, idx, w)
        err = (out.float() - ref.float()).abs().max().item()
        print(f"layer {li}: max|out - twin| {err:.5f}  max|twin| {ref.abs().max().item():.4f}")
        assert err <= 1e-2 * max(1.0, ref.abs().max().item()), (li, err)
    err = (logits - ref_logits).abs().max().item()
    print(f"logits: max|model - twin| {err:.5f}  max|twin| {ref_logits.abs().max().item():.4f}")
    assert err <= 1e-2 * max(1.0, ref_logits.abs().max().item()), err
    with torch.no_grad():
        ga = model.generate(ids, max_new_tokens=8, do_sample=False)
    assert ga.shape == (1, 20)


def test_tiny_mixtral_at_3_bits_decode_step_capture(tmp_path, monkeypatch):
    from transformers import StaticCache
    from autogptq_amd.model_utils import capture_decode_step
    TM, model, _ = _tiny3(tmp_path, monkeypatch, False)
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
