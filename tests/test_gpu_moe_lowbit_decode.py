"""GPU: 2- and 3-bit routed experts on the decode path (QuantMoEExperts.post_init(low_bit_decode=True) -> GPTQ_MOE_LOW_BIT_DECODE): gptq_moe_decode_forward
at 1..4 tokens on the experts' decode copy, two launches of the 2- / 3-bit forms of moe_shared_kernel.

Oracle and bound are those of test_gpu_moe_decode.check -- the decode family's error model with the project's constant C = 4:

    |y - y64|  <=  (1/2 + 1/64) ulp(y64)  +  C sqrt(K) 2^-24 A,      A = |a| @ |W64|,   W64 = scales[g] (w - z[g]) in fp64, UNROUNDED

H is checked through the propagated silu * mul bound, out against the fp64 product of the kernel's OWN H rows; every output is checked.  That file's _w64
cuts whole fields per checkpoint word, which is wrong at 3 bits: here W64 is built from the integer tensors of gptq_unpack_weights / gptq_unpack_zeros
(pinned bit-exact to the reference fixtures by test_gpu_parity.py), and ``check`` below is that file's check with this W64.

Shapes (each confirmed on the CPU against the 4-bit decode plan: tests/test_moe_lowbit_decode_host.py):
  (E 8, topk 2, H 256, I 512)     2 / 4 chunks of 128 k: one pass, waves that see clamped chunks only
  (E 4, topk 2, H 320, I 448)     a ragged last chunk: dead k-slots on 2- and 3-word lanes
  (E 60, topk 4, H 2048, I 1408)  16 / 11 chunks: 3 waves per strip of the down launch, several passes of the pair launch"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _guarded as G  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.moe import QuantMoEExperts, moe_forward, moe_shared_forward  # noqa: E402
from test_gpu_moe import _fill, _routing, _ulp  # noqa: E402
from test_gpu_moe_decode import C, _x, make_experts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEC = _lib.MOE_LOW_BIT_DECODE


def low_bit_decode_experts(E, H, I, bits, gs, act, dtype, seed=0, top_k=2, low_bit=False):
    q = make_experts(E, H, I, bits, gs, act, dtype, seed=seed, top_k=top_k, decode_copy=False)
    assert q.plan(1)["path"] == "per_expert" and q._decode_table is None          # without the switch: as before
    q.post_init(low_bit=low_bit, low_bit_decode=True)
    assert q._decode_table is not None and q.decode_copy_bytes > 0 and q._moe.flags == (DEC | (_lib.MOE_LOW_BIT if low_bit else 0))
    return q


def _w64(lin):
    """scales[g(k)] * (w[k] - z[g(k)]) in fp64, unrounded, [K, N], from the library's integer unpack of the checkpoint tensors."""
    lib = _lib.load()
    bits, K, N = lin.bits, lin.infeatures, lin.outfeatures
    w = torch.empty((K, N), dtype=torch.uint8, device=DEV)
    _lib.check(lib.gptq_unpack_weights(lin.qweight.data_ptr(), K, N, bits, w.data_ptr(), None))
    Gn = lin.qzeros.shape[0]
    z = torch.empty((Gn, N), dtype=torch.int32, device=DEV)
    _lib.check(lib.gptq_unpack_zeros(lin.qzeros.data_ptr(), Gn, N, bits, int(lin.resolved_zero_mode() != _lib.ZERO_WRAP), z.data_ptr(), None))
    torch.cuda.synchronize()
    g = lin.g_idx.long()
    return lin.scales.double()[g] * (w.to(torch.int32) - z[g]).double()


def check(q, x, idx, w, dtype, cache=None):
    """test_gpu_moe_decode.check with the W64 above (``cache``: {(expert, projection): W64}, shared by the calls on one set of experts)."""
    cache = {} if cache is None else cache
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
        for p, lin in enumerate(q[e].layers()):
            if (e, p) not in cache:
                cache[(e, p)] = _w64(lin)
        W1, W3, W2 = cache[(e, 0)], cache[(e, 1)], cache[(e, 2)]
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
    print(f"moe low-bit decode T={T} bits={q.bits} {str(dtype)[6:]}: worst err/bound H {worst_h:.3f} out {worst_o:.3f}")
    assert bool((err <= bound).all()), f"out: worst err/bound {worst_o:.3f}"
    return out, hs, pos


GRID = [(8, 2, 256, 512, 32), (8, 2, 256, 512, 128), (8, 2, 256, 512, -1),
        (4, 2, 320, 448, 32), (4, 2, 320, 448, 64), (4, 2, 320, 448, -1),
        (60, 4, 2048, 1408, 128)]


@pytest.mark.parametrize("shape", GRID, ids=lambda s: f"e{s[0]}-h{s[2]}-g{s[4]}")
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("bits", [2, 3])
def test_parity_grid(bits, act, dtype, shape):
    E, topk, H, I, gs = shape
    q = low_bit_decode_experts(E, H, I, bits, gs, act, dtype, seed=bits + gs + E, top_k=topk)
    ref4 = _lib.describe_moe_decode_plan(_plan_twin(q, E, H, I, gs, dtype, act), 1, topk)
    assert ref4["path"] == "decode"                                  # the 4-bit plan takes the shape
    cache = {}
    for T in (1, 2, 3, 4):
        idx, w = _routing(T, E, topk, T + E)
        check(q, _x(T, H, dtype, T), idx, w, dtype, cache)


def _plan_twin(q, E, H, I, gs, dtype, act):
    from test_moe_decode_host import _moe
    return _moe(E, H, I, bits=4, gs=gs, dtype=_lib.DTYPE_ENUM[dtype], act=act)


@pytest.mark.parametrize("bits", [2, 3])
def test_routing_edge_cases(bits):
    dtype = torch.float16
    q = low_bit_decode_experts(8, 256, 512, bits, 128, False, dtype, seed=3)
    cache = {}
    T = 4
    x = _x(T, 256, dtype, 1)
    w = torch.full((T, 2), 0.5, device=DEV)
    # all tokens on one expert: every assignment of the call reads the same table entry and the same strips
    idx = torch.full((T, 2), 5, dtype=torch.int64, device=DEV)
    check(q, x, idx, w, dtype, cache)
    check(q, x, idx[:, :1].contiguous(), torch.ones((T, 1), device=DEV), dtype, cache)          # topk 1
    # indices == E and -1 are dropped; a token with none left gets exactly 0
    idx = torch.tensor([[8, 3], [1, -1], [8, -1], [6, 0]], dtype=torch.int64, device=DEV)
    out, _, pos = check(q, x, idx, w, dtype, cache)
    assert pos.tolist() == [[-1, 1], [2, -1], [-1, -1], [6, 7]]
    assert bool((out[2] == 0).all()) and bool((out[0] != 0).any())
    # a repeated expert within a token's top-k counts twice
    idx = torch.tensor([[4, 4], [1, 1], [7, 7], [0, 0]], dtype=torch.int64, device=DEV)
    out2, _, pos2 = check(q, x, idx, w, dtype, cache)
    assert bool((pos2[:, 0] != pos2[:, 1]).all())
    with torch.no_grad():
        single = moe_forward(q, x, idx[:, :1], torch.ones((T, 1), device=DEV))
    assert torch.allclose(out2.float(), single.float(), rtol=1e-2, atol=1e-3)
    with torch.no_grad():
        out0 = moe_forward(q, x[:0], idx[:0], w[:0])
    assert out0.shape == (0, 256)


@pytest.mark.parametrize("bits,shape,dtype,act", [(3, (60, 4, 2048, 1408, 128), torch.bfloat16, True), (2, (4, 2, 320, 448, 32), torch.float16, True),
                                                  (3, (4, 2, 320, 448, 64), torch.float16, False), (2, (60, 4, 2048, 1408, 128), torch.bfloat16, False)],
                         ids=["b3-e60", "b2-ragged", "b3-ragged", "b2-e60"])
def test_reproducible_permutation_invariant_and_row_independent(bits, shape, dtype, act):
    E, topk, H, I, gs = shape
    q = low_bit_decode_experts(E, H, I, bits, gs, act, dtype, seed=5, top_k=topk)
    T = 4
    x = _x(T, H, dtype, 9)
    idx, w = _routing(T, E, topk, 9)
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


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("bits", [2, 3])
def test_decode_agrees_with_the_grouped_low_bit_path(bits, act):
    """The same experts on both paths, at the tolerance test_gpu_moe_lowbit.py uses between paths."""
    dtype = torch.float16
    E, topk, H, I = 8, 2, 256, 512
    q = low_bit_decode_experts(E, H, I, bits, 64, act, dtype, seed=8)
    ins = [(_x(T, H, dtype, T),) + _routing(T, E, topk, T) for T in (1, 2, 3, 4)]
    with torch.no_grad():
        dec = [moe_forward(q, *a) for a in ins]
    assert q.last_plan["path"] == "decode"
    q.post_init(low_bit=True)                                      # decode off: the grouped low-bit kernels on the checkpoint rows
    assert q._decode_table is None and q.decode_copy_bytes == 0
    for a, d in zip(ins, dec):
        with torch.no_grad():
            g = moe_forward(q, *a)
        assert q.last_plan["path"] == "grouped"
        assert torch.allclose(d.float(), g.float(), rtol=1e-2, atol=1e-3), float((d.float() - g.float()).abs().max())


def _edge_routing(T, E, topk):
    idx, w = _routing(T, E, topk, T + E)
    idx[0, 0] = E
    if T > 1:
        idx[1, 1] = -1
    if T > 2:
        idx[2] = torch.tensor([E, -1], device=DEV)
    return idx, w


@pytest.mark.parametrize("shape", [(8, 2, 256, 512, 128), (4, 2, 320, 448, 32)], ids=["e8", "ragged"])
@pytest.mark.parametrize("bits", [2, 3])
def test_stays_inside_guarded_buffers(bits, shape):
    """x, topk_idx, topk_w, out, h_out and a workspace of exactly gptq_moe_decode_workspace_bytes inside guard bands; bit-identical to moe_forward."""
    dtype = torch.float16
    E, topk, H, I, gs = shape
    q = low_bit_decode_experts(E, H, I, bits, gs, True, dtype, seed=bits)
    lib = _lib.load()
    es = 2
    m = ctypes.byref(q._moe)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for T in (1, 4):
        R = T * topk
        need = int(lib.gptq_moe_decode_workspace_bytes(m, T, topk))
        assert need > 0 and need == q.workspace_bytes(T, topk)
        x = _x(T, H, dtype, T)
        for name, (idx, w) in (("random", _routing(T, E, topk, T)), ("E-and-minus-1", _edge_routing(T, E, topk))):
            with torch.no_grad():
                y_mod, hs_mod, pos_mod = moe_forward(q, x, idx, w, return_intermediate=True)
            gx, _ = G.guarded_like(x, G.guard_for(H * es))
            gi, _ = G.guarded_like(idx, G.guard_for(topk * 8))
            gw, _ = G.guarded_like(w, G.guard_for(topk * 4))
            ws = G.Guarded(need, max(64 << 10, (need + 255) // 256 * 256), 0x00, G.OUT_GUARD, DEV)
            valid = pos_mod >= 0
            for launch in (1, 2):
                go = G.Guarded(T * H * es, G.guard_for(H * es), 0xFF, G.OUT_GUARD, DEV)
                gh = G.Guarded(R * I * es + 4 * R, G.guard_for(I * es), 0xFF, G.OUT_GUARD, DEV)
                _lib.check(lib.gptq_moe_decode_forward(m, q._decode_table.data_ptr(), gx.ptr, gi.ptr, gw.ptr, T, topk, go.ptr, gh.ptr, ws.ptr, need, stream))
                for g, nm in ((gx, "x"), (gi, "topk_idx"), (gw, "topk_w"), (go, "out"), (gh, "h_out"), (ws, f"workspace ({need} bytes = its query)")):
                    g.assert_intact(f"gptq_moe_decode_forward int{bits} T={T} routing={name}: {nm} (launch {launch})")
                assert torch.equal(go.view(dtype, (T, H)), y_mod), (name, launch)
                pos = gh.body[R * I * es:].view(torch.int32).view(T, topk)
                hs = gh.body[:R * I * es].view(dtype).view(R, I)
                assert torch.equal(pos, pos_mod)
                assert torch.equal(hs[pos[valid].long()], hs_mod[pos_mod[valid].long()])


@pytest.mark.parametrize("bits", [2, 3])
def test_the_switch_is_opt_in_and_survives_a_re_init(bits, caplog):
    dtype = torch.float16
    E, topk, H, I = 8, 2, 256, 512
    q = low_bit_decode_experts(E, H, I, bits, 128, False, dtype, seed=1, low_bit=True)
    assert [q.plan(T)["path"] for T in (1, 4, 5, 64, 65)] == ["decode", "decode", "grouped", "grouped", "grouped"]
    assert q.workspace_bytes(4) == int(_lib.load().gptq_moe_decode_workspace_bytes(ctypes.byref(q._moe), 4, topk)) > 0
    q.low_bit_decode_max_tokens = 2
    assert [q.plan(T)["path"] for T in (1, 2, 3, 4)] == ["decode", "decode", "grouped", "grouped"]
    q.low_bit_decode_max_tokens = 4
    q._invalidate()                                                # the tables are rebuilt with the remembered choice
    assert q.plan(1)["path"] == "decode" and q._moe.flags == (DEC | _lib.MOE_LOW_BIT) and q.decode_copy_bytes > 0
    # without low_bit: the composition above the decode range; the flag bits are independent
    q.post_init(low_bit_decode=True)
    assert q._moe.flags == DEC
    assert [q.plan(T)["path"] for T in (1, 4, 5, 70)] == ["decode", "decode", "per_expert", "per_expert"]
    # batch and prefill have no effect on such experts: logged, dropped, the decode copy stays
    caplog.clear()
    q.post_init(batch=True, prefill=True, low_bit=True, low_bit_decode=True)
    assert "post_init(batch=True) has no effect" in caplog.text and "post_init(prefill=True) has no effect" in caplog.text and f"{bits}-bit" in caplog.text
    assert q._decode_table is not None and not q._switches["batch"] and not q._switches["prefill"] and q._live == {"decode"}
    assert [q.plan(T)["path"] for T in (1, 4, 5, 64, 65)] == ["decode", "decode", "grouped", "grouped", "grouped"]
    # without the keyword: as before
    q.post_init(decode_copy=True, batch=True, low_bit=True)
    assert q._decode_table is None and q.decode_copy_bytes == 0 and q._moe.flags == _lib.MOE_LOW_BIT
    q.post_init()
    assert q.plan(1)["path"] == "per_expert" and q._moe.flags == 0


def test_the_keyword_changes_nothing_for_4_bit_experts():
    dtype = torch.float16
    a = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, decode_copy=False)
    b = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, decode_copy=False)
    b.post_init(low_bit_decode=True)
    assert b._decode_table is None and b.decode_copy_bytes == 0
    for T in (1, 4, 5, 70):
        assert a.plan(T) == b.plan(T)
    a.post_init(decode_copy=True)
    b.post_init(decode_copy=True, low_bit_decode=True)
    b.low_bit_decode_max_tokens = 1                                 # (the limit of the 2- / 3-bit forms: not theirs)
    x = _x(4, 256, dtype, 2)
    idx, w = _routing(4, 8, 2, 2)
    for T in (1, 4, 5, 70):
        assert a.plan(T) == b.plan(T)
    with torch.no_grad():
        assert torch.equal(moe_forward(a, x, idx, w), moe_forward(b, x, idx, w))
    assert a.last_plan["path"] == b.last_plan["path"] == "decode"


def test_graph_capture_replays_with_new_inputs():
    dtype = torch.float16
    q = low_bit_decode_experts(8, 256, 512, 3, 32, True, dtype, seed=4)
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


# ---------------------------------------------------------------------------------------------------------------- the tiny models
def test_moe_shared_forward_takes_its_combine_form(tmp_path, monkeypatch):
    """A tiny Qwen2-MoE quantised at 3 bits: the fused shared call declines 3-bit routed experts, so the bound block forward runs the routed experts on
    the new decode path, the shared MLP, and the combine launch; against the fp16 twin's block at the shared tests' tolerance (1e-2 of max(1, |ref|))."""
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    import _tiny_mixtral as TM
    import _tiny_qwen2_moe as TQ
    from autogptq_amd.model_utils import autogptq_post_init
    from autogptq_amd.moe import inject_shared_expert, shared_plan
    monkeypatch.setattr(TM, "BITS", 3)
    monkeypatch.setattr(TQ, "BITS", 3)
    model, twin = TQ.build(tmp_path)
    model, twin = model.to(DEV), twin.to(DEV)
    assert inject_shared_expert(model) == 2
    autogptq_post_init(model, max_input_length=64, expert_low_bit=True, expert_low_bit_decode=True)
    for li, layer in enumerate(model.model.layers):
        blk, ex = layer.mlp, layer.mlp.experts
        assert ex.bits == 3 and ex._decode_table is not None
        shared_layers = tuple(getattr(blk.shared_expert, n) for n in TQ.NAMES)
        d = shared_plan(ex, shared_layers, 1)
        assert d["path"] == "none" and "3-bit routed experts" in d["reason"], d
        for T in (1, 2, 4, 7):
            hs = ((torch.rand((1, T, TQ.H), generator=torch.Generator().manual_seed(T)) - 0.5)).half().to(DEV)
            with torch.no_grad():
                out = blk(hs)
                ref = twin.model.layers[li].mlp(hs)
            assert ex.last_plan["shared"] == "combine" and ex.last_plan["path"] == ("decode" if T <= 4 else "grouped"), (T, ex.last_plan)
            err = (out.float() - ref.float()).abs().max().item()
            assert out.shape == ref.shape and err <= 1e-2 * max(1.0, ref.abs().max().item()), (li, T, err)


def test_tiny_mixtral_at_3_bits_decode_step_capture(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    import _tiny_mixtral as TM
    from transformers import StaticCache
    from autogptq_amd.model_utils import autogptq_post_init, capture_decode_step
    monkeypatch.setattr(TM, "BITS", 3)
    src = TM.fresh_model(0)
    TM.quantize_and_pack(src, False)
    TM.save_checkpoint(src, str(tmp_path), False)
    model, _, qc = TM.load_checkpoint(str(tmp_path))
    assert qc["bits"] == 3
    model = model.to(DEV)
    autogptq_post_init(model, max_input_length=64, expert_low_bit=True, expert_low_bit_decode=True)
    experts = [layer.mlp.experts for layer in model.model.layers]
    assert all(isinstance(ex, QuantMoEExperts) and ex.bits == 3 and ex.decode_copy_bytes > 0 and ex.plan(1)["path"] == "decode" for ex in experts)
    ids = torch.randint(0, 512, (1, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        ref = model.generate(ids, max_new_tokens=8, do_sample=False)[0, 8:]
    cache = StaticCache(config=model.config, max_cache_len=64)
    with torch.no_grad():
        logits = model(ids, past_key_values=cache, use_cache=True).logits
    assert all(ex.last_plan["path"] == "grouped" for ex in experts)
    tok = logits[:, -1].argmax(-1)
    step = capture_decode_step(model, cache)
    assert all(ex.last_plan["path"] == "decode" for ex in experts)
    got = [tok.item()]
    for _ in range(7):
        tok = step(tok.view(1, 1))[:, -1].argmax(-1)
        got.append(tok.item())
    assert got == ref.tolist()
