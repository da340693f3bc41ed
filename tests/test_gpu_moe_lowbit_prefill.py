"""GPU: 2- and 3-bit routed experts on the prefill path (QuantMoEExperts.low_bit_prefill = True before post_init -> GPTQ_MOE_LOW_BIT_PREFILL):
gptq_moe_prefill_forward at 65 tokens and more on the experts' decode copy, the launches of the 4-bit prefill path with
moe_panel_lowbit_kernel<T, 2 | 3> as the GEMM.

The checker is test_gpu_moe_prefill.verify: every output of H and of out against the fp64 product of dequantize() with the project's error model
(1/2 + 1/64 ulp + 16 sqrt(K) 2^-24 A), no new constant.  A wrong field, pair order, k position or zero point misses that bound by orders of magnitude.

Shapes (E, topk, H, I), the 4-bit file's: (8, 2, 256, 512) -- 4 k-steps for the pair stage's waves (waves run empty), exactly one per wave in the down
stage; (60, 4, 512, 384) -- every tile partial, 6 down steps; (4, 2, 2048, 768) -- several steps per wave, 12 down steps (the last two waves empty),
group boundaries inside a wave's range at g64 / g128.

The kernels were paid for by folding two template parameters into launch arguments (gemm_f32_kernel's BITS, gemm_reduce_kernel's dtype): the last test
holds their outputs to the bits recorded from the library before the fold (tests/golden/fold_f32_reduce_bits.json)."""
import ctypes
import hashlib
import json
import logging
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.moe import moe_forward, moe_shared_forward  # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear  # noqa: E402
from test_gpu_moe import _fill, _routing  # noqa: E402
from test_gpu_moe import make_experts as plain_experts  # noqa: E402
from test_gpu_moe_prefill import DEV, SHAPES, _direct, _x, verify  # noqa: E402

pytestmark = pytest.mark.gpu
PRE = getattr(_lib, "MOE_LOW_BIT_PREFILL", 0x20)
BAT = _lib.MOE_LOW_BIT_BATCH
_CACHE = {}


def low_bit_prefill_experts(E, H, I, bits, gs, act, dtype, seed=0, top_k=2, **post_init):
    q = plain_experts(E, H, I, bits, gs, act, dtype, seed=seed, top_k=top_k)
    assert q.plan(65)["path"] == "per_expert" and q._decode_table is None         # without the switch: as before
    q.low_bit_prefill = True
    q.post_init(**post_init)
    assert q._decode_table is not None and q.decode_copy_bytes > 0 and q._moe_batch.flags & PRE and not q._moe.flags & PRE
    return q


def shared(bits, dtype=torch.float16, act=False):
    """One set of (8, 2, 256, 512) g128 experts per (bits, dtype, act) with low_bit and backward on as well, shared by the tests that only read them."""
    key = (bits, dtype, act)
    if key not in _CACHE:
        _CACHE[key] = low_bit_prefill_experts(8, 256, 512, bits, 128, act, dtype, seed=70 + bits, low_bit=True, backward=True)
    return _CACHE[key]


def check(q, x, idx, w, dtype):
    """Run the prefill path with its intermediate and check H and out against the fp64 oracles; returns (out, H, pos)."""
    T, topk = idx.shape
    plan = q.plan(T, topk)
    gate, up, down = q.projections()
    R = T * topk
    assert plan["path"] == "prefill" and plan["bits"] == q.bits and plan["bm"] == 64, plan
    assert plan["launches"] == 5 + int(any(l._layer.perm for l in down)), plan
    assert plan["tiles"] == R // 64 + min(q.num_experts, R) and plan["waves"] == 8 and plan["nt_pair"] == 2 and plan["nt_down"] == 4, plan
    assert plan["waves_pair"] == (4 if any(l._layer.perm for l in gate + up) else 8), plan
    with torch.no_grad():
        out, hs, pos = moe_forward(q, x, idx, w, return_intermediate=True)
    assert q.last_plan["path"] == "prefill"
    verify(q, x, idx, w, dtype, out, hs, pos, tag="low-bit prefill")
    return out, hs, pos


@pytest.mark.parametrize("shape", SHAPES, ids=["e8", "e60", "e4"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [64, 128, -1])
@pytest.mark.parametrize("bits", [2, 3])
def test_parity_grid(bits, gs, act, dtype, shape):
    E, topk, H, I = shape
    q = low_bit_prefill_experts(E, H, I, bits, gs, act, dtype, seed=bits + gs + E, top_k=topk)
    for T in (65, 100, 129, 300) + ((520,) if E == 4 else ()):      # 520 on four experts: four full tiles plus a short one per expert
        idx, w = _routing(T, E, topk, T + E)
        check(q, _x(T, H, dtype, T), idx, w, dtype)
    assert q.plan(64, topk)["path"] == "per_expert" and q.plan(4, topk)["path"] == "per_expert"


@pytest.mark.parametrize("bits", [2, 3])
def test_routing_edge_cases(bits):
    dtype = torch.float16
    E, topk, H, I = SHAPES[0]
    q = shared(bits)
    T = 130
    x = _x(T, H, dtype, 1)
    w = torch.full((T, 2), 0.5, device=DEV)
    # every token to the same two experts: each gets 130 rows = tiles of 64, 64 and 2; six experts nobody picks
    check(q, x, torch.tensor([[5, 2]] * T, dtype=torch.int64, device=DEV), w, dtype)
    # every token on ONE expert, twice: 260 rows of one expert
    check(q, x, torch.tensor([[5, 5]] * T, dtype=torch.int64, device=DEV), w, dtype)
    # an expert with exactly 64 rows and one with 65 (a full tile; a full tile and a tile of one row); expert 4 is picked by nobody
    first = [3] * 64 + [6] * 65 + [0]
    check(q, x, torch.tensor([[a, 7] for a in first], dtype=torch.int64, device=DEV), w, dtype)
    # indices == E, -1 and far outside are dropped; a token with none left gets exactly 0 and pos == -1
    idx, _ = _routing(T, E, topk, 17)
    idx[0] = torch.tensor([8, 3], device=DEV)
    idx[1] = torch.tensor([1, -1], device=DEV)
    idx[2] = torch.tensor([8, -1], device=DEV)
    idx[4] = torch.tensor([2, 1 << 40], device=DEV)
    idx[3::7, 0] = E
    out, _, pos = check(q, x, idx, w, dtype)
    assert pos[2].tolist() == [-1, -1] and pos[0, 0].item() == -1 and pos[1, 1].item() == -1 and pos[4, 1].item() == -1
    assert bool((out[2] == 0).all()) and bool((out[0] != 0).any())


@pytest.mark.parametrize("bits", [2, 3])
def test_reproducible_and_row_independent(bits):
    """A token's output bits depend only on its own x, indices and weights: not on the rest of the batch, not on T (65 or 300)."""
    dtype = torch.bfloat16
    E, topk, H, I = SHAPES[2]
    q = low_bit_prefill_experts(E, H, I, bits, 128, True, dtype, seed=5, top_k=topk)
    T = 300
    x = _x(T, H, dtype, 9)
    idx, w = _routing(T, E, topk, 9)
    with torch.no_grad():
        a = moe_forward(q, x, idx, w)
        b = moe_forward(q, x, idx, w)
        assert q.last_plan["path"] == "prefill"
        first = moe_forward(q, x[:65], idx[:65], w[:65])             # the same tokens at T = 65
        assert q.last_plan["path"] == "prefill"
        x2, (idx2, w2) = _x(T, H, dtype, 10), _routing(T, E, topk, 10)      # ... and with another batch around them
        x2[:65], idx2[:65], w2[:65] = x[:65], idx[:65], w[:65]
        other = moe_forward(q, x2, idx2, w2)
    assert torch.equal(a, b)
    assert torch.equal(a[:65], first) and torch.equal(a[:65], other[:65]) and not torch.equal(a[65:], other[65:])


@pytest.mark.parametrize("bits", [2, 3])
def test_prefill_agrees_with_grouped_low_bit_and_per_expert_and_allocates_nothing(bits):
    """The three routes compute the same fp32 sums in different orders: each is within the bound of the fp64 oracle, so two of them differ by at most two
    bounds -- checked through verify() on the prefill and the grouped outputs, and directly against the composition's rows."""
    from autogptq_amd.model_utils import autogptq_post_init
    from autogptq_amd.moe import _per_expert
    dtype = torch.float16
    E, topk, H, I = SHAPES[0]
    q = plain_experts(E, H, I, bits, 64, False, dtype, seed=8)
    grouped = plain_experts(E, H, I, bits, 64, False, dtype, seed=8)
    autogptq_post_init(torch.nn.Sequential(q), max_input_length=300, expert_low_bit=True, expert_low_bit_prefill=True)
    autogptq_post_init(torch.nn.Sequential(grouped), max_input_length=300, expert_low_bit=True)
    assert q.low_bit_prefill is True and grouped.low_bit_prefill is False and grouped._decode_table is None
    assert q.workspace_bytes(300) == int(_lib.load().gptq_moe_prefill_workspace_bytes(ctypes.byref(q._moe_batch), 300, topk))
    for T in (65, 300):
        x = _x(T, H, dtype, T)
        idx, w = _routing(T, E, topk, T)
        assert q.plan(T)["path"] == "prefill" and grouped.plan(T)["path"] == "grouped" and q.plan(64)["path"] == "grouped"
        with torch.no_grad():
            ref = _per_expert(grouped, x, idx, w)
            g, gh, gpos = moe_forward(grouped, x, idx, w, return_intermediate=True)
            moe_forward(q, x, idx, w)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            out = moe_forward(q, x, idx, w)
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated() - before
            _, ph, ppos = moe_forward(q, x, idx, w, return_intermediate=True)
        assert q.last_plan["path"] == "prefill" and grouped.last_plan["path"] == "grouped"
        assert grown <= out.numel() * out.element_size() + 512, grown
        verify(q, x, idx, w, dtype, out, ph, ppos, tag="low-bit prefill")
        verify(grouped, x, idx, w, dtype, g, gh, gpos, tag="low-bit grouped")
        # the composition rounds every expert's y to T before the weighted sum: the tolerance the batch path's test of the same kind uses
        assert torch.allclose(out.float(), ref.float(), rtol=2e-2, atol=2e-3), float((out.float() - ref.float()).abs().max())
        assert torch.allclose(out.float(), g.float(), rtol=2e-2, atol=2e-3), float((out.float() - g.float()).abs().max())


@pytest.mark.parametrize("bits,act", [(3, True), (2, False), (3, False), (2, True)], ids=["b3-act", "b2-seq", "b3-seq", "b2-act"])
def test_c_abi_takes_any_token_count_and_stays_inside_its_buffers(bits, act):
    dtype = torch.float16
    E, topk, H, I = SHAPES[0]
    q = low_bit_prefill_experts(E, H, I, bits, 64, act, dtype, seed=12)
    raw = types.SimpleNamespace(_moe=q._moe_batch, _decode_table=q._decode_table, hidden_dim=H, intermediate_dim=I)      # the struct that carries the bit
    for T in (1, 5, 64, 65):
        x = _x(T, H, dtype, T)
        idx, w = _routing(T, E, topk, T)
        out, hs, pos = _direct(raw, x, idx, w, dtype)
        verify(q, x, idx, w, dtype, out, hs, pos, tag="low-bit prefill (C ABI)")
    # x, topk_idx, topk_w, out, h_out and a workspace of exactly its query inside guard bands: all guards intact, same bits as moe_forward
    T = 129
    x = _x(T, H, dtype, T)
    idx, w = _routing(T, E, topk, T)
    idx[::5, 0] = E                                        # dropped assignments: sorted rows past the count stay unwritten and unread
    with torch.no_grad():
        y_mod, hs_mod, pos_mod = moe_forward(q, x, idx, w, return_intermediate=True)
    assert q.last_plan["path"] == "prefill"
    out, hs, pos = _direct(raw, x, idx, w, dtype, guarded=True)
    valid = pos_mod >= 0
    assert torch.equal(out, y_mod) and torch.equal(pos, pos_mod)
    assert torch.equal(hs[pos[valid].long()], hs_mod[pos_mod[valid].long()])


@pytest.mark.parametrize("bits,act", [(3, True), (2, False)], ids=["b3-act", "b2-seq"])
def test_graph_capture_replays_with_new_inputs(bits, act):
    dtype = torch.float16
    E, topk, H, I = SHAPES[0]
    q = low_bit_prefill_experts(E, H, I, bits, 64, act, dtype, seed=4)
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
    for r in range(2):
        xn = _x(T, H, dtype, r)
        idn, wn = _routing(T, E, topk, 100 + r)
        x.copy_(xn), idx.copy_(idn), w.copy_(wn)
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = moe_forward(q, xn, idn, wn)
        assert torch.equal(out, eager), r


def test_backward_node_runs_the_prefill_path_in_its_forward():
    """_MoEBackward's forward is the no-grad path plan(T) names: the prefill path at T = 65, bit for bit; its backward is the grouped backward (low_bit)."""
    from test_gpu_moe_backward import check_backward
    dtype, T = torch.float16, 65
    q = shared(3, dtype)
    assert q._grad_table is not None and q._moe.flags == _lib.MOE_LOW_BIT
    x = _x(T, 256, dtype, 3)
    idx, w = _routing(T, 8, 2, 3)
    gy = _x(T, 256, dtype, 4)
    with torch.no_grad():
        want = moe_forward(q, x, idx, w)
    assert q.last_plan["path"] == "prefill"
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = moe_forward(q, xg, idx, wg)
    assert q.last_plan["path"] == "prefill" and q.last_plan["backward"] == "grouped", q.last_plan
    assert torch.equal(out.detach(), want)
    out.backward(gy)
    dx, dw = check_backward(q, x, idx, w, gy)                      # the C entry point against its fp64 oracle ...
    assert torch.equal(xg.grad, dx) and torch.equal(wg.grad, dw)   # ... and the node returns that call's answers


def test_moe_shared_forward_combine_form_runs_the_prefill_path():
    dtype, T = torch.float16, 65
    H, Is = 256, 320
    q = shared(3, dtype)
    gen = torch.Generator().manual_seed(1070)
    layers = []
    for k, n in ((H, Is), (H, Is), (Is, H)):
        l = QuantLinear(4, 64, k, n, False, weight_dtype=dtype)
        _fill(l, gen, False)
        layers.append(l.to(DEV))
    for l in layers:
        l.post_init()
    layers = tuple(layers)
    gw = ((torch.rand((1, H), generator=gen) - 0.5) * 0.25).to(dtype).to(DEV)
    x = _x(T, H, dtype, 5)
    idx, w = _routing(T, 8, 2, 5)
    with torch.no_grad():
        out = moe_shared_forward(q, layers, gw, x, idx, w)
        assert q.last_plan["shared"] == "combine" and q.last_plan["path"] == "prefill", q.last_plan
        routed = moe_forward(q, x, idx, w)
        ys = layers[2](torch.nn.functional.silu(layers[0](x)) * layers[1](x))
    ref = routed.double() + torch.sigmoid(x.double() @ gw.double().t()) * ys.double()
    assert float((out.double() - ref).abs().max()) <= 2e-2 * max(1.0, float(ref.abs().max()))      # (the tolerance of the shared tests' combine form)


@pytest.mark.parametrize("bits", [2, 3])
def test_the_switch_is_opt_in_and_composes(bits, caplog):
    dtype = torch.float16
    q = plain_experts(8, 256, 512, bits, 128, False, dtype, seed=7)
    # without the attribute: plan(T) and the log lines are what they were
    caplog.set_level(logging.WARNING, logger="autogptq_amd.moe")
    q.post_init(prefill=True, low_bit=True)
    assert "post_init(prefill=True) has no effect" in caplog.text and f"{bits}-bit" in caplog.text and "low_bit_prefill" not in caplog.text
    assert q._decode_table is None and q.decode_copy_bytes == 0 and q._moe.flags == _lib.MOE_LOW_BIT and q._moe_batch is None
    assert [q.plan(T)["path"] for T in (1, 64, 65, 300)] == ["grouped"] * 4
    q.post_init()
    assert [q.plan(T)["path"] for T in (1, 65, 300)] == ["per_expert"] * 3 and q._moe.flags == 0
    # the attribute alone: the prompt band, the composition below it; prefill=True next to it still says it has no effect
    q.low_bit_prefill = True
    caplog.clear()
    q.post_init(prefill=True)
    assert "post_init(prefill=True) has no effect" in caplog.text and not q._switches["prefill"] and "prefill" in q._live
    assert [q.plan(T)["path"] for T in (1, 4, 5, 64, 65, 300)] == ["per_expert"] * 4 + ["prefill"] * 2
    assert q._moe.flags == 0 and q._moe_batch.flags == PRE
    # the whole ladder: decode up to 4, batch 5..64, prefill from 65
    q.low_bit_batch = True
    q.post_init(low_bit=True, low_bit_decode=True)
    assert [q.plan(T)["path"] for T in (1, 4, 5, 64, 65, 300)] == ["decode", "decode", "batch", "batch", "prefill", "prefill"]
    assert q._moe.flags == (_lib.MOE_LOW_BIT | _lib.MOE_LOW_BIT_DECODE) and q._moe_batch.flags == (q._moe.flags | BAT | PRE)
    # the threshold can be raised per module (and never lowered below 65)
    q.low_bit_prefill_min_tokens = 200
    assert q.plan(65)["path"] == "grouped" and q.plan(129)["path"] == "grouped" and q.plan(199)["path"] == "grouped" and q.plan(200)["path"] == "prefill"
    q.low_bit_prefill_min_tokens = 1
    assert q.plan(64)["path"] == "batch" and q.plan(65)["path"] == "prefill"
    q.low_bit_prefill_min_tokens = 65
    q._invalidate()                                                # the tables are rebuilt with the remembered choice
    assert q.plan(65)["path"] == "prefill" and q.plan(5)["path"] == "batch" and q.plan(1)["path"] == "decode" and q.decode_copy_bytes > 0
    # experts the prefill plan declines: said once, the attribute is unset, they behave as without it
    for kw, frag in ((dict(I=192, gs=64), "multiples of 128"), (dict(I=512, gs=32), "group_size 32")):
        odd = plain_experts(8, 256, kw["I"], bits, kw["gs"], False, dtype, seed=1)
        odd.low_bit_prefill = True
        caplog.clear()
        odd.post_init(low_bit=True)
        assert caplog.text.count("low_bit_prefill = True has no effect") == 1 and frag in caplog.text, caplog.text
        assert odd.low_bit_prefill is False and odd.plan(300)["path"] == "grouped" and odd.decode_copy_bytes == 0


def test_the_attribute_changes_nothing_for_4_bit_experts():
    from test_gpu_moe_prefill import make_experts
    dtype = torch.float16
    a = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, prefill=True)
    b = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, prefill=False)
    b.low_bit_prefill = True
    b.post_init()
    assert b._decode_table is None and b._moe_batch is None and b.plan(100)["path"] == "grouped"
    b.post_init(prefill=True)
    assert b._moe_batch is None and b._moe.flags == 0
    x = _x(100, 256, dtype, 2)
    idx, w = _routing(100, 8, 2, 2)
    for T in (1, 5, 64, 65, 300):
        assert a.plan(T) == b.plan(T)
    with torch.no_grad():
        assert torch.equal(moe_forward(a, x, idx, w), moe_forward(b, x, idx, w))


# ---- what paid for the four kernels ---------------------------------------------------------------------------------------------------------------
def fold_cases():
    """(name, output tensor) of the launches whose kernels lost a template parameter: gemm_f32_kernel at every width (fp32 layers above 8 rows, forced
    onto the matrix-core kernel) and gemm_reduce_kernel behind the K-split strip16 / skinny / tiled GEMMs of fp16 and bf16 layers without a decode copy.
    Inputs and weights are seeded on the CPU, so the bits are a function of the library alone."""
    from oracle import gptq_oracle as O
    from test_gpu_parity import _module_from, _tuning
    for bits, gs, K, N, M, act in ((2, 16, 256, 96, 64, False), (3, 32, 1024, 256, 130, True), (4, 128, 1024, 512, 9, False), (8, 32, 512, 384, 300, True)):
        L = O.random_quant_layer(K, N, bits, gs, act_order=act, dtype=torch.float32, seed=bits + K + N + M, bias=True)
        q = _module_from(L["qweight"], L["qzeros"], L["scales"], L["g_idx"] if act else None, L["bias"], bits, gs)
        q.post_init()
        x = (torch.rand(M, K, generator=torch.Generator().manual_seed(M)) - 0.5).float()
        with torch.no_grad():
            yield f"f32_b{bits}_m{M}", q(x.to(DEV), tuning=_tuning(path=3))
    for dtype in (torch.float16, torch.bfloat16):
        K, N = 2048, 512
        L = O.random_quant_layer(K, N, 4, 128, dtype=dtype, seed=11, bias=True)
        q = _module_from(L["qweight"], L["qzeros"], L["scales"], None, L["bias"], 4, 128)
        q.post_init(tiled=False)                                   # checkpoint rows only: the K-split GEMMs and their reduction
        for M, kernel in ((16, "strip16"), (48, "skinny64"), (128, "tiled")):
            d = _lib.describe_plan(q._layer, M)
            assert d["kernel"] == kernel and d["ksplit"] > 1, d
            x = (torch.rand(M, K, generator=torch.Generator().manual_seed(M)) - 0.5).to(dtype)
            with torch.no_grad():
                yield f"reduce_{str(dtype)[6:]}_{kernel}_m{M}", q(x.to(DEV))


def fold_digests():
    return {name: hashlib.sha256(y.contiguous().cpu().numpy().tobytes() if y.dtype != torch.bfloat16 else y.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()
            for name, y in fold_cases()}


def test_the_folds_that_paid_leave_every_output_bit_as_it_was():
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fold_f32_reduce_bits.json")))
    got = fold_digests()
    assert set(got) == set(golden["sha256"]) and len(got) == 10
    assert got == golden["sha256"], {k: (got[k], golden["sha256"][k]) for k in got if got[k] != golden["sha256"][k]}
