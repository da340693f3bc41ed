"""GPU: 2- and 3-bit routed experts on the batch path (QuantMoEExperts.low_bit_batch = True before post_init -> GPTQ_MOE_LOW_BIT_BATCH):
gptq_moe_batch_forward at 5..64 tokens on the experts' decode copy, the launches of the 4-bit batch path with moe_rows_lowbit_kernel<T, 2 | 3> as the GEMM.

The checker is test_gpu_moe_batch.check: every output of H and of out against the fp64 product of dequantize() with the project's error model, C = 16.
A wrong field, pair order, k position or zero point misses that bound by orders of magnitude.

Shapes: the smallest at which the split of K over the waves can go wrong (chunks of 128 k; waves = min(8, chunks / 2), no wave without a chunk):
  (E 8, topk 2, H 256, I 512)     2 chunks -> one wave in the pair stage, 4 chunks -> two waves in the down stage; groups of 32, of 128, one group
  (E 4, topk 2, H 640, I 384)     5 chunks -> 2 waves of 3 + 2 (ragged), 3 chunks -> 1 wave; groups of 64 (the half-chunk record offsets), one group
  (E 60, topk 4, H 2048, I 1408)  16 chunks -> 8 waves x 2, 11 chunks -> 4 waves of 3, 3, 3, 2; many experts with few rows each"""
import logging
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.moe import moe_forward, moe_shared_forward  # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear  # noqa: E402
from test_gpu_moe import _fill, _routing  # noqa: E402
from test_gpu_moe import make_experts as plain_experts  # noqa: E402
from test_gpu_moe_batch import DEV, _x, check  # noqa: E402

pytestmark = pytest.mark.gpu
BAT = getattr(_lib, "MOE_LOW_BIT_BATCH", 0x10)
_CACHE = {}


def low_bit_batch_experts(E, H, I, bits, gs, act, dtype, seed=0, top_k=2, **post_init):
    q = plain_experts(E, H, I, bits, gs, act, dtype, seed=seed, top_k=top_k)
    assert q.plan(5)["path"] == "per_expert" and q._decode_table is None          # without the switch: as before
    q.low_bit_batch = True
    q.post_init(**post_init)
    assert q._decode_table is not None and q.decode_copy_bytes > 0 and q._moe_batch.flags & BAT and not q._moe.flags & BAT
    return q


def shared(bits, dtype=torch.float16, act=False):
    """One set of (8, 2, 256, 512) g128 experts per (bits, dtype, act) with low_bit and backward on as well, shared by the tests that only read them."""
    key = (bits, dtype, act)
    if key not in _CACHE:
        _CACHE[key] = low_bit_batch_experts(8, 256, 512, bits, 128, act, dtype, seed=60 + bits, low_bit=True, backward=True)
    return _CACHE[key]


GRID = [((8, 2, 256, 512), 32), ((8, 2, 256, 512), 128), ((8, 2, 256, 512), -1), ((4, 2, 640, 384), 64), ((4, 2, 640, 384), -1), ((60, 4, 2048, 1408), 128)]
TS = (5, 7, 16, 33, 64)


@pytest.mark.parametrize("shape,gs", GRID, ids=["e8-g32", "e8-g128", "e8-one", "e4-g64", "e4-one", "e60-g128"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("bits", [2, 3])
def test_parity_grid(bits, act, dtype, shape, gs):
    E, topk, H, I = shape
    q = low_bit_batch_experts(E, H, I, bits, gs, act, dtype, seed=bits + gs + E, top_k=topk)
    d = q.plan(5, topk)
    assert d["bits"] == bits and d["waves_pair"] == {256: 1, 640: 2, 2048: 8}[H] and d["waves_down"] == {512: 2, 384: 1, 1408: 4}[I], d
    for T in TS:
        idx, w = _routing(T, E, topk, T + E)
        check(q, _x(T, H, dtype, T), idx, w, dtype, act)          # (prints the worst error / bound of H and of out)
    assert q.plan(4, topk)["path"] == "per_expert" and q.plan(65, topk)["path"] == "per_expert"


@pytest.mark.parametrize("bits", [2, 3])
def test_routing_edge_cases(bits):
    dtype = torch.float16
    q = shared(bits)
    T = 64
    x = _x(T, 256, dtype, 1)
    w = torch.full((T, 2), 0.5, device=DEV)
    # every token on one expert (twice): 128 rows = eight full tiles of one expert, every other expert empty
    check(q, x, torch.tensor([[5, 5]] * T, dtype=torch.int64, device=DEV), w, dtype)
    # an expert with exactly 16 rows and one with 17 (a full tile; a full tile and a tile of one row)
    first = [3] * 16 + [6] * 17 + [0] * 31
    check(q, x, torch.tensor([[a, 7] for a in first], dtype=torch.int64, device=DEV), w, dtype)
    # ids outside [0, E) are dropped; a token with no valid expert gets exactly 0 and pos == -1
    T = 6
    x, w = x[:T], w[:T]
    idx = torch.tensor([[8, 3], [1, -1], [8, -1], [6, 0], [2, 2], [3, 1 << 40]], dtype=torch.int64, device=DEV)
    out, _, pos = check(q, x, idx, w, dtype)
    assert pos[2].tolist() == [-1, -1] and pos[0, 0].item() == -1 and pos[1, 1].item() == -1 and pos[5, 1].item() == -1
    assert bool((out[2] == 0).all()) and bool((out[0] != 0).any())


@pytest.mark.parametrize("bits", [2, 3])
def test_reproducible_and_row_independent(bits):
    dtype = torch.bfloat16
    q = low_bit_batch_experts(60, 2048, 1408, bits, 128, True, dtype, seed=5, top_k=4)
    T = 40
    x = _x(T, 2048, dtype, 9)
    idx, w = _routing(T, 60, 4, 9)
    with torch.no_grad():
        a = moe_forward(q, x, idx, w)
        b = moe_forward(q, x, idx, w)
        five = moe_forward(q, x[:5], idx[:5], w[:5])
    assert q.last_plan["path"] == "batch"
    assert torch.equal(a, b)
    assert torch.equal(a[:5], five)


@pytest.mark.parametrize("bits", [2, 3])
def test_batch_agrees_with_grouped_low_bit_and_per_expert_and_allocates_nothing(bits):
    from autogptq_amd.model_utils import autogptq_post_init
    from autogptq_amd.moe import _per_expert
    dtype = torch.float16
    q = plain_experts(8, 256, 512, bits, 64, False, dtype, seed=8)
    grouped = plain_experts(8, 256, 512, bits, 64, False, dtype, seed=8)
    autogptq_post_init(torch.nn.Sequential(q), max_input_length=64, expert_low_bit=True, expert_low_bit_batch=True)
    autogptq_post_init(torch.nn.Sequential(grouped), max_input_length=64, expert_low_bit=True)
    assert q.low_bit_batch is True and grouped.low_bit_batch is False and grouped._decode_table is None
    for T in (5, 16, 64):
        x = _x(T, 256, dtype, T)
        idx, w = _routing(T, 8, 2, T)
        assert q.plan(T)["path"] == "batch" and grouped.plan(T)["path"] == "grouped"
        with torch.no_grad():
            ref = _per_expert(grouped, x, idx, w)
            g = moe_forward(grouped, x, idx, w)
            moe_forward(q, x, idx, w)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            out = moe_forward(q, x, idx, w)
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated() - before
        assert q.last_plan["path"] == "batch" and grouped.last_plan["path"] == "grouped"
        assert grown <= out.numel() * out.element_size() + 512, grown
        assert torch.allclose(out.float(), g.float(), rtol=2e-2, atol=2e-3), float((out.float() - g.float()).abs().max())
        assert torch.allclose(out.float(), ref.float(), rtol=2e-2, atol=2e-3), float((out.float() - ref.float()).abs().max())


@pytest.mark.parametrize("bits,act", [(3, True), (2, False)], ids=["b3-act", "b2-seq"])
def test_graph_capture_replays_with_new_inputs(bits, act):
    dtype = torch.float16
    q = low_bit_batch_experts(8, 256, 512, bits, 32, act, dtype, seed=4)
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


def test_backward_node_runs_the_batch_path_in_its_forward():
    """_MoEBackward's forward is the no-grad path plan(T) names: the batch path at T = 16, bit for bit; its backward is the grouped backward (low_bit)."""
    from test_gpu_moe_backward import check_backward
    dtype, T = torch.float16, 16
    q = shared(3, dtype)
    assert q._grad_table is not None and q._moe.flags == _lib.MOE_LOW_BIT
    x = _x(T, 256, dtype, 3)
    idx, w = _routing(T, 8, 2, 3)
    gy = _x(T, 256, dtype, 4)
    with torch.no_grad():
        want = moe_forward(q, x, idx, w)
    assert q.last_plan["path"] == "batch"
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = moe_forward(q, xg, idx, wg)
    assert q.last_plan["path"] == "batch" and q.last_plan["backward"] == "grouped", q.last_plan
    assert torch.equal(out.detach(), want)
    out.backward(gy)
    dx, dw = check_backward(q, x, idx, w, gy)                      # the C entry point against its fp64 oracle ...
    assert torch.equal(xg.grad, dx) and torch.equal(wg.grad, dw)   # ... and the node returns that call's answers


def test_moe_shared_forward_combine_form_runs_the_batch_path():
    dtype, T = torch.float16, 16
    bits, gs, H, Is = 3, 128, 256, 320
    q = shared(bits, dtype)
    gen = torch.Generator().manual_seed(1060)
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
        assert q.last_plan["shared"] == "combine" and q.last_plan["path"] == "batch", q.last_plan
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
    q.post_init(batch=True, low_bit=True)
    assert "post_init(batch=True) has no effect" in caplog.text and f"{bits}-bit" in caplog.text and "low_bit_batch" not in caplog.text
    assert q._decode_table is None and q.decode_copy_bytes == 0 and q._moe.flags == _lib.MOE_LOW_BIT and q._moe_batch is None
    assert [q.plan(T)["path"] for T in (1, 4, 5, 64, 65)] == ["grouped"] * 5
    q.post_init()
    assert [q.plan(T)["path"] for T in (1, 5, 64)] == ["per_expert"] * 3 and q._moe.flags == 0
    # the attribute alone: the batch band, the composition around it; batch=True next to it still says it has no effect
    q.low_bit_batch = True
    caplog.clear()
    q.post_init(batch=True)
    assert "post_init(batch=True) has no effect" in caplog.text and not q._switches["batch"] and "batch" in q._live
    assert [q.plan(T)["path"] for T in (1, 4, 5, 64, 65)] == ["per_expert", "per_expert", "batch", "batch", "per_expert"]
    assert q._moe.flags == 0 and q._moe_batch.flags == BAT
    # with low_bit_decode and low_bit: decode up to 4, batch 5..64, grouped beyond; the band can be narrowed per module
    q.post_init(low_bit=True, low_bit_decode=True)
    assert [q.plan(T)["path"] for T in (1, 4, 5, 64, 65)] == ["decode", "decode", "batch", "batch", "grouped"]
    assert q._moe.flags == (_lib.MOE_LOW_BIT | _lib.MOE_LOW_BIT_DECODE) and q._moe_batch.flags == (q._moe.flags | BAT)
    q.low_bit_batch_max_tokens = 16
    assert q.plan(16)["path"] == "batch" and q.plan(17)["path"] == "grouped"
    q.low_bit_batch_max_tokens = 64
    q._invalidate()                                                # the tables are rebuilt with the remembered choice
    assert q.plan(5)["path"] == "batch" and q.plan(1)["path"] == "decode" and q.decode_copy_bytes > 0
    # experts the batch plan declines: said once, the attribute is unset, they behave as without it
    odd = plain_experts(8, 256, 192, bits, 64, False, dtype, seed=1)          # I = 192 is not a multiple of 128
    odd.low_bit_batch = True
    caplog.clear()
    odd.post_init(low_bit=True)
    assert "low_bit_batch = True has no effect" in caplog.text and "multiples of 128" in caplog.text
    assert odd.low_bit_batch is False and odd.plan(16)["path"] == "grouped" and odd.decode_copy_bytes == 0


def test_the_attribute_changes_nothing_for_4_bit_experts():
    from test_gpu_moe_batch import make_experts
    dtype = torch.float16
    a = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, batch=True)
    b = make_experts(8, 256, 512, 4, 128, False, dtype, seed=7, batch=False)
    b.low_bit_batch = True
    b.post_init()
    assert b._decode_table is None and b._moe_batch is None and b.plan(16)["path"] == "grouped"
    b.post_init(batch=True)
    assert b._moe_batch is None and b._moe.flags == 0
    x = _x(16, 256, dtype, 2)
    idx, w = _routing(16, 8, 2, 2)
    for T in (1, 5, 64, 65):
        assert a.plan(T) == b.plan(T)
    with torch.no_grad():
        assert torch.equal(moe_forward(a, x, idx, w), moe_forward(b, x, idx, w))
