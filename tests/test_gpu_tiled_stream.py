"""GPU (-m gpu): the K loop of the decode-copy kernel (gemv_tiled_kernel, csrc/gemv_tiled_kernel.cuh) with its rolling refill: behind the first
pass a wave requests chunk c + waves * U into the registers of chunk c as soon as that chunk has been decoded, leaves the loop on its OWN chunk count, and its
last pass is peeled.  What can go wrong there depends on the pass count = chunks / (waves * U) (a chunk = 128 k, 64 k at 8 bits) and on where the strip ends:
  * one pass (nothing to refill), one pass + ONE chunk (15 of 16 waves skip the second pass), 2 passes + 1 chunk, the down projection's ragged third pass;
  * a last chunk with a single live k-slot (K mod 128 = 32);
  * groups of 128 / 64 / 32 k and one whole-K group: the constants address of a chunk within one group, and of a chunk that spans four;
  * the neighbours of a wave's strip: three layers in one launch, two strips per workgroup, the [gate | up] pair form, a K slice (cb / ce of the slice).
Geometries are forced through the tuning (tuning.path = 8, waves, reserved[DEPTH]) and checked with describe_plan.  EVERY output is held against x (fp64) @
W_oracle (fp64) with the tolerance helper of test_gpu_tiled.py; one-hot rows must return the oracle's dequantised rows exactly; the same launch twice must
return the same bits.  Layer widths are multiples of 32 (the packed layout's requirement): 32 (two strips) and 96 (six); three layers in one launch: 32, 96, 64."""
import pytest
import torch

import test_gpu_tiled as TT
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear, forward_multi
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = TT.DEV
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])


def _twice(q, x, t):
    with torch.no_grad():
        y, y2 = q(x, tuning=t), q(x, tuning=t)
    assert torch.equal(y, y2), "the same launch twice gave different bits"
    return y


def _forced(q, M, waves, u, ks=1):
    t = TT._tune(waves, u, ks)                                       # (ks = 1: no K slices, whatever the planner would choose for so few strips)
    d = _lib.describe_plan(q._layer, M, t)
    assert d["kernel"] == "strips" and int(d["ksplit"]) == ks and (int(d["waves"]), int(d["u"])) == (waves, u), d
    return t


def _check(q, W, K, dtype, t, rows, what):
    """Rows of x 1 .. rows[-1]: with the layer's bias (if any) every output; without it every output and the one-hot rows exactly."""
    for M in rows:
        x, hot = TT._x(M, K, dtype, M + K)
        if q.bias is not None:
            TT._assert_all(_twice(q, x, t), x, W, q.bias, dtype, f"{what} M={M} with bias")
        saved, q._layer.bias = q._layer.bias, None
        try:
            y0 = _twice(q, x, t)
        finally:
            q._layer.bias = saved
        for r, k in hot:
            assert torch.equal(y0[r], W[k]), f"one-hot row {r} (k={k}) is not the oracle's W[k]: {what} M={M}"
        TT._assert_all(y0, x, W, None, dtype, f"{what} M={M} without bias")


# 16 waves x 2 chunks = 32 chunks per pass: 32 chunks (one pass), 33 (ONE live chunk in the second pass), 65, 86 (the down projection: 22 of 32 slots live in the third)
@DTYPES
@pytest.mark.parametrize("K,gs", [(4096, 128), (4224, 128), (4224, 64), (4224, 32), (4224, 4224), (8320, 128), (8320, 32), (11008, 128), (11008, 64)])
def test_rolling_refill_16_waves_2_chunks(K, gs, dtype):
    L, q, W = TT._layer(K, 32, gs, dtype, K + gs, bias=True)
    _check(q, W, K, dtype, _forced(q, 1, 16, 2), (1, 2, 3, 4), f"16x2 {K}x32 g{gs}")
    if (K, gs) == (4224, 128):                                       # 5..8 rows: a second A operand per decoded pair, the same loop
        x, hot = TT._x(8, K, dtype, 8)
        y = _twice(q, x, _forced(q, 8, 16, 2))
        TT._assert_all(y, x, W, q.bias, dtype, f"16x2 {K}x32 g{gs} M=8")


# 16 / 16 / 32 chunks per pass: 16 chunks, 17, 32, and 50 with one live k-slot in the last
@DTYPES
@pytest.mark.parametrize("waves,u", [(4, 4), (8, 2), (8, 4)])
@pytest.mark.parametrize("K,gs", [(2048, 128), (2176, 128), (2176, 64), (4096, 128), (4096, 32), (6304, 32), (6304, 6304)])
def test_rolling_refill_small_workgroups(K, gs, waves, u, dtype):
    L, q, W = TT._layer(K, 96, gs, dtype, K + gs + waves + u, bias=(gs == 128))
    _check(q, W, K, dtype, _forced(q, 1, waves, u), (1, 2, 3, 4), f"{waves}x{u} {K}x96 g{gs}")


@DTYPES
@pytest.mark.parametrize("bits,K,gs", [(2, 6304, 6304), (3, 6304, 32), (8, 6304, 32), (8, 2112, 64)])
def test_rolling_refill_other_bit_widths(bits, K, gs, dtype):
    """2 / 3 / 8 bits at a ragged K (8 bits: 64 k per chunk -- 99 chunks, the last with two live k-slots; groups of half a chunk and of one chunk)."""
    L, q, W = TT._layer(K, 96, gs, dtype, K + bits, bits=bits)
    for waves, u in ((4, 4), (16, 2)):
        _check(q, W, K, dtype, _forced(q, 1, waves, u), (1, 4), f"int{bits} {waves}x{u} {K}x96 g{gs}")


@DTYPES
@pytest.mark.parametrize("waves,u", [(16, 2), (4, 4), (8, 4)])
def test_rolling_refill_three_layers_in_one_launch(waves, u, dtype):
    """A wave's refill stays inside its own strip: layers of 2, 6 and 4 strips behind one another in one launch, 17 chunks each."""
    K = 2176
    made = [TT._layer(K, n, 128, dtype, 700 + n) for n in (32, 96, 64)]
    layers = [m[1] for m in made]
    t = TT._tune(waves, u)
    for M in (1, 3):
        x, hot = TT._x(M, K, dtype, M)
        with torch.no_grad():
            ys, ys2 = forward_multi(layers, x, t), forward_multi(layers, x, t)
        for (L, q, W), y, y2 in zip(made, ys, ys2):
            assert torch.equal(y, y2)
            TT._assert_all(y, x, W, None, dtype, f"three layers, N={q.outfeatures} M={M} waves={waves} u={u}")
            for r, k in hot:
                assert torch.equal(y[r], W[k])


@DTYPES
def test_rolling_refill_act_order(dtype):
    K = 2176
    L, q, W = TT._layer(K, 96, 128, dtype, 31, act=True)
    for waves, u in ((4, 4), (16, 2)):
        _check(q, W, K, dtype, _forced(q, 1, waves, u), (1, 3), f"act-order {waves}x{u} {K}x96")


@DTYPES
def test_rolling_refill_two_strips_per_workgroup(dtype):
    K, N = 2176, 3072
    L, q, W = TT._layer(K, N, 128, dtype, 77)
    # 4 / 2 / 8 waves per strip: 16 / 8 / 16 chunks per pass, 17 chunks (two chunks in flight: compiled for this form from 3 rows)
    for waves, u, rows in ((8, 4, (1, 2)), (4, 4, (1, 2)), (16, 2, (3, 4))):
        t = TT._tune(waves, u)
        t.reserved[_lib.LAB.OPT] = 2
        for M in rows:
            d = _lib.describe_plan(q._layer, M, t)
            assert d["kernel"] == "strips" and int(d["strips"]) == N // 32 and (int(d["waves"]), int(d["u"])) == (waves, u), d
        for M in rows:
            x, hot = TT._x(M, K, dtype, M + K)
            y = _twice(q, x, t)
            for r, k in hot:
                assert torch.equal(y[r], W[k]), f"one-hot row {r} (k={k}) is not the oracle's W[k]: two strips per workgroup {waves}x{u} M={M}"
            TT._assert_all(y, x, W, None, dtype, f"two strips per workgroup {waves}x{u} M={M}")


@DTYPES
def test_rolling_refill_pair_form(dtype):
    """[gate | up] with the SiLU * mul epilogue at a ragged K (K mod 128 = 32): the halves of the waves stream two strips N / 32 apart."""
    from autogptq_amd.fused import fuse_gate_up
    K, I, gs = 2208, 352, 32
    Ls = [O.random_quant_layer(K, I, 4, gs, dtype=dtype, seed=K + I + i) for i in range(2)]
    mods = []
    for L in Ls:
        L["scales"] = (L["scales"].float() * 4).to(dtype)             # gate pre-activations of order 1
        m = QuantLinear(4, gs, K, I, False, weight_dtype=dtype)
        m.qweight, m.qzeros, m.scales, m.g_idx = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone()
        mods.append(m)
    fused = fuse_gate_up(*mods).to(DEV)
    q = next(m for m in fused.modules() if isinstance(m, QuantLinear))
    q.post_init()
    mode = O.reference_zero_mode(False, 4)
    Wg, Wu = (O.dequantize(L["qweight"], L["qzeros"], L["scales"], L["g_idx"], 4, mode).to(DEV).double() for L in Ls)
    rtol, atol = {torch.float16: (2e-3, 2e-3), torch.bfloat16: (1.6e-2, 1.6e-2)}[dtype]      # test_gpu_tiled.py: one rounding of the product of two sums
    for M in (1, 3):
        x, _ = TT._x(M, K, dtype, M, hot=False)
        ref = torch.nn.functional.silu(x.double() @ Wg) * (x.double() @ Wu)
        for t in (TT._tune(16, 2), TT._tune(8, 4), TT._tune(8, 2)):
            d = _lib.describe_plan(q._layer, M, t)
            assert (d["kernel"], int(d["pair"])) == ("strips", 1), d
            y = _twice(q, x, t)
            bad = (y.double() - ref).abs() > atol * float(ref.abs().max()) + rtol * ref.abs()
            assert not bool(bad.any()), f"pair form M={M} {d}: {int(bad.sum())}/{bad.numel()} outputs out of tolerance"


@DTYPES
def test_rolling_refill_inside_a_k_slice(dtype):
    """K slices: a wave's chunks are [cb, ce) of its slice, not of the strip -- 65 chunks in two slices, 50 chunks (the last with one live k-slot) in three."""
    for K, gs, waves, u, ks in ((8320, 128, 16, 2, 2), (6304, 32, 4, 4, 3)):
        L, q, W = TT._layer(K, 96, gs, dtype, K + ks, bias=True)
        _check(q, W, K, dtype, _forced(q, 1, waves, u, ks), (1, 3), f"K slices {waves}x{u}x{ks} {K}x96 g{gs}")
