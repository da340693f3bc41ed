"""GPU (-m gpu): the head of the decode-copy kernel (gemv_tiled_kernel, csrc/gemv_tiled_kernel.cuh) in front of its first weight load.

The head reads its arguments in one batch, chooses the layer of a multi-layer launch with scalar compares and selects (the weight / constant pointers of all
four layers are in the batch), issues the x and constant DMAs in straight-line code for zero, one or two pieces per lane (a loop from the third on) and keeps
the K-slice decomposition in a cold block.  Each of those paths is forced here (tuning.path = 8, waves, reserved[DEPTH], reserved[OPT], ksplit) and EVERY
output is held against x (fp64) @ W_oracle (fp64) with the helpers of test_gpu_tiled.py; where a layer has no bias, one-hot rows must return the oracle's
dequantised rows exactly; the same launch twice must return the same bits.

  * layer selector: 1..4 layers of 6, 2, 10 and 4 strips in one launch -- every workgroup index, each boundary and the fourth layer -- bias on some layers
    only (the tail's bias / out / N come from a load indexed by the selector), 1..4 rows, fp16 / bf16;
  * DMA trip counts at forced (waves, chunks in flight): fewer x pieces than one wave (K = 256), a ragged K with one piece per lane for some waves only
    (K = 4160), two pieces per lane at 16 waves (K = 8320), the loop beyond two (K = 16640); K slices switched off (ksplit = 1) so that the whole K is staged;
  * forced K slices (the cold decomposition);
  * the other forms that share the head: two strips per workgroup, the [gate | up] pair, act-order, 2 / 3 / 8 bits, the 5..8-row form;
  * a captured graph of three launches replays to the eager bits."""
import pytest
import torch

import test_gpu_tiled as TT
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear, forward_multi
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = TT.DEV
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
GEOMETRIES = [(16, 2), (8, 2), (8, 4), (4, 4), (1, 2)]
# A layer's width is a multiple of 32 (the checkpoint layout; QuantLinear and the C ABI refuse anything else), i.e. of two 16-column strips, so the narrowest
# layer has two strips and the four layers of the selector test are twice 3, 1, 5 and 2 strips wide: layers of 48 or 16 columns cannot be made.
WIDTHS = (96, 32, 160, 64)


def _twice(q, x, t):
    with torch.no_grad():
        y, y2 = q(x, tuning=t), q(x, tuning=t)
    assert torch.equal(y, y2), "the same launch twice gave different bits"
    return y


def _check(q, W, x, hot, t, dtype, what):
    """With the layer's bias (if any): every output; without: every output and the one-hot rows exactly."""
    if q.bias is not None:
        TT._assert_all(_twice(q, x, t), x, W, q.bias, dtype, what + " with bias")
    saved, q._layer.bias = q._layer.bias, None
    try:
        y0 = _twice(q, x, t)
    finally:
        q._layer.bias = saved
    for r, k in hot:
        assert torch.equal(y0[r], W[k]), f"one-hot row {r} (k={k}) is not the oracle's W[k]: {what}"
    TT._assert_all(y0, x, W, None, dtype, what + " without bias")


@DTYPES
@pytest.mark.parametrize("n_layers", [1, 2, 3, 4])
def test_layer_selector(n_layers, dtype):
    K, widths = 256, WIDTHS                                          # strips 6, 2, 10, 4: workgroups 0..21, boundaries at 6, 8 and 18
    made = [TT._layer(K, n, 128, dtype, 1100 + n, bias=(i % 2 == 0)) for i, n in enumerate(widths[:n_layers])]
    layers = [m[1] for m in made]
    for M in (1, 2, 3, 4):
        x, hot = TT._x(M, K, dtype, M)
        for t in (TT._tune(), TT._tune(4, 4), TT._tune(16, 2)):
            with torch.no_grad():
                ys, ys2 = forward_multi(layers, x, t), forward_multi(layers, x, t)
            for i, ((L, q, W), y, y2) in enumerate(zip(made, ys, ys2)):
                assert tuple(y.shape) == (M, widths[i]) and torch.equal(y, y2), f"layer {i} of {n_layers}, M={M}: the same launch twice gave different bits"
                TT._assert_all(y, x, W, q.bias, dtype, f"layer {i} of {n_layers} (N={widths[i]}), M={M}, waves={t.waves}")
                if q.bias is None:
                    for r, k in hot:
                        assert torch.equal(y[r], W[k]), f"one-hot row {r} (k={k}), layer {i} of {n_layers}, M={M}"


@DTYPES
@pytest.mark.parametrize("waves,u", GEOMETRIES)
@pytest.mark.parametrize("K,N,gs,rows", [(256, 32, 128, (1, 2, 4)), (4160, 32, 32, (1, 2, 4)), (8320, 32, 128, (1, 2, 4)), (16640, 32, 128, (1,))],
                         ids=["k256-less-than-a-wave", "k4160-ragged", "k8320-two-pieces", "k16640-loop"])
def test_dma_trip_counts(K, N, gs, rows, waves, u, dtype):
    L, q, W = TT._layer(K, N, gs, dtype, K + waves * 5 + u, bias=True)
    t = TT._tune(waves, u, 1)                                        # no K slices: every workgroup stages the whole K
    d = _lib.describe_plan(q._layer, 1, t)
    assert d["kernel"] == "strips" and int(d["ksplit"]) == 1 and (int(d["waves"]), int(d["u"])) == (waves, u), d
    for M in rows:
        x, hot = TT._x(M, K, dtype, M + u)
        _check(q, W, x, hot, t, dtype, f"waves={waves} u={u} {K}x{N} g{gs} M={M}")


@DTYPES
@pytest.mark.parametrize("ks", [2, 4])
def test_forced_k_slices(ks, dtype):
    from autogptq_amd import qlinear_mi355x as qm
    K, N = 2048, 32
    L, q, W = TT._layer(K, N, 128, dtype, 31 + ks, bias=True)
    t = TT._tune(0, 0, ks)
    assert int(_lib.describe_plan(q._layer, 1, t)["ksplit"]) == ks
    for M in (1, 4):
        x, hot = TT._x(M, K, dtype, M)
        _check(q, W, x, hot, t, dtype, f"ksplit={ks} {K}x{N} M={M}")
    assert not qm.exchange_error(DEV)


@DTYPES
def test_two_strips_per_workgroup(dtype):
    K, N = 1024, 6400                                                # (the planner keeps one strip per workgroup below 96 workgroups)
    L, q, W = TT._layer(K, N, 128, dtype, 42, bias=True)
    t = TT._tune()
    t.reserved[_lib.LAB.OPT] = 2
    for M in (1, 4):
        assert int(_lib.describe_plan(q._layer, M, t)["strips"]) == N // 32
        x, hot = TT._x(M, K, dtype, M)
        _check(q, W, x, hot, t, dtype, f"two strips per workgroup, M={M}")


def test_pair_form():
    from autogptq_amd.fused import fuse_gate_up
    dtype, K, I, gs = torch.float16, 512, 96, 128
    Ls = [O.random_quant_layer(K, I, 4, gs, dtype=dtype, seed=K + I + i, bias=True) for i in range(2)]
    mods = []
    for L in Ls:
        L["scales"] = (L["scales"].float() * 8).to(dtype)            # gate pre-activations of order 1
        m = QuantLinear(4, gs, K, I, True, weight_dtype=dtype)
        m.qweight, m.qzeros, m.scales, m.g_idx, m.bias = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone(), L["bias"].clone()
        mods.append(m)
    fused = fuse_gate_up(*mods).to(DEV)
    q = next(m for m in fused.modules() if isinstance(m, QuantLinear))
    q.post_init()
    mode = O.reference_zero_mode(False, 4)
    Wg, Wu = (O.dequantize(L["qweight"], L["qzeros"], L["scales"], L["g_idx"], 4, mode).to(DEV).double() for L in Ls)
    bg, bu = (L["bias"].to(DEV).double() for L in Ls)
    rtol, atol = 2e-3, 2e-3                                          # test_gpu_tiled.py: one rounding of the product of two sums
    for M in (1, 4):
        x, _ = TT._x(M, K, dtype, M, hot=False)
        ref = torch.nn.functional.silu(x.double() @ Wg + bg) * (x.double() @ Wu + bu)
        for t in (None, TT._tune(16, 2), TT._tune(8, 4)):
            d = _lib.describe_plan(q._layer, M, t)
            assert (d["kernel"], int(d["pair"])) == ("strips", 1), d
            y = _twice(q, x, t)
            bad = (y.double() - ref).abs() > atol * float(ref.abs().max()) + rtol * ref.abs()
            assert not bool(bad.any()), f"pair form M={M} {d}: {int(bad.sum())}/{bad.numel()} outputs out of tolerance"


@DTYPES
def test_act_order(dtype):
    K, N = 512, 64
    L, q, W = TT._layer(K, N, 128, dtype, 77, bias=True, act=True)
    for M in (1, 4):
        x, hot = TT._x(M, K, dtype, M)
        for t in (TT._tune(), TT._tune(16, 2), TT._tune(4, 4)):
            assert _lib.describe_plan(q._layer, M, t)["kernel"] == "strips"
            _check(q, W, x, hot, t, dtype, f"act-order {K}x{N} M={M} waves={t.waves}")


@DTYPES
@pytest.mark.parametrize("bits", [2, 3, 8])
def test_other_packings(bits, dtype):
    K, N = 512, 32
    L, q, W = TT._layer(K, N, 128, dtype, 60 + bits, bias=True, bits=bits)
    for M in (1, 4):
        x, hot = TT._x(M, K, dtype, M)
        for t in (TT._tune(), TT._tune(16, 2), TT._tune(4, 4)):
            assert _lib.describe_plan(q._layer, M, t)["kernel"] == "strips"
            _check(q, W, x, hot, t, dtype, f"int{bits} {K}x{N} M={M} waves={t.waves}")


@DTYPES
def test_six_rows(dtype):
    K, N = 512, 32
    L, q, W = TT._layer(K, N, 128, dtype, 66, bias=True)
    x, hot = TT._x(6, K, dtype, 6)
    for t in (TT._tune(), TT._tune(16, 2), TT._tune(4, 4)):
        assert _lib.describe_plan(q._layer, 6, t)["kernel"] == "strips"
        _check(q, W, x, hot, t, dtype, f"six rows {K}x{N} waves={t.waves}")


def test_captured_graph_replays_to_the_eager_bits():
    K = 256
    made = [TT._layer(K, n, 128, torch.float16, 1300 + n, bias=(n == 32)) for n in WIDTHS]
    layers = [m[1] for m in made]
    La, qa, Wa = TT._layer(512, 64, 128, torch.float16, 78, act=True)
    Lk, qk, Wk = TT._layer(2048, 32, 128, torch.float16, 79, bits=3)
    x, _ = TT._x(2, K, torch.float16, 2)
    xa, _ = TT._x(2, 512, torch.float16, 3)
    xk, _ = TT._x(2, 2048, torch.float16, 4)
    t = TT._tune()

    def run():
        return list(forward_multi(layers, x, t)) + [qa(xa, tuning=t), qk(xk, tuning=t)]
    with torch.no_grad():
        eager = [y.clone() for y in run()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        outs = run()
    for _ in range(3):
        for y in outs:
            y.zero_()
        g.replay()
        torch.cuda.synchronize()
        for i, (y, e) in enumerate(zip(outs, eager)):
            assert torch.equal(y, e), f"output {i} of the replayed graph differs from the eager launch"
    for (L, q, W), y in zip(made, eager[:4]):
        TT._assert_all(y, x, W, q.bias, torch.float16, f"graph, N={q.outfeatures}")
    TT._assert_all(eager[4], xa, Wa, None, torch.float16, "graph, act-order")
    TT._assert_all(eager[5], xk, Wk, None, torch.float16, "graph, 3 bits")
