"""GPU (-m gpu): TWO-STEP staging of the decode-copy kernel against the one-step form.

A plain 4-bit fp16 launch without K slices whose K is deeper than one pass of its workgroup (waves x u chunks of 128 k) stages only that pass's part of x and of
the constants in front of its first weight burst; the rest follows behind the staging barrier and is in the LDS by a second barrier in front of the second pass
(describe_plan: xstage=2).  reserved[GEMM_VARIANT] = VARIANT_TILED_ONE_STEP keeps one step, so EVERY case here runs the same layer through both plans in one
process and requires the same bits (torch.equal): the second step changes when bytes reach the LDS, never where they lie, the chunk sequence or the order of the
sums.  One case is also held to the per-output error model (tests/_error_model.py) against x (fp64) @ W (fp64), the others to the tolerance of test_gpu_tiled.py.

Shapes: the geometry is forced to 4 waves x 2 chunks (one pass = 1024 k) so that the K values where the second step can go wrong are small --
  1024  exactly one pass: one step;
  1152  one chunk in step 2: three of four waves have no later chunk and must still reach the second barrier;
  2048  two whole passes;  2688  a ragged third pass of whole chunks (aligned form);
  2752, 2112  not whole chunks (general form): a ragged k-slot at the end of step 2;
-- at 1 .. 4 rows (4 rows of x: the row stride of step 2's destinations), groups of 32 / 128 / whole K (the last: every record belongs to step 1), bias, three
layers in one launch (the layer selector next to the new word), and the real 16-wave x 2-chunk form once at K = 4224 and K = 11008.  Act-order, bf16, 3- / 8-bit and
K-sliced launches stay one-step: plan assertions."""
import pytest
import torch

import _error_model as EM
import test_gpu_tiled as TT
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import forward_multi
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
PASS = 1024                                                              # k of one pass of 4 waves x 2 chunks


def _one_step(t):
    g = type(t).from_buffer_copy(t)
    g.reserved[_lib.LAB.GEMM_VARIANT] = _lib.LAB.VARIANT_TILED_ONE_STEP
    return g


def _both(q, x, t, want, what):
    """The layer through the planner's staging (xstage = want) and the forced one-step plan: the same bits.  Returns the output."""
    M = x.shape[0]
    t1 = _one_step(t)
    d, d1 = _lib.describe_plan(q._layer, M, t), _lib.describe_plan(q._layer, M, t1)
    assert d["kernel"] == d1["kernel"] == "strips" and int(d["xstage"]) == want and int(d1["xstage"]) == 1, (what, d, d1)
    assert {k: v for k, v in d.items() if k != "xstage"} == {k: v for k, v in d1.items() if k != "xstage"}, (what, d, d1)
    with torch.no_grad():
        y, y1, y2 = q(x, tuning=t), q(x, tuning=t1), q(x, tuning=t)
    assert torch.equal(y, y2), f"{what}: the same launch twice gave different bits"
    assert torch.equal(y, y1), f"{what}: two-step and one-step staging differ in {int((y != y1).sum())} of {y.numel()} outputs"
    return y


@pytest.mark.parametrize("K,gs", [(1024, 128), (1152, 128), (2048, 128), (2688, 128), (2752, 64), (2112, 32)])
def test_two_steps_equal_one_step_at_every_pass_shape(K, gs):
    t = TT._tune(4, 2, 1)
    for N in (32, 96):
        L, q, W = TT._layer(K, N, gs, torch.float16, K + N, bias=(N == 96))
        for M in (1, 2, 3, 4):
            x, hot = TT._x(M, K, torch.float16, M + K)
            y = _both(q, x, t, 2 if K > PASS else 1, f"4x2 {K}x{N} g{gs} M={M}")
            TT._assert_all(y, x, W, q.bias, torch.float16, f"4x2 {K}x{N} g{gs} M={M}")
            if q.bias is None:
                for r, k in hot:                                         # a one-hot row returns the dequantised row, from either step's part of x (k = K - 1, 0, 129)
                    assert torch.equal(y[r], W[k]), (K, N, M, r, k)


@pytest.mark.parametrize("gs", [32, 128, 2048])
def test_two_steps_at_every_group_size(gs):
    K = 2048                                                             # groups of 32 / 128: 32 / 8 records in each step; one group: all of it in step 1
    L, q, W = TT._layer(K, 32, gs, torch.float16, K + gs, bias=True)
    for waves, u in ((4, 2), (4, 4), (8, 2)):
        for M in (1, 4, 6):                                              # (6 rows: the second A operand's rows come from step 2 as well)
            x, _ = TT._x(M, K, torch.float16, gs + waves + M)
            y = _both(q, x, TT._tune(waves, u, 1), 2 if K > waves * u * 128 else 1, f"{waves}x{u} {K}x32 g{gs} M={M}")
            TT._assert_all(y, x, W, q.bias, torch.float16, f"{waves}x{u} {K}x32 g{gs} M={M}")


@pytest.mark.parametrize("K", [4224, 11008])
def test_the_sixteen_wave_form(K):
    """16 waves x 2 chunks (o, down): one pass = 4096 k; K = 4224: one chunk in step 2; K = 11008: the down projection's three passes, the last with 11 live waves."""
    L, q, W = TT._layer(K, 32, 128, torch.float16, K, bias=True)
    t = TT._tune(16, 2, 1)
    for M in (1, 4):
        x, _ = TT._x(M, K, torch.float16, K + M)
        y = _both(q, x, t, 2, f"16x2 {K}x32 M={M}")
        TT._assert_all(y, x, W, q.bias, torch.float16, f"16x2 {K}x32 M={M}")


def test_two_steps_within_the_error_model():
    """x (fp64) @ W (fp64) + bias under the per-output bound of tests/_error_model.py (C of the decode kernels), 1 and 4 rows, uniform and outlier activations."""
    K, N, gs = 2752, 96, 64
    L = EM.make_layer(K, N, 4, gs, torch.float16, False, "narrow", seed=K + N)
    q = TT.QuantLinear(4, gs, K, N, True, weight_dtype=torch.float16)
    q.qweight, q.qzeros, q.scales, q.g_idx, q.bias = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone(), L["bias"].clone()
    q = q.to(TT.DEV)
    q.post_init()
    W64 = EM.w64(L, 4, O.ZERO_WRAP, TT.DEV)
    b64 = L["bias"].to(TT.DEV).double()
    t = TT._tune(4, 2, 1)
    for regime in ("uniform", "outlier"):
        for M in (1, 4):
            x = EM.make_x(regime, M, K, torch.float16, K * 7 + M).to(torch.float16).to(TT.DEV)
            y = _both(q, x, t, 2, f"error model {regime} M={M}")
            x64 = x.double()
            y64, A = x64 @ W64 + b64, x64.abs() @ W64.abs()
            plan = _lib.describe_plan(q._layer, M, t)
            bnd = EM.bound(y64, A, K, torch.float16, EM.constant_for(plan, torch.float16, gs))
            err = (y.double() - y64).abs()
            print(f"two-step error model {regime} M={M}: worst err / bound = {float((err / bnd).max()):.3f}")
            assert not bool((err > bnd).any()), (regime, M, float((err / bnd).max()))


@pytest.mark.parametrize("waves,u", [(4, 2), (16, 2)])
def test_two_steps_three_layers_in_one_launch(waves, u):
    K = waves * u * 128 + 384
    made = [TT._layer(K, n, 128, torch.float16, 700 + n, bias=(n == 96)) for n in (32, 96, 64)]
    layers = [m[1] for m in made]
    t = TT._tune(waves, u)
    for M in (1, 3):
        x, _ = TT._x(M, K, torch.float16, waves + M)
        with torch.no_grad():
            ys, y1 = forward_multi(layers, x, t), forward_multi(layers, x, _one_step(t))
        for (L, q, W), y, g in zip(made, ys, y1):
            assert torch.equal(y, g), f"three layers, N={q.outfeatures} M={M}: two-step and one-step staging differ"
            TT._assert_all(y, x, W, q.bias, torch.float16, f"three layers N={q.outfeatures} {waves}x{u} M={M}")
    tk = TT._tune(waves, u, 1)
    assert int(_lib.describe_plan(layers[0]._layer, 1, tk)["xstage"]) == 2


def test_the_other_forms_stay_one_step():
    K = 2048
    for what, kw, dtype in (("act-order", dict(act=True), torch.float16), ("bf16", {}, torch.bfloat16), ("3-bit", dict(bits=3), torch.float16), ("8-bit", dict(bits=8), torch.float16)):
        L, q, W = TT._layer(K, 32, 128, dtype, 31, **kw)
        for M in (1, 4):
            d = _lib.describe_plan(q._layer, M, TT._tune(4, 2, 1))
            assert d["kernel"] == "strips" and int(d["xstage"]) == 1, (what, M, d)
    L, q, W = TT._layer(K, 32, 128, torch.float16, 32)
    d = _lib.describe_plan(q._layer, 1, TT._tune(4, 2, 2))
    assert d["kernel"] == "strips" and int(d["ksplit"]) == 2 and int(d["xstage"]) == 1, d
    x, _ = TT._x(1, K, torch.float16, 5)
    with torch.no_grad():
        y = q(x, tuning=TT._tune(4, 2, 2))                               # K slices of a layer that would take two steps unsplit: each slice is one pass here
    TT._assert_all(y, x, W, None, torch.float16, "two K slices")


def test_two_steps_inside_guard_bands():
    """x, the output and the workspace inside guard bands (the helper of test_gpu_memory_contract.py): one pass + one chunk at both workgroup sizes."""
    import test_gpu_memory_contract as MC
    for waves, u in ((4, 2), (16, 2)):
        K = waves * u * 128 + 128
        q = MC._make(K, 96, 4, 128, False, torch.float16, K)
        t = TT._tune(waves, u, 1)
        assert int(_lib.describe_plan(q._layer, 1, t)["xstage"]) == 2
        for M in (1, 4):
            assert MC._dense_case(q, M, t, "two-step staging")[0] == "strips"
