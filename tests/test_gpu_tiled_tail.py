"""GPU (-m gpu): the tail of the decode-copy kernel (gemv_tiled_kernel, csrc/gemv_tiled_kernel.cuh) behind its K loop.

A launch without K slices ends in straight-line code: the k-slots of a column meet through two register swaps, the waves of the workgroup through one LDS
round trip whose wave count is a compile-time constant of the arm taken (4 / 8 / 16 waves in the single-strip form, 2 / 4 / 8 waves per strip in the
two- / four-strip and [gate | up] pair forms), the bias was requested in the first pass of the K loop.  Launches WITH K slices, and wave counts outside that
list, take the cold block (granules, epochs, the run-time loops).  The existing tiled tests reach these arms mostly through the default plan; here every arm
is forced (tuning.path = 8, waves, reserved[DEPTH], reserved[OPT]) -- 1..4 rows, fp16 / bf16, with and without bias, whole and ragged K, one and three
layers per launch -- and EVERY output is held against x (fp64) @ W_oracle (fp64) with the tolerance helper of test_gpu_tiled.py; one-hot rows must return
the oracle's dequantised rows exactly, and the same launch twice must return the same bits."""
import pytest
import torch

import test_gpu_tiled as TT
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear, forward_multi
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = TT.DEV
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
# (waves, chunks in flight): the straight-line arms (4 / 8 / 16 waves; 16 x 4 is not compiled for single-strip workgroups) ...
LEAN = [(4, 2), (4, 4), (8, 2), (8, 4), (16, 2)]
# ... and wave counts that keep the run-time loops behind the same K loop
GENERIC = [(2, 4), (3, 4), (1, 2)]


def _twice(q, x, t):
    with torch.no_grad():
        y, y2 = q(x, tuning=t), q(x, tuning=t)
    assert torch.equal(y, y2), "the same launch twice gave different bits"
    return y


@DTYPES
@pytest.mark.parametrize("waves,u", LEAN + GENERIC)
@pytest.mark.parametrize("K,N,gs", [(2048, 256, 128), (4160, 96, 32), (1056, 64, 1056)], ids=["whole-k", "ragged-k", "ragged-k-one-group"])
def test_unsplit_tail_single_strip(K, N, gs, waves, u, dtype):
    L, q, W = TT._layer(K, N, gs, dtype, K + N + waves * 7 + u, bias=True)
    t = TT._tune(waves, u)
    d = _lib.describe_plan(q._layer, 1, t)
    assert d["kernel"] == "strips" and int(d["ksplit"]) == 1 and (int(d["waves"]), int(d["u"])) == (waves, u), d
    for M in (1, 2, 3, 4):
        x, hot = TT._x(M, K, dtype, M + u)
        y = _twice(q, x, t)
        TT._assert_all(y, x, W, q.bias, dtype, f"waves={waves} u={u} {K}x{N} g{gs} M={M} with bias")
        saved, q._layer.bias = q._layer.bias, None
        try:
            y0 = _twice(q, x, t)
        finally:
            q._layer.bias = saved
        for r, k in hot:
            assert torch.equal(y0[r], W[k]), f"one-hot row {r} (k={k}) is not the oracle's W[k]: waves={waves} u={u} {K}x{N} M={M}"
        TT._assert_all(y0, x, W, None, dtype, f"waves={waves} u={u} {K}x{N} g{gs} M={M} without bias")


@DTYPES
@pytest.mark.parametrize("waves,u", [(4, 4), (8, 2), (8, 4), (16, 2)])
def test_unsplit_tail_three_layers_in_one_launch(waves, u, dtype):
    """The layer's output pointer, bias pointer and width are per WORKGROUP (the layer selector at kernel entry): three widths."""
    K = 2048
    made = [TT._layer(K, n, 128, dtype, 900 + n, bias=(n != 288)) for n in (512, 288, 64)]
    layers = [m[1] for m in made]
    for M in (1, 2, 3, 4):
        x, hot = TT._x(M, K, dtype, M)
        for t in (None, TT._tune(waves, u)):
            with torch.no_grad():
                ys, ys2 = forward_multi(layers, x, t), forward_multi(layers, x, t)
            for (L, q, W), y, y2 in zip(made, ys, ys2):
                assert torch.equal(y, y2)
                TT._assert_all(y, x, W, q.bias, dtype, f"three layers, N={q.outfeatures} M={M} waves={waves} u={u}")
                if q.bias is None:
                    for r, k in hot:
                        assert torch.equal(y[r], W[k])


@DTYPES
@pytest.mark.parametrize("nstr,waves,u", [(2, 0, 0), (2, 8, 4), (2, 4, 4), (2, 16, 2), (4, 0, 0), (4, 16, 2), (4, 8, 2)])
def test_unsplit_tail_several_strips_per_workgroup(nstr, waves, u, dtype):
    """Two / four strips per workgroup: the waves of a strip are summed in ascending order; 2, 4 or 8 waves per strip are straight-line arms.  A geometry
    the planner refuses for a row count (its compilation does not exist) is not launched -- the planner's own (waves = 0) always is."""
    LAB = _lib.LAB
    K, N = 1024, 6400                                                # (the planner keeps one strip per workgroup below 96 workgroups)
    L, q, W = TT._layer(K, N, 128, dtype, 40 + nstr, bias=True)
    ran = 0
    for M in (1, 2, 3, 4):
        if nstr == 4 and M < 3:                                      # the four-strip form exists from 3 rows
            continue
        x, hot = TT._x(M, K, dtype, M)
        t = TT._tune(waves, u)
        t.reserved[LAB.OPT] = nstr
        try:
            d = _lib.describe_plan(q._layer, M, t)
        except _lib.GptqError:
            d = {}
        if d.get("kernel") != "strips":                              # a forced geometry without a compilation at this row count
            assert waves != 0, "the planner refused its own geometry"
            continue
        assert int(d["strips"]) == N // 16 // nstr, d
        y = _twice(q, x, t)
        TT._assert_all(y, x, W, q.bias, dtype, f"{nstr} strips per workgroup, waves={waves} u={u} M={M}")
        saved, q._layer.bias = q._layer.bias, None
        try:
            y0 = _twice(q, x, t)
        finally:
            q._layer.bias = saved
        for r, k in hot:
            assert torch.equal(y0[r], W[k])
        ran += 1
    assert ran or waves != 0


@DTYPES
def test_unsplit_tail_pair_form(dtype):
    """[gate | up] with the SiLU * mul epilogue: gate and up strips summed over the two halves of the waves (2 / 4 / 8 waves per half), two bias words per output."""
    from autogptq_amd.fused import fuse_gate_up
    K, I, gs = 2112, 352, 64                                         # ragged K
    for bias in (True, False):
        Ls = [O.random_quant_layer(K, I, 4, gs, dtype=dtype, seed=K + I + i, bias=bias) for i in range(2)]
        mods = []
        for L in Ls:
            L["scales"] = (L["scales"].float() * 4).to(dtype)        # gate pre-activations of order 1
            m = QuantLinear(4, gs, K, I, bias, weight_dtype=dtype)
            m.qweight, m.qzeros, m.scales, m.g_idx = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone()
            if bias:
                m.bias = L["bias"].clone()
            mods.append(m)
        fused = fuse_gate_up(*mods).to(DEV)
        q = next(m for m in fused.modules() if isinstance(m, QuantLinear))
        q.post_init()
        mode = O.reference_zero_mode(False, 4)
        Wg, Wu = (O.dequantize(L["qweight"], L["qzeros"], L["scales"], L["g_idx"], 4, mode).to(DEV).double() for L in Ls)
        bg, bu = ((L["bias"].to(DEV).double() if bias else 0.0) for L in Ls)
        rtol, atol = {torch.float16: (2e-3, 2e-3), torch.bfloat16: (1.6e-2, 1.6e-2)}[dtype]      # test_gpu_tiled.py: one rounding of the product of two sums
        for M in (1, 2, 3, 4):
            x, _ = TT._x(M, K, dtype, M, hot=False)
            ref = torch.nn.functional.silu(x.double() @ Wg + bg) * (x.double() @ Wu + bu)
            for t in (None, TT._tune(16, 2), TT._tune(8, 4), TT._tune(8, 2), TT._tune(4, 4), TT._tune(2, 2)):
                d = _lib.describe_plan(q._layer, M, t)
                assert (d["kernel"], int(d["pair"])) == ("strips", 1), d
                y = _twice(q, x, t)
                bad = (y.double() - ref).abs() > atol * float(ref.abs().max()) + rtol * ref.abs()
                assert not bool(bad.any()), f"pair form bias={bias} M={M} {d}: {int(bad.sum())}/{bad.numel()} outputs out of tolerance"


def test_k_slices_still_take_the_cold_block():
    """K slices are no longer on the hot path: the planner's own four slices of a 28672-deep shard, forced slices at every straight-line wave count, the
    sticky error word clean and the strip epochs moving (a second launch on the same workspace combines under a new tag and gives the same bits)."""
    from autogptq_amd import qlinear_mi355x as qm
    L, q, W = TT._layer(28672, 1024, 128, torch.float16, 78)
    assert int(_lib.describe_plan(q._layer, 1)["ksplit"]) == 4
    x, _ = TT._x(1, 28672, torch.float16, 4)
    with torch.no_grad():
        y, y2 = q(x), q(x)
    assert torch.equal(y, y2)
    TT._assert_all(y, x, W, None, torch.float16, "28672x1024, the planner's four K slices")
    assert not qm.exchange_error(DEV)
    for dtype in (torch.float16, torch.bfloat16):
        L, q, W = TT._layer(8192, 256, 128, dtype, 5, bias=True)
        for M in (1, 3):
            x, hot = TT._x(M, 8192, dtype, M)
            for waves, u, ks in ((16, 2, 2), (8, 4, 4), (4, 4, 3), (2, 4, 2)):
                y = _twice(q, x, TT._tune(waves, u, ks))
                TT._assert_all(y, x, W, q.bias, dtype, f"K slices: waves={waves} u={u} ksplit={ks} M={M}")
    assert not qm.exchange_error(DEV)
