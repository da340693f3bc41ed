"""GPU (-m gpu): the ALIGNED form of the decode-copy kernel's K loop (gemv_tiled_kernel<..., FL = 2>) against the general form.

The planner takes the aligned form for 4-bit plain layers whose K is a whole number of 128-k chunks, where the form is compiled: one strip per workgroup at one
row, two strips per workgroup (8 waves x 4 chunks) at one and two rows; everything else keeps the general kernel and describe_plan says so (aligned=0).  The lab
switch reserved[GEMM_VARIANT] = VARIANT_TILED_GENERAL keeps the general form, so EVERY case here runs the same layer through both in one process and requires the
same bits (torch.equal) -- the aligned form changes addresses, never the chunk sequence or the order of the sums.  One case per family is also held against
x (fp64) @ W_oracle (fp64) with the helper and tolerance of test_gpu_tiled_stream.py / test_gpu_tiled.py.

Shapes are the smallest at which the addressing can go wrong (a chunk = 128 k): K = 128 (one chunk: all waves but one skip the loop), one pass + one chunk, 11
chunks (a ragged last pass at 2 and at 4 chunks per wave), groups of 32 / 64 / 128 / 256 k and one whole-K group (the group of a chunk: four, two, one, half, none
per chunk), three layers in one launch, the two-strip form, bf16, and K = 160 / 4128 (not whole chunks: aligned=0).  Layer widths are multiples of 32 (the packed
layout's requirement; 48 columns cannot be built): 32 (two strips) and 96 (six)."""
import pytest
import torch

import test_gpu_tiled as TT
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import forward_multi

pytestmark = pytest.mark.gpu
GEOMS = [(16, 2), (8, 2), (4, 4), (8, 4)]


def _general(t):
    g = type(t).from_buffer_copy(t)
    g.reserved[_lib.LAB.GEMM_VARIANT] = _lib.LAB.VARIANT_TILED_GENERAL
    return g


def _expect_aligned(K, M, nstr=1, u=4, bits=4):
    mt = 8 if M >= 5 else (4 if M >= 3 else M)
    return int(bits == 4 and K % 128 == 0 and ((nstr == 1 and mt == 1) or (nstr == 2 and mt <= 2 and u == 4)))


def _both(q, x, t, want, what):
    """The layer through the planner's form (aligned = want) and the forced general form: the same bits.  Returns the output."""
    M = x.shape[0]
    tg = _general(t)
    d, dg = _lib.describe_plan(q._layer, M, t), _lib.describe_plan(q._layer, M, tg)
    assert d["kernel"] == dg["kernel"] == "strips" and int(d["aligned"]) == want and int(dg["aligned"]) == 0, (what, d, dg)
    assert {k: v for k, v in d.items() if k != "aligned"} == {k: v for k, v in dg.items() if k != "aligned"}, (what, d, dg)
    with torch.no_grad():
        y, yg, y2 = q(x, tuning=t), q(x, tuning=tg), q(x, tuning=t)
    assert torch.equal(y, y2), f"{what}: the same launch twice gave different bits"
    assert torch.equal(y, yg), f"{what}: aligned and general forms differ in {int((y != yg).sum())} of {y.numel()} outputs"
    return y


@pytest.mark.parametrize("waves,u", GEOMS)
def test_aligned_equals_general_at_every_pass_shape(waves, u):
    """K = one chunk, one pass + one chunk, 11 chunks; N = 32 and 96; 1 / 2 / 4 rows (2 and 4 rows: the general kernel either way -- the plan says so)."""
    for K in (128, 128 * waves * u + 128, 1408):
        for N in (32, 96):
            L, q, W = TT._layer(K, N, 128, torch.float16, K + N + waves, bias=(N == 96))
            t = TT._tune(waves, u, 1)
            for M in (1, 2, 4):
                x, hot = TT._x(M, K, torch.float16, M + K)
                y = _both(q, x, t, _expect_aligned(K, M), f"{waves}x{u} {K}x{N} M={M}")
                if N == 96:
                    TT._assert_all(y, x, W, q.bias, torch.float16, f"{waves}x{u} {K}x{N} M={M}")


@pytest.mark.parametrize("gs", [32, 64, 128, 256, 1536])
def test_aligned_equals_general_at_every_group_size(gs):
    K = 1536                                                             # 12 chunks: 6 groups of 256
    L, q, W = TT._layer(K, 32, gs, torch.float16, K + gs)
    for waves, u in ((16, 2), (4, 4)):
        x, _ = TT._x(1, K, torch.float16, gs + waves)
        y = _both(q, x, TT._tune(waves, u, 1), 1, f"{waves}x{u} {K}x32 g{gs}")
        TT._assert_all(y, x, W, None, torch.float16, f"{waves}x{u} {K}x32 g{gs}")
    x, hot = TT._x(2, K, torch.float16, gs)                             # one-hot row: the dequantised row exactly (general kernel at 2 rows)
    y = _both(q, x, TT._tune(4, 4, 1), 0, f"4x4 {K}x32 g{gs} M=2")
    for r, k in hot:
        assert torch.equal(y[r], W[k])


@pytest.mark.parametrize("waves,u", [(16, 2), (4, 4)])
def test_aligned_three_layers_in_one_launch(waves, u):
    K = 1408
    made = [TT._layer(K, n, 128, torch.float16, 900 + n) for n in (32, 96, 64)]
    layers = [m[1] for m in made]
    t = TT._tune(waves, u)
    x, _ = TT._x(1, K, torch.float16, waves)
    with torch.no_grad():
        ys, yg = forward_multi(layers, x, t), forward_multi(layers, x, _general(t))
    for (L, q, W), y, g in zip(made, ys, yg):
        assert int(_lib.describe_plan(q._layer, 1, t)["aligned"]) == 1
        assert torch.equal(y, g), f"three layers, N={q.outfeatures}: aligned and general forms differ"
        TT._assert_all(y, x, W, None, torch.float16, f"three layers N={q.outfeatures} {waves}x{u}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_aligned_two_strips_per_workgroup(dtype):
    K, N = 256, 3072
    L, q, W = TT._layer(K, N, 128, dtype, 78, bias=True)
    for waves in (8, 4):
        t = TT._tune(waves, 4)
        t.reserved[_lib.LAB.OPT] = 2
        for M in (1, 2):
            x, _ = TT._x(M, K, dtype, M + waves)
            assert int(_lib.describe_plan(q._layer, M, t)["strips"]) == N // 32
            y = _both(q, x, t, 1, f"two strips {waves}x4 {K}x{N} M={M}")
            TT._assert_all(y, x, W, q.bias, dtype, f"two strips {waves}x4 {K}x{N} M={M}")


@pytest.mark.parametrize("M", [1, 4])
def test_aligned_bf16(M):
    for K, (waves, u) in ((1408, (16, 2)), (128 * 16 + 128, (4, 4))):
        L, q, W = TT._layer(K, 96, 128, torch.bfloat16, K + M, bias=True)
        x, _ = TT._x(M, K, torch.bfloat16, M)
        y = _both(q, x, TT._tune(waves, u, 1), _expect_aligned(K, M), f"bf16 {waves}x{u} {K}x96 M={M}")
        TT._assert_all(y, x, W, q.bias, torch.bfloat16, f"bf16 {waves}x{u} {K}x96 M={M}")


@pytest.mark.parametrize("K,gs", [(160, 32), (4128, 32)])
def test_k_that_is_no_whole_number_of_chunks_keeps_the_general_form(K, gs):
    L, q, W = TT._layer(K, 32, gs, torch.float16, K)
    for waves, u in ((16, 2), (4, 4)):
        x, _ = TT._x(1, K, torch.float16, K)
        y = _both(q, x, TT._tune(waves, u, 1), 0, f"{waves}x{u} {K}x32 g{gs}")
        TT._assert_all(y, x, W, None, torch.float16, f"{waves}x{u} {K}x32 g{gs}")


def test_aligned_form_inside_guard_bands():
    """x, the output and the workspace inside guard bands (the helper of test_gpu_memory_contract.py): one pass + one chunk at both depths."""
    import test_gpu_memory_contract as MC
    K = 128 * 32 + 128
    q = MC._make(K, 96, 4, 128, False, torch.float16, K)
    for t in (TT._tune(16, 2, 1), TT._tune(4, 4, 1)):
        assert int(_lib.describe_plan(q._layer, 1, t)["aligned"]) == 1
        assert MC._dense_case(q, 1, t, "aligned form")[0] == "strips"
