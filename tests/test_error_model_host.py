"""CPU: the sensitivity of the error-model assertion itself (tests/_error_model.py), with no GPU.  An EMULATED correct kernel -- fp32 sums per group, the
group's scale applied to the fp32 sum, the bias added in fp32, one rounding to the layer dtype -- must lie inside the bound on every output in every value
regime, and each emulated defect must be flagged on at least one output.  The count of outputs that the older per-tensor rule (1e-3 max|y| sqrt(K / 1024) +
1e-3 |y|; 8e-3 for bf16, 1e-4 for fp32: test_gpu_parity.py / test_gpu_fuzz.py) flags for the same defect is printed beside it, not asserted.

Two things this file shows about the model rather than about a kernel:
  * bf16.  The GPU tests take A on the biased weights, |s| (2 (2^bits - 1) + 128), because the bf16 decode forms carry 128 + w.  The emulated kernel forms
    w - z exactly and carries no such bias, so the assertions here use A = |x| @ |W64| (stricter for the correct kernel); the count under the biased A is
    printed beside each.  Under the biased A, at 1056 x 96 and 4 rows, 'W rounded per weight' (uniform, narrow: worst err / bound 0.84), 'last k dropped'
    (outlier, narrow: 0.90; runs, narrow: 0.80) and 'previous zero-point' (outlier, narrow: 0.94) stay below the bound: there it is about 1.3 bf16 ulp wide.
  * fp32.  With C = 16 on every fp32 layer, x silently rounded to fp16 was NOT flagged at 1056 x 96 with uniform x and the oracle's scales: worst err / bound
    0.73 (0.68 - 0.79 over six draws of x), 0 of 384 outputs.  The sum term models the fp32 accumulation, which is the same whatever dtype the store has (the
    decode kernels are one template over the layer dtype: _error_model.constant_for), so an fp32 layer on a decode family now has that family's C = 4 -- the
    stricter value -- and the defect is flagged on 151 of 384 outputs (worst err / bound 2.94).  The emulated correct fp32 kernel uses 0.004 - 0.07 of the
    bound.  16 stays the constant of the fp32 matrix-core GEMM alone (one unbroken chain over K: test_gpu_grad_input.py).
'W rounded per weight' is also the documented arithmetic of the matrix-core GEMMs: with its K roundings as explicit ulp terms (extra_roundings) it passes."""
import numpy as np
import pytest
import torch

import _error_model as EM
from autogptq_amd import _lib
from oracle import gptq_oracle as O

SHAPES = [(1056, 96, 4, 96, 4), (256, 64, 8, 32, 4)]                              # K, N, bits, group size, M
OLD_TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3, torch.float32: 1e-4}
DEV = "cpu"
# 'last k dropped' is visible only where x[:, K - 1] is: a draw whose last run is all zeros in the four rows, or whose last term is below half an ulp of every
# bf16 output it feeds, changes nothing that any assertion could see (4 of 6 draws tried had such a case).  The draw is fixed to one where every listed case has data to show.
X_SEED = 4


def _parts(K, N, bits, gs, M, dtype, regime):
    xr, sr = regime
    L = EM.make_layer(K, N, bits, gs, dtype, False, sr, seed=K + N + bits)
    w = torch.from_numpy(O.unpack_weights(L["qweight"], bits).astype(np.int32))
    z = torch.from_numpy(O.unpack_zeros(L["qzeros"], bits, O.ZERO_WRAP))
    x = EM.make_x(xr, M, K, dtype, seed=K + M + X_SEED).to(dtype)
    W64 = EM.w64(L, bits, O.ZERO_WRAP, DEV)
    b64 = L["bias"].double()
    y64 = x.double() @ W64 + b64
    A = x.double().abs() @ W64.abs()                                   # the emulated kernel's own arithmetic: w - z formed as an exact integer
    Ab = x.double().abs() @ EM.abs_weights(L, bits, dtype, W64)       # what the GPU tests use: bf16 on the biased weights (the same A otherwise)
    return L, w, z, x, y64, A, Ab


def _emulate(L, w, z, x, dtype, gs, defect=None):
    """y of the emulated kernel, in the layer dtype."""
    K, N = w.shape
    G = K // gs
    s = L["scales"].float()                                                       # [G, N]
    xf = x.float()
    if defect == "x_to_fp16":
        xf = xf.half().float()
    if defect == "last_k":
        xf = xf.clone()
        xf[:, K - 1] = 0
    if defect == "w_rounded":                                                     # scales * (w - z) rounded to the layer dtype per weight, then one fp32 sum over K
        Wr = (L["scales"].float().repeat_interleave(gs, 0) * (w - z.repeat_interleave(gs, 0)).float()).to(dtype).float()
        return (xf @ Wr + L["bias"].float()).to(dtype)
    zk = z.repeat_interleave(gs, 0).clone()                                       # [K, N]: the zero-point that k is decoded with
    first = torch.arange(gs, K, gs)                                               # the first k of every group but the first
    if defect == "prev_zero":
        zk[first] = z[:-1]
    D = (w - zk).float().reshape(G, gs, N)                                        # exact small integers
    S = torch.einsum("mgk,gkn->mgn", xf.reshape(-1, G, gs), D)                    # fp32 sums per group
    y = (S * s[None]).sum(1)
    if defect == "prev_scale":                                                    # the first k of each group meets the scale of the group before
        y = y + torch.einsum("mg,gn->mn", xf[:, first], D[1:, 0, :] * (s[:-1] - s[1:]))
    return (y + L["bias"].float()).to(dtype)


def _flags(y, y64, A, K, dtype):
    C = EM.constant_for("strips", dtype, 0)                                       # the emulation sums per group like the decode kernels: C = 4, fp32 layers too
    err = (y.double() - y64).abs()
    b = EM.bound(y64, A, K, dtype, C)
    old = OLD_TOL[dtype] * float(y64.abs().max().clamp_min(1.0)) * max(1.0, (K / 1024) ** 0.5) + OLD_TOL[dtype] * y64.abs()
    return int((err > b).sum()), float((err / b).max()), int((err > old).sum())


def _defects(dtype, regime):
    """(defect, asserted?) for this dtype and regime."""
    xr, sr = regime
    out = [("last_k", True), ("prev_zero", True),
           # +-10 % scales under an outlier: the defect moves an output by 0.1 s x (w - z) of ONE small term, legitimately below the bound of a row that an outlier scales
           ("prev_scale", regime == ("uniform", "narrow") or sr == "wide")]
    if dtype != torch.float32:
        out.append(("w_rounded", True))
    else:
        out.append(("x_to_fp16", xr in ("uniform", "runs")))
    return out


@pytest.mark.parametrize("regime", EM.REGIMES, ids=["-".join(r) for r in EM.REGIMES])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("K,N,bits,gs,M", SHAPES, ids=["1056x96-int4-g96", "256x64-int8-g32"])
def test_the_bound_passes_a_correct_kernel_and_flags_each_defect(K, N, bits, gs, M, dtype, regime):
    L, w, z, x, y64, A, Ab = _parts(K, N, bits, gs, M, dtype, regime)
    assert bool(torch.isfinite(y64).all()) and float(Ab.max()) < torch.finfo(dtype).max / 4
    n, worst, old = _flags(_emulate(L, w, z, x, dtype, gs), y64, A, K, dtype)
    print(f"\n{K}x{N} int{bits} g{gs} {EM.NAMES[dtype]} {regime}: correct kernel worst err / bound {worst:.3f} (old rule flags {old})")
    assert n == 0 and worst < 1.0, (n, worst)
    for defect, asserted in _defects(dtype, regime):
        yd = _emulate(L, w, z, x, dtype, gs, defect)
        n, worst, old = _flags(yd, y64, A, K, dtype)
        biased = f", on the biased weights {_flags(yd, y64, Ab, K, dtype)[0]:3d}" if dtype == torch.bfloat16 else ""
        print(f"  {defect:10s}: model flags {n:3d} / {y64.numel()} (worst err / bound {worst:8.2f}){biased}, old rule flags {old:3d}{'' if asserted else '   [not asserted]'}")
        if asserted:
            assert n >= 1, (defect, worst)
        if defect == "w_rounded":      # ... which is the documented arithmetic of the matrix-core GEMMs: with its K roundings as explicit ulp terms it passes
            err = (yd.double() - y64).abs()
            full = EM.bound(y64, A, K, dtype, EM.constant_for("strips", dtype, 0), ((x.double(), EM.w64(L, bits, O.ZERO_WRAP, DEV)),))
            print(f"              with extra_roundings=((x, W64),): worst err / bound {float((err / full).max()):.3f}")
            assert bool((err <= full).all())


def test_helper_pieces():
    """ulp at the binade edges and the subnormal floor; the constants are the project's existing ones."""
    v = torch.tensor([1.0, 1.999, 2.0, 2.0 ** -14, 2.0 ** -20, 0.0], dtype=torch.float64)
    assert EM.ulp(v, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24]
    assert EM.ulp(v[:3], torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    assert EM.ulp(v[:3], torch.float32).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22]
    for k in EM.DECODE_KERNELS:
        assert EM.constant_for(k, torch.float16, 128) == 4.0 and EM.constant_for({"kernel": k}, torch.bfloat16, -1) == 4.0
    assert EM.constant_for("rows", torch.float16, 128) == 8.0 and EM.constant_for("panel", torch.bfloat16, 1024) == 16.0
    assert EM.constant_for("wide_sk", torch.float16, -1) == 16.0 and EM.constant_for("strips", torch.float32, 32) == 4.0 and EM.constant_for("f32_mfma", torch.float32, 32) == 16.0
    y64 = torch.tensor([1.0], dtype=torch.float64)
    A = torch.tensor([2.0], dtype=torch.float64)
    b0 = EM.bound(y64, A, 1024, torch.float16, 4.0)
    assert float(b0) == (0.5 + 1 / 64) * 2.0 ** -10 + 4 * 32 * 2.0 ** -24 * 2
    pre = 4 * 32 * 2.0 ** -24 * 2 + (0.5 + 1 / 64) * 2.0 ** -8
    assert float(EM.bound(y64, A, 1024, torch.float16, 4.0, extra_roundings=(y64 * 4,))) == (0.5 + 1 / 64) * 2.0 ** -10 + pre
    # K roundings carried by |coef|; a zero value has none; the store's ulp is taken at |y64| + pre (2 - 2^-10 + pre is past 2: spacing 2^-9)
    coef, vals = torch.tensor([[2.0, -3.0, 5.0]], dtype=torch.float64), torch.tensor([[1.0], [0.0], [0.25]], dtype=torch.float64)
    pre = 4 * 32 * 2.0 ** -24 * 2 + (0.5 + 1 / 64) * (2 * 2.0 ** -10 + 5 * 2.0 ** -12)
    assert float(EM.bound(2 - y64 * 2.0 ** -10, A, 1024, torch.float16, 4.0, extra_roundings=((coef, vals),))) == (0.5 + 1 / 64) * 2.0 ** -9 + pre
    assert EM.rounds_each_weight({"path": "gemm", "kernel": "rows"}, torch.float16) and not EM.rounds_each_weight({"path": "gemv", "kernel": "strips"}, torch.bfloat16)
    assert not EM.rounds_each_weight({"path": "gemm", "kernel": "f32_mfma"}, torch.float32)
    x = EM.make_x("runs", 8, 96, torch.float16, 3)
    runs = x.reshape(8, 3, 32)
    assert bool(((runs == 0).all(-1) | (runs != 0).any(-1)).all()) and bool((runs == 0).all(-1).any())
    xo = EM.make_x("outlier", 5, 96, torch.float16, 3)
    assert (xo.abs() == 48).sum(1).tolist() == [4] * 5 and float(xo.abs().median()) < 2.0 ** -6


def test_the_edge_tables_plan_onto_the_frozen_kernel_families():
    """Host only (gptq_describe_plan never touches the device): the default plans of every (layer, M) of test_gpu_error_model_edges.py's table land on exactly
    the families frozen there -- what its closing test asserts of the GPU run -- and the planner refuses none of them."""
    import test_gpu_error_model_edges as E
    seen = E.planned_families()
    assert set(seen) == E.FAMILIES, (sorted(seen), sorted(E.FAMILIES))
    assert {"strips", "generic", "rows"} <= set(seen) and set(seen) - set(EM.DECODE_KERNELS) - {"rows"}
    assert len(E.EDGE_CASES) == 75 and len(E.REGIME_CASES) == 41
    # 2c: the fused sites of the gated shapes -- the pair form at 1..4 rows with the decode copy, the fused GEMV epilogue without it on `tiny` alone
    import test_gpu_gated_act as GA
    for shape, want in E.FUSED_GEMV_ROWS.items():
        K, I, gs, bits = GA.PAIR_SHAPES[GA.PAIR_IDS.index(shape)]
        for dtype in (torch.float16, torch.bfloat16):
            for copy, rows in ((True, [1, 2, 3, 4]), (False, want)):
                L = E.host_layer(K, 2 * I, bits, gs, dtype, False, copy, "nowrap" if bits == 3 else "wrap", "silu_mul")
                assert [M for M in E.GATED_ROWS if _lib.describe_plan(L, M)["epilogue"] == "fused"] == rows, (shape, dtype, copy)
