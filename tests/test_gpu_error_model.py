"""GPU: a per-output error MODEL instead of a per-tensor tolerance (review item, round 5: `1e-3 max|y| + 1e-3 |y|` is ~2 fp16 ulps at the largest output
and loose for the small ones).  What the kernels of the default plans compute is known exactly -- w - z as exact integers in the layer dtype, products with x
exact in fp32, fp32 sums per group, the group's scale applied to the fp32 sum, ONE rounding to the layer dtype at the store -- so against the fp64 value of the
same expression (oracle unpack, scales[g] * (w - z[g]) in fp64: oracle.forward_f64's dequant) every output obeys

    |y - y64|  <=  (1/2 + 1/64) ulp_dtype(y64)  +  C * sqrt(K) * 2^-24 * A,        A = |x| @ |W64|   (the condition of that output's sum)

C, measured (profiles/r06_error_model_report.log: worst err / bound per kernel family at C = 4): the decode kernels (1..4 rows: 4x4x4 matrix-core steps into
per-group fp32 sums, then shuffles / LDS in a fixed order) stay below 0.8 at C = 4; the matrix-core GEMMs (rows / panel / stream-K: 16x16x32 and 32x32x16
steps chained over a whole group, or over the whole K of a group_size = -1 layer) reach 1.0 - 1.6 with groups of at most 128 and 2.7 with one group -- the
matrix core's accumulation of a long chain errs more than a tree of fp32 adds of the same terms -- so C = 8 for them, 16 for whole-K groups.  bf16 layers:
the decode forms carry the zero-point on the matrix core or as a run sum (raw biased pairs 128 + w, then -(128 + z) * sum(x): gemv_tiled_kernel.cuh) and the
8-bit forms multiply w and z separately (w - z needs 9 bits, bf16 has 8), so A is taken on the biased weights: A = |x| @ (|s| (2 (2^bits - 1) + 128)).  A dropped or
doubled term of ANY output -- large or small -- breaks it; the old tolerance only caught one at the scale of the largest output.  The reference's own
arithmetic (scales * (w - z) ROUNDED to fp16 per weight, qlinear_cuda_old.py:331-349) is further from y64 than this bound: the product is checked against the
exact expression here and against the reference's outputs in tests/test_oracle_golden.py / test_gpu_parity.py (fixtures, KATs, at the reference's tolerances).
"""
import os

import numpy as np
import pytest
import torch

from _error_model import DECODE_KERNELS, ulp as _ulp      # shared with test_gpu_error_model_edges.py: the same spacing table, the same C = 4 families
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEN = {}


def _layer(K, N, bits, gs, dtype, act, seed):
    L = O.random_quant_layer(K, N, bits, gs, dtype=dtype, seed=seed, act_order=act)
    q = QuantLinear(bits, gs, K, N, False, weight_dtype=dtype)
    q.qweight, q.qzeros, q.scales, q.g_idx = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone().to(torch.int32)
    q = q.to(DEV)
    q.post_init()
    mode = O.ZERO_NOWRAP if (bits == 3 or act) else O.ZERO_WRAP                   # zero_mode "auto": the reference class for this layer (qlinear_mi355x.resolved_zero_mode)
    assert q.resolved_zero_mode() == (_lib.ZERO_NOWRAP if mode == O.ZERO_NOWRAP else _lib.ZERO_WRAP)
    w = O.unpack_weights(L["qweight"], bits).astype(np.int32)
    z = O.unpack_zeros(L["qzeros"], bits, mode)
    g = L["g_idx"].cpu().numpy().astype(np.int64)
    s64 = L["scales"].double()[torch.from_numpy(g)]
    W64 = (s64 * torch.from_numpy((w - z[g]).astype(np.float64))).to(DEV)
    Sabs = s64.abs().to(DEV)
    return q, W64, Sabs


CASES = [
    # K, N, bits, gs, act, dtype
    (4096, 4096, 4, 128, False, torch.float16),
    (4096, 4096, 4, 128, True, torch.float16),
    (4096, 4096, 4, 128, False, torch.bfloat16),
    (4096, 4096, 4, 128, True, torch.bfloat16),
    (4096, 11008, 4, 128, False, torch.float16),
    (11008, 4096, 4, 128, True, torch.float16),
    (4096, 4096, 3, 32, False, torch.float16),
    (4096, 4096, 8, 32, False, torch.float16),
    (4096, 4096, 8, 32, True, torch.bfloat16),
    (4096, 4096, 2, 64, False, torch.float16),
    (2048, 2048, 4, -1, False, torch.float16),
]
ROWS = (1, 2, 3, 4, 7, 16, 64, 128, 256, 512, 2048)


@pytest.mark.parametrize("K,N,bits,gs,act,dtype", CASES)
def test_every_output_within_the_error_model(K, N, bits, gs, act, dtype):
    q, W64, Sabs = _layer(K, N, bits, gs, dtype, act, K + N + bits)
    Wabs = W64.abs()
    biased = dtype == torch.bfloat16                                             # the bf16 decode forms carry 128 + w through the matrix core (or a run sum)
    Wb = Sabs * float(2 * ((1 << bits) - 1) + 128) if biased else None
    worst = {}
    for M in ROWS:
        x = (torch.rand(M, K, generator=torch.Generator().manual_seed(M + K)) - 0.5).to(dtype).to(DEV)
        with torch.no_grad():
            y = q(x)
        plan = _lib.describe_plan(q._layer, M)
        x64 = x.double()
        y64 = x64 @ W64
        A = x64.abs() @ (Wb if biased else Wabs)
        C = 4.0 if plan["kernel"] in DECODE_KERNELS else (16.0 if (gs == -1 or gs >= 1024) else 8.0)
        bound = (0.5 + 1.0 / 64) * _ulp(y64, dtype) + C * (K ** 0.5) * 2.0 ** -24 * A
        err = (y.double() - y64).abs()
        ratio = float((err / bound).max())
        worst[(M, plan["kernel"])] = round(ratio, 3)
        SEEN[plan["kernel"]] = max(SEEN.get(plan["kernel"], 0.0), ratio)
        bad = err > bound
        if os.environ.get("GPTQ_ERR_MODEL_REPORT"):
            continue
        assert not bool(bad.any()), (f"int{bits} g{gs} {K}x{N} act={act} {dtype} M={M} [{plan['kernel']}]: {int(bad.sum())} / {bad.numel()} outputs outside the error model, "
                                     f"worst err / bound = {ratio:.3f} at {torch.nonzero(bad)[0].tolist()}")
    print(f"\nerror model int{bits} g{gs} {K}x{N} act={act} {str(dtype)[6:]}: worst err / bound per (M, kernel) = {worst}")


def test_the_error_model_saw_the_default_kernel_families():
    if not SEEN:
        pytest.skip("run together with the cases above")
    assert {"strips", "rows", "panel"} <= set(SEEN) and ({"wide_sk", "wide", "wide_copy"} & set(SEEN)), SEEN
    print(f"\nworst err / bound per kernel family: { {k: round(v, 3) for k, v in SEEN.items()} }")
