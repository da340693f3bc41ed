"""The per-output error model of the dense forward, shared by test_gpu_error_model.py, test_gpu_error_model_edges.py and test_error_model_host.py (a helper
module: no pytest hooks, no fixtures).  What the decode kernels compute is w - z as exact integers, exact products with x in fp32, fp32 sums per group, the
group's scale applied to the fp32 sum, the bias added in fp32, ONE rounding to the layer dtype at the store; against the fp64 value of the same expression

    |y - y64|  <=  (1/2 + 1/64) ulp_dtype(y64)  +  C * sqrt(K) * 2^-24 * A,        A = |x| @ |W64|   (the condition of that output's sum; the bias adds nothing to it)

The matrix-core GEMMs round every weight to the layer dtype first (the reference's W, bit for bit: rounds_each_weight below); their bound carries those K
roundings as explicit ulp terms.  With uniform x they average out below the sum term, which is why the full-size cases of test_gpu_error_model.py pass
without them; under an outlier activation the rounding of the one weight it meets is the whole error of an output.
The bound scales with A, so it needs no tolerance per value regime: an outlier activation raises the bound of the outputs it feeds and of no other.  The
value regimes (outlier activations, block-wise exponents with all-zero runs, scales spread over many binades) are built here too, seeded, on the CPU."""
import math

import numpy as np
import torch

from oracle import gptq_oracle as O

MANT_EMIN = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}      # the table of test_gpu_grad_input._ulp
DECODE_KERNELS = ("strips", "mfma", "mfma_generic", "generic", "stream")      # fp32 sums per group outside the matrix core's long chains: C = 4
NAMES = {torch.float16: "fp16", torch.bfloat16: "bf16", torch.float32: "fp32"}
REGIMES = (("uniform", "narrow"), ("outlier", "narrow"), ("uniform", "wide"), ("outlier", "wide"), ("runs", "narrow"), ("runs", "wide"))


def ulp(v64, dtype):
    """Spacing of `dtype` at |v64| (normal range; the subnormal floor for tiny values)."""
    mant, emin = MANT_EMIN[dtype]
    e = torch.floor(torch.log2(v64.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v64.device), e - mant)


def w64(L, bits, zero_mode, device):
    """The layer's exact weights in fp64 on `device` (oracle.forward_f64's dequant, once per layer): scales[g] * (w - z[g])."""
    w = O.unpack_weights(L["qweight"], bits).astype(np.int32)
    z = O.unpack_zeros(L["qzeros"], bits, zero_mode)
    g = torch.from_numpy(L["g_idx"].cpu().numpy().astype(np.int64)).to(device)
    return L["scales"].to(device).double()[g] * torch.from_numpy(w - z[g.cpu().numpy()]).to(device).double()


def abs_weights(L, bits, dtype, W64):
    """|W64| -- for bf16 layers on the biased weights, |s| (2 (2^bits - 1) + 128): the bf16 decode forms carry 128 + w through the matrix core (or a run
    sum) and the 8-bit forms multiply w and z separately (test_gpu_error_model.py's docstring)."""
    if dtype != torch.bfloat16:
        return W64.abs()
    g = torch.from_numpy(L["g_idx"].cpu().numpy().astype(np.int64)).to(W64.device)
    return L["scales"].to(W64.device).double().abs()[g] * float(2 * ((1 << bits) - 1) + 128)


def bound(y64, A, K, dtype, C, extra_roundings=()):
    """The model's bound per output.  `extra_roundings`: what the DOCUMENTED arithmetic of a kernel family rounds to the layer dtype on the way, one more
    (1/2 + 1/64) ulp each (as test_gpu_grad_input._check(partials=) accounts for accumulate steps).  An entry is an fp64 tensor of values of the outputs'
    shape, or a pair (coef [M, K], values [K, N]): K roundings per output, the error of the one at k carried to output (m, n) by |coef[m, k]| --
    sum_k |coef[m, k]| (1/2 + 1/64) ulp(values[k, n]); a value that is exactly zero has no rounding.
    The store rounds what the kernel summed, not y64: with such roundings in front of it that sum lies up to `pre` (their total and the sum term) away from
    y64 -- across a power of two, where the spacing doubles, if y64 sits just below one -- so the store's ulp is then taken at |y64| + pre.  (Measured, the
    only outputs outside the bound with ulp(y64) there -- 14 single outputs of test_gpu_error_model_edges.py's grid, err / bound 1.005 - 1.11, all of this kind: y64 = 7.99965, the fp64 product of the rounded weights 8.00394, the
    kernel's y = 8.0078 = fp16(8.00394); 15.9756 / 16.063 / 16.125 in bf16; 3.9994 / 4.0023 / 4.0039.)  Without extra roundings the formula is the
    project's own, ulp at y64."""
    pre = C * math.sqrt(K) * 2.0 ** -24 * A
    for p in extra_roundings:
        if isinstance(p, tuple):
            coef, v = p
            pre = pre + coef.abs() @ ((0.5 + 1.0 / 64) * ulp(v, dtype) * (v != 0))
        else:
            pre = pre + (0.5 + 1.0 / 64) * ulp(p, dtype)
    return (0.5 + 1.0 / 64) * ulp(y64.abs() + pre if extra_roundings else y64, dtype) + pre


def rounds_each_weight(plan, dtype):
    """The matrix-core GEMM families (describe_plan: path=gemm) feed the matrix core W = T(scales * (w - z)): w - z exact, ONE rounding of every weight to the
    layer dtype T, "the reference's scales * (weight - zeros), bit for bit" -- csrc/gemm.hip:20-26 and :299-301 (tiled, skinny64, strip16, stream64),
    gemm_mid.hip:80-81 and :132 (mid), gemm_rows_kernel.cuh:46 (rows), gemm_panel_kernel.cuh:13 (panel), gemm_wide_common.cuh:61 and :101 (wide, wide_sk,
    wide_copy).  Their bound carries those K roundings: extra_roundings=((x64, W64),).  The decode families (path=gemv) apply the scale to the fp32 sum of
    a group and round no weight; an fp32 layer's weights are exact fp32 products (gemm.hip:1488-1497)."""
    return plan.get("path") == "gemm" and dtype != torch.float32


def constant_for(plan, dtype, group_size):
    """C of the bound: the project's existing constants (test_gpu_error_model.py, test_gpu_grad_input.py), nothing fitted here.  `plan`: describe_plan's
    dict or its kernel name; `group_size`: -1 (or anything >= 1024) for a group that spans the whole K.
    fp32 layers: 16 on their matrix-core GEMM (f32_mfma: one unbroken chain over K, test_gpu_grad_input.py's fp32 constant), but 4 on a decode family.  The sum
    term models the fp32 accumulation, and that does not depend on the dtype of the store: gemv_generic.hip:114-128 is one template for every T -- x widened to
    fp32, w - z an exact integer, fmaf into the group's sum, the scale by fmaf into the accumulator -- so an fp32 layer gets the constant its fp16 twin has.  With
    16 there the bound could not see x rounded to fp16 at K = 1056 (test_error_model_host.py: worst err / bound 0.73); 4 is the stricter of the two."""
    kernel = plan["kernel"] if isinstance(plan, dict) else plan
    if kernel in DECODE_KERNELS:
        return 4.0
    if dtype == torch.float32:
        return 16.0
    return 16.0 if (group_size == -1 or group_size >= 1024) else 8.0


# ---- value regimes -------------------------------------------------------------------------------------------------------------------------------------
def make_x(regime, M, K, dtype, seed):
    """[M, K] activations in fp32 on the CPU (cast by the caller).  'uniform': rand - 0.5, the suite's own.  'outlier': (rand - 0.5) 2^-6 with four positions
    per row at +-48.  'runs': per (row, run of 32 consecutive k) values (rand - 0.5) 2^e, e an integer uniform in [-12, 4] (fp16, fp32) or [-40, 12] (bf16),
    one run in four all exact zeros."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(M, K, generator=gen) - 0.5
    if regime == "uniform":
        return u
    if regime == "outlier":
        x = u * 2.0 ** -6
        pos = torch.rand(M, K, generator=gen).topk(4, dim=1).indices      # four distinct positions per row
        sign = torch.randint(0, 2, (M, 4), generator=gen).float() * 2 - 1
        x.scatter_(1, pos, sign * 48.0)
        return x
    assert regime == "runs", regime
    lo, hi = (-40, 12) if dtype == torch.bfloat16 else (-12, 4)
    R = K // 32
    e = torch.randint(lo, hi + 1, (M, R), generator=gen).float()
    keep = (torch.randint(0, 4, (M, R), generator=gen) != 0).float()
    return u * (torch.exp2(e) * keep).repeat_interleave(32, dim=1)


def wide_scales(G, N, dtype, seed):
    """2^u (1 + 0.5 rand) per (group, column), u an integer uniform in [-14, -4] (fp16) or [-20, -4] (bf16, fp32)."""
    gen = torch.Generator().manual_seed(seed)
    lo = -14 if dtype == torch.float16 else -20
    u = torch.randint(lo, -4 + 1, (G, N), generator=gen).float()
    return (torch.exp2(u) * (1 + 0.5 * torch.rand(G, N, generator=gen))).to(dtype)


def make_layer(K, N, bits, gs, dtype, act, scales="narrow", seed=0):
    """The oracle's random layer with a bias; 'wide' replaces its scales and keeps its qweight / qzeros."""
    L = O.random_quant_layer(K, N, bits, gs, act_order=act, dtype=dtype, seed=seed, bias=True)
    if scales == "wide":
        L["scales"] = wide_scales(L["scales"].shape[0], N, dtype, seed + 1)
    return L
