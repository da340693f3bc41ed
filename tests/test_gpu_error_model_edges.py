"""GPU: the per-output error model (tests/_error_model.py; test_gpu_error_model.py holds 11 full-size layers to it) at the EDGE shapes, on fp32 layers, with a
bias, and in value regimes that the rest of the suite never enters.  Every assertion is the model itself,

    |y - y64|  <=  (1/2 + 1/64) ulp(y64)  +  C sqrt(K) 2^-24 A,     A = |x| @ |W64|     (bf16: |W| on the biased weights),

with the project's existing constants (C = 4 decode families, 8 matrix-core GEMMs, 16 whole-K groups and the fp32 matrix-core GEMM; an fp32 layer on a decode
family has that family's 4: _error_model.constant_for); y64 = x @ W64 + bias and A are fp64 products of the exact dequantisation, formed on the device.  The
bias is added in fp32 in front of the one store, so it widens no term.  The bound scales with A, so an outlier activation or a scale 2^16 below its neighbour needs no tolerance of its own.

Finding, and the one extra term here: the matrix-core GEMM families (describe_plan: path=gemm) do NOT apply the scale to an fp32 group sum.
They feed the matrix core W = T(scales * (w - z)), every weight rounded once to the layer dtype -- the reference's W bit for bit, as their comments say
(_error_model.rounds_each_weight lists file and line per family).  With uniform x those K roundings average out below the sum term (which is why the 11
full-size cases pass without them); under an outlier the rounding of the one weight it meets is the whole error: mid at 9 rows 9.7 - 14.9 x the plain bound,
skinny64 6.7 x, the multi-layer rows kernel 7.5 x, and already 1.8 x with uniform x on 512 x 2048 g512 int3.  No kernel is wrong: at every output examined,
y is the correctly rounded fp64 product of the rounded weights.  Their bound therefore carries the K roundings as explicit ulp terms,
sum_k |x_k| (1/2 + 1/64) ulp(W64[k, n]) through extra_roundings, and takes the store's ulp at the value the store sees (_error_model.bound).  C stays 8 / 16.

2a  the edge table (EDGES below): uniform x, the oracle's scales, bias on; fp16 / bf16 / fp32, plain / act-order, with / without the decode copy, both zero-point
    conventions on plain layers; 14 row counts on both sides of every planner threshold; the default plan twice (equal bits), every output inside the bound.
2b  value regimes on the rows with K in {96, 1056, 4160} and 512 x 2048 g512: (outlier, narrow), (uniform, wide), (outlier, wide), (runs, narrow), (runs, wide)
    -- _error_model.make_x / wide_scales.  Precondition, asserted: y64 finite and max A + max|bias| < finfo(dtype).max / 4.  Computed on the CPU for every
    entry, regime and dtype before this file was written: the closest is 512 x 2048 g512 int8 fp16 (runs, wide) at 0.55 of the limit, so no entry needed a
    lowered top exponent.
2c  the gated epilogues at the FUSED sites (describe_plan: epilogue=fused): the pair form of the decode-copy kernel at 1..4 rows and the fused GEMV epilogue of
    the checkpoint-row family, SiLU and tanh-GELU, the bound propagated through act * mul as test_gpu_moe_decode.check does.
2d  forward_multi: three layers of one x, uniform and (outlier, wide).
2e  the closing test: the default plans of 2a / 2b reached exactly FAMILIES (frozen from a host-only walk of the tables through gptq_describe_plan:
    test_error_model_host.py repeats that walk without a GPU).

Table entries: every entry of the table is accepted by post_init and the forward (none replaced); the planner refuses none (host walk).  3-bit layers take
the group sizes that are multiples of 32 (96 x 96: 32, 96).  Families that no table entry reaches, left to the full-size cases of test_gpu_error_model.py: see
FAMILIES.

Measured on the MI355X (profiles/error_model_edges_gpu.log; 305 cases, 53 340 (layer, M) forwards of 2a / 2b, 34 s), worst err / bound per kernel family over
all dtypes and regimes: strips 0.970, generic 0.970, mfma 0.969, mfma_generic 0.970 (C = 4); rows 0.305, panel 0.965, mid 0.965, skinny64 0.968, strip16 0.967,
tiled 0.969 (C = 8 / 16 and the weight roundings); pair form and fused GEMV epilogue 0.853 (SiLU), 0.849 (tanh-GELU); forward_multi 0.956.  fp32 layers:
generic (C = 4) 0.245 with uniform x and the oracle's scales, 0.828 under an outlier, 0.957 - 0.970 with wide scales or block-wise exponents; f32_mfma (C = 16)
0.018 / 0.140 / 0.173 and 0.801 - 0.959.  A ratio of 0.96 - 0.97 is the store's half ulp over (1/2 + 1/64) ulp -- on fp32 layers too, at outputs whose sum is
small beside the bias: the sum and weight terms are not what is used up.  No xfail, no kernel change.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _error_model as EM
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear, forward_multi
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float16, torch.bfloat16, torch.float32)
ROWS = (1, 2, 3, 4, 5, 8, 9, 17, 64, 65, 128, 129, 300, 1024)
# K, N, group sizes (2 / 4 / 8 bits), group sizes (3 bits: multiples of 32), the edge
EDGES = [
    (64, 32, (8, 32, 64), (32, 64), "smallest legal layer; one chunk or less"),
    (96, 96, (12, 24, 48, 96), (32, 96), "groups that are not whole packing units; N not a multiple of 64"),
    (160, 64, (16, 32, 160), (32, 160), "K not a power of two"),
    (1056, 1056, (32, 48, 96), (32, 96), "ragged K chunks and a ragged last column tile"),
    (2112, 256, (64,), (64,), "in-launch K slices with a tail"),
    (4160, 96, (32, 64, 160), (32, 64, 160), "long ragged K, narrow N"),
    (512, 2048, (128, 512), (128, 512), "whole-K group (C = 16) beside g128"),
    (1024, 1024, (128,), (128,), "the aligned control"),
]
EDGE_CASES = [(K, N, gs, bits) for K, N, g248, g3, _ in EDGES for bits in (2, 3, 4, 8) for gs in (g3 if bits == 3 else g248)]
REGIME_CASES = [c for c in EDGE_CASES if c[0] in (96, 1056, 4160) or c[:3] == (512, 2048, 512)]
REGIMES_2B = [r for r in EM.REGIMES if r != ("uniform", "narrow")]
# The kernel families the default plans of EDGE_CASES land on (host walk: planned_families(); (layer, M) cases: generic 7266, mfma_generic 3552, tiled 2874,
# skinny64 1398, strips 1200, mid 1134, mfma 576, strip16 486, panel 144, f32_mfma 138, rows 132).  Reached by no shape this small, and left to the full-size
# cases of test_gpu_error_model.py: stream, stream64, wide_sk, wide, wide_copy (the streamed GEMVs and the stream-K / wide-tile prefill GEMMs want layers of
# 2048 x 2048 and more).
FAMILIES = frozenset(("strips", "generic", "mfma", "mfma_generic", "rows", "panel", "mid", "skinny64", "strip16", "tiled", "f32_mfma"))
SEEN = {}
WORST = {}
CASES_RUN = set()


def _case_id(c):
    return f"{c[0]}x{c[1]}-g{c[2]}-int{c[3]}"


def _module(L, bits, gs, dtype, copy, zm, epilogue="none"):
    q = QuantLinear(bits, gs, L["K"], L["N"], True, weight_dtype=dtype, zero_mode=zm, epilogue=epilogue)
    q.qweight, q.qzeros, q.scales, q.g_idx, q.bias = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone().to(torch.int32), L["bias"].clone()
    q = q.to(DEV)
    q.post_init(tiled=copy)
    assert (q._qweight_tiled is not None) <= copy
    return q


def _zero_modes(act, bits, both):
    if act:
        return ("nowrap",)
    return ("wrap", "nowrap") if both else (("nowrap",) if bits == 3 else ("wrap",))


def _record(kernel, dtype, regime, ratio):
    key = (kernel, EM.NAMES[dtype], "-".join(regime))
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    return key


def _sweep(K, N, gs, bits, regime, both_zero_modes):
    """Every (dtype, act-order, zero mode, copy, M) of one table entry in one regime; returns the worst err / bound per (kernel, dtype, regime)."""
    xr, sr = regime
    worst = {}
    for dtype in DTYPES:
        xs = {M: EM.make_x(xr, M, K, dtype, K * 7 + M).to(dtype).to(DEV) for M in ROWS}
        for act in (False, True):
            L = EM.make_layer(K, N, bits, gs, dtype, act, sr, seed=K + N + bits + gs)
            b64 = L["bias"].to(DEV).double()
            for zm in _zero_modes(act, bits, both_zero_modes):
                W64 = EM.w64(L, bits, O.ZERO_NOWRAP if zm == "nowrap" else O.ZERO_WRAP, DEV)
                Wabs = EM.abs_weights(L, bits, dtype, W64)
                mods = [(copy, _module(L, bits, gs, dtype, copy, zm)) for copy in (True, False)]
                for M, x in xs.items():
                    x64 = x.double()
                    y64 = x64 @ W64 + b64
                    Ax = x64.abs() @ Wabs
                    assert bool(torch.isfinite(y64).all()) and float(Ax.max()) + float(b64.abs().max()) < torch.finfo(dtype).max / 4, \
                        f"precondition: max A {float(Ax.max()):.4g} + max|bias| against {torch.finfo(dtype).max / 4:.4g}"
                    for copy, q in mods:
                        what = f"int{bits} g{gs} {K}x{N} {EM.NAMES[dtype]} act={act} zero={zm} copy={copy} M={M} x={xr} scales={sr}"
                        with torch.no_grad():
                            y, y2 = q(x), q(x)
                        plan = _lib.describe_plan(q._layer, M)
                        assert torch.equal(y, y2), f"{what}: not reproducible: {plan}"
                        bnd = EM.bound(y64, Ax, K, dtype, EM.constant_for(plan, dtype, -1 if gs >= K else gs),
                                       ((x64, W64),) if EM.rounds_each_weight(plan, dtype) else ())
                        err = (y.double() - y64).abs()
                        ratio = float((err / bnd).max())
                        SEEN[plan["kernel"]] = SEEN.get(plan["kernel"], 0) + 1
                        key = _record(plan["kernel"], dtype, regime, ratio)
                        worst[key] = max(worst.get(key, 0.0), ratio)
                        bad = err > bnd
                        assert not bool(bad.any()), (f"{what} [{plan['kernel']}]: {int(bad.sum())} / {bad.numel()} outputs outside the error model, "
                                                     f"worst err / bound = {ratio:.3f} at {torch.nonzero(bad)[0].tolist()}")
    return worst


def _fmt(worst):
    return ", ".join(f"{k[0]}/{k[1]}/{k[2]} {v:.3f}" for k, v in sorted(worst.items()))


# ---- 2a ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,gs,bits", EDGE_CASES, ids=[_case_id(c) for c in EDGE_CASES])
def test_edge_table_within_the_error_model(K, N, gs, bits):
    worst = _sweep(K, N, gs, bits, ("uniform", "narrow"), True)
    CASES_RUN.add((K, N, gs, bits))
    print(f"\nedges int{bits} g{gs} {K}x{N}: worst err / bound per (kernel, dtype, regime): {_fmt(worst)}")


# ---- 2b ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES_2B, ids=["-".join(r) for r in REGIMES_2B])
@pytest.mark.parametrize("K,N,gs,bits", REGIME_CASES, ids=[_case_id(c) for c in REGIME_CASES])
def test_value_regimes_within_the_error_model(K, N, gs, bits, regime):
    worst = _sweep(K, N, gs, bits, regime, False)
    print(f"\nregimes int{bits} g{gs} {K}x{N}: worst err / bound per (kernel, dtype, regime): {_fmt(worst)}")


# ---- 2c ------------------------------------------------------------------------------------------------------------------------------------------------
GATED_ROWS = (1, 2, 3, 4, 5, 8, 16)
FUSED_GEMV_ROWS = {"tiny": [1, 2, 3, 4], "ragged-k": [], "int3": [], "int8": []}      # of GATED_ROWS, layers without the decode copy (test_error_model_host.py walks it)
ACTS = {"silu_mul": lambda g: g * torch.sigmoid(g), "gelu_tanh_mul": lambda g: F.gelu(g, approximate="tanh")}


def _gated_check(q, Lg, Lu, K, gs, bits, dtype, epi, rows, what):
    """The rows whose plan says epilogue=fused, against act(g64) * u64 with the bound propagated through act * mul:
    (1/2 + 1/64) ulp(h64) + 1.13 Eg (|u64| + Eu) + |act(g64)| Eu + 1e-6 |h64|; Eg, Eu: the sum terms of the two halves (1.13 bounds the slope of SiLU, 1.10,
    and of tanh-GELU, 1.13; 1e-6: the __expf term of test_gpu_moe_decode.check).  Returns the fused row counts."""
    mode = O.reference_zero_mode(False, bits)
    halves = []
    for L in (Lg, Lu):
        W64 = EM.w64(L, bits, mode, DEV)
        halves.append((W64, EM.abs_weights(L, bits, dtype, W64), L["bias"].to(DEV).double()))
    fused, gmax = [], 0.0
    for M in rows:
        plan = _lib.describe_plan(q._layer, M)
        if plan["epilogue"] != "fused":
            continue
        fused.append(M)
        x = (torch.rand(M, K, generator=torch.Generator().manual_seed(K + M)) - 0.5).to(dtype).to(DEV)
        with torch.no_grad():
            y, y2 = q(x), q(x)
        assert torch.equal(y, y2), (what, M, plan)
        x64 = x.double()
        C = EM.constant_for(plan, dtype, -1 if gs >= K else gs)
        (g64, Eg), (u64, Eu) = [(x64 @ W + b, C * K ** 0.5 * 2.0 ** -24 * (x64.abs() @ Wa)) for W, Wa, b in halves]
        a64 = ACTS[epi](g64)
        h64 = a64 * u64
        bnd = (0.5 + 1 / 64) * EM.ulp(h64, dtype) + 1.13 * Eg * (u64.abs() + Eu) + a64.abs() * Eu + 1e-6 * h64.abs()
        err = (y.double() - h64).abs()
        ratio = float((err / bnd).max())
        gmax = max(gmax, float(g64.abs().max()))
        _record(plan["kernel"] + "+" + epi, dtype, ("uniform", "scaled-up"), ratio)
        bad = err > bnd
        assert not bool(bad.any()), f"{what} M={M} [{plan['kernel']}, fused]: {int(bad.sum())} / {bad.numel()} outside the bound, worst err / bound = {ratio:.3f}"
        print(f"{what} M={M} [{plan['kernel']}, fused]: worst err / bound {ratio:.3f}")
    assert not fused or gmax > 1.0, gmax                          # the activation off its linear part
    return fused


@pytest.mark.parametrize("epi", ["silu_mul", "gelu_tanh_mul"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", ["tiny", "ragged-k", "int3", "int8"])
def test_gated_epilogues_at_the_fused_sites(shape, dtype, epi):
    import test_gpu_gated_act as GA
    from autogptq_amd.fused import fuse_gate_up
    K, I, gs, bits = GA.PAIR_SHAPES[GA.PAIR_IDS.index(shape)]
    Lg, Lu, _, _ = GA._gate_up(K, I, gs, bits, dtype)             # its layers and scaled-up scales (max|g| > 1); its dequantised weights are not used here
    act = {"silu_mul": "silu", "gelu_tanh_mul": "gelu_tanh"}[epi]
    sites = {}
    for copy in (True, False):
        q = fuse_gate_up(GA._module(Lg, bits, gs, dtype), GA._module(Lu, bits, gs, dtype), act=act).to(DEV)
        assert q.epilogue == epi
        q.post_init(tiled=copy)
        sites[copy] = _gated_check(q, Lg, Lu, K, gs, bits, dtype, epi, GATED_ROWS, f"{epi} {shape} {EM.NAMES[dtype]} copy={copy}")
    assert sites[True] == [1, 2, 3, 4], sites                    # the pair form of the decode-copy kernel
    # the fused GEMV epilogue of the checkpoint-row family: of these shapes only `tiny` has it (host walk through gptq_describe_plan: the wider and deeper
    # layers without a copy run their GEMV plain and SiLU * mul as a pass of its own -- a staged form, left with test_gpu_gated_act.py's tolerances)
    assert sites[False] == FUSED_GEMV_ROWS[shape], sites


# ---- 2d ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", [("uniform", "narrow"), ("outlier", "wide")], ids=["uniform-narrow", "outlier-wide"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("bits", [4, 8])
def test_forward_multi_within_the_error_model(bits, dtype, regime):
    """gptq_forward_multi reports no plan of its own: up to 4 rows its launches are decode kernels wherever the layer's own plan is one (the constant of the
    layer's own plan); beyond, a multi-layer matrix-core kernel (gemm_rows / gemm_mid / gemm_stream64: capi.hip route_forward_multi) may replace a layer's own
    GEMV: the larger of the layer's own constant and 8, and the matrix-core GEMMs' rounding of every weight (_error_model.rounds_each_weight)."""
    K, gs, widths = 1056, 96, (64, 256, 96)
    xr, sr = regime
    for copy in (True, False):
        Ls = [EM.make_layer(K, n, bits, gs, dtype, False, sr, seed=K + n + bits) for n in widths]
        mods = [_module(L, bits, gs, dtype, copy, "wrap") for L in Ls]
        refs = []
        for L in Ls:
            W64 = EM.w64(L, bits, O.ZERO_WRAP, DEV)
            refs.append((W64, EM.abs_weights(L, bits, dtype, W64), L["bias"].to(DEV).double()))
        for M in (1, 4, 5, 64, 130):
            x = EM.make_x(xr, M, K, dtype, K * 7 + M).to(dtype).to(DEV)
            with torch.no_grad():
                ys, ys2 = forward_multi(mods, x), forward_multi(mods, x)
            x64 = x.double()
            for q, y, y2, (W64, Wabs, b64) in zip(mods, ys, ys2, refs):
                assert torch.equal(y, y2)
                y64 = x64 @ W64 + b64
                Ax = x64.abs() @ Wabs
                assert bool(torch.isfinite(y64).all()) and float(Ax.max()) + float(b64.abs().max()) < torch.finfo(dtype).max / 4
                own = EM.constant_for(_lib.describe_plan(q._layer, M), dtype, gs)
                bnd = EM.bound(y64, Ax, K, dtype, own if M <= 4 else max(own, 8.0), () if M <= 4 else ((x64, W64),))
                err = (y.double() - y64).abs()
                ratio = float((err / bnd).max())
                _record("multi", dtype, regime, ratio)
                bad = err > bnd
                assert not bool(bad.any()), (f"forward_multi int{bits} {EM.NAMES[dtype]} copy={copy} M={M} width {q.outfeatures} {regime}: {int(bad.sum())} / {bad.numel()} "
                                             f"outputs outside the error model, worst err / bound = {ratio:.3f}")
    print(f"\nforward_multi int{bits} {EM.NAMES[dtype]} {regime}: worst err / bound {WORST[('multi', EM.NAMES[dtype], '-'.join(regime))]:.3f}")


# ---- 2e ------------------------------------------------------------------------------------------------------------------------------------------------
def host_layer(K, N, bits, gs, dtype, act, copy, zero_mode, epilogue="none"):
    """What post_init hands the planner for such a layer, with pointers that are never dereferenced (host only, as tests/test_host_logic.py does): act-order
    layers of uniform groups carry their re-sequenced rows, the decode copy exists where gptq_prepack_decode_bytes accepts the layer."""
    lib = _lib.load()
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = L.bias = 0x1000
    L.K, L.N, L.bits, L.group_size, L.dtype = K, N, bits, gs, _lib.DTYPE_ENUM[dtype]
    L.zero_mode = _lib.ZERO_NOWRAP if zero_mode == "nowrap" else _lib.ZERO_WRAP
    L.epilogue = _lib.EPILOGUE_ENUM[epilogue]
    if act:
        g = EM.make_layer(K, N, bits, gs, dtype, True, seed=K + N + bits + gs)["g_idx"].to(torch.int32).contiguous()
        perm = torch.empty(K, dtype=torch.int32)
        uniform = ctypes.c_int(0)
        _lib.check(lib.gptq_make_sequential(g.data_ptr(), K, gs, perm.data_ptr(), ctypes.byref(uniform)))
        L.g_idx = 0x1000
        if uniform.value:
            L.qweight_seq = L.perm = 0x1000
    if copy:
        tb, cb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if lib.gptq_prepack_decode_bytes(ctypes.byref(L), ctypes.byref(tb), ctypes.byref(cb)) == 0:
            L.qweight_tiled = L.qconst_tiled = 0x2000
            L.tiled_cols = _lib.STRIP_COLS
    return L


def planned_families():
    """kernel -> count over every (layer, M) of EDGE_CASES, from gptq_describe_plan alone."""
    seen = {}
    for K, N, gs, bits in EDGE_CASES:
        for dtype in DTYPES:
            for act in (False, True):
                for zm in _zero_modes(act, bits, True):
                    for copy in (True, False):
                        L = host_layer(K, N, bits, gs, dtype, act, copy, zm)
                        for M in ROWS:
                            k = _lib.describe_plan(L, M)["kernel"]
                            seen[k] = seen.get(k, 0) + 1
    return seen


def test_the_edge_tables_reached_their_kernel_families():
    """Runs last in this file: the default plans of 2a / 2b landed on exactly the frozen set, so the grid cannot shrink silently."""
    if not SEEN:
        pytest.skip("run together with the cases above")
    assert {"strips", "generic", "rows"} <= FAMILIES and FAMILIES - set(EM.DECODE_KERNELS) - {"rows"}
    if CASES_RUN >= set(EDGE_CASES):
        assert set(SEEN) == FAMILIES, (sorted(SEEN), sorted(FAMILIES))
    else:
        assert set(SEEN) <= FAMILIES, (sorted(SEEN), sorted(FAMILIES))
    fam = {}
    for (k, d, r), v in WORST.items():
        fam[k] = max(fam.get(k, 0.0), v)
    print("\nworst err / bound per (kernel family, dtype, regime):")
    for key, v in sorted(WORST.items()):
        print(f"  {key[0]:28s} {key[1]:5s} {key[2]:18s} {v:.3f}")
    print(f"worst err / bound per kernel family: { {k: round(v, 3) for k, v in sorted(fam.items())} }")
    print(f"(layer, M) cases per kernel family: {dict(sorted(SEEN.items()))}")
