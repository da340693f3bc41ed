"""GPU: the GeGLU epilogue ('gelu_tanh_mul') and the fused MLP callers for Gemma and Phi-3.  The activation is a launch-uniform argument of the five dense
sites that formed SiLU * mul (the pair form of the decode-copy kernel, the fused GEMV epilogue of the checkpoint-row family, silu_mul_kernel, silu_mul2_kernel,
silu_mul2_permute_rows4_kernel); every site is driven here with tanh-GELU and compared, output by output, with fp64 F.gelu(g, approximate='tanh') * u formed
from the oracle's dequantised weights.  Tolerances are the ones the SiLU tests of the same arithmetic use (tanh-GELU's slope stays within 3 % of SiLU's maximum
slope, 1.13 against 1.10).  Every case also requires the SiLU reference to FAIL the same check on the same output -- a kernel that ignored the argument would
otherwise pass wherever the pre-activations are small -- and the SiLU path to give the bits it gave before it became an argument."""
import functools

import pytest
import torch
import torch.nn.functional as F

from autogptq_amd import _lib
from autogptq_amd import qlinear_mi355x as qm
from autogptq_amd.fused import FusedGateUpMLP, fuse_gate_up, inject_fused_llama, remove_fused_mlp
from autogptq_amd.qlinear_mi355x import QuantLinear, mlp_forward
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIR_TOL = {torch.float16: (2e-3, 2e-3), torch.bfloat16: (1.6e-2, 1.6e-2)}      # (rtol, atol): atol * max|ref| + rtol * |ref| -- one rounding of the product of two sums
STAGED_TOL = {torch.float16: 4e-3, torch.bfloat16: 3e-2}                        # rtol * (|ref| + 0.05 max|ref|) -- up to 3 roundings to T on the unfused path
MLP_TOL = {torch.float16: (4e-3, 2e-3), torch.bfloat16: (3e-2, 1.6e-2)}         # (rtol, atol) of test_mlp_forward_one_call: three roundings to T in front of a K = I matmul
PAIR_SHAPES = [(160, 32, 32, 4), (1024, 704, 128, 4), (2112, 96, 64, 4), (1024, 1408, 32, 3), (1024, 1408, 32, 8)]
PAIR_IDS = ["tiny", "1024x704", "ragged-k", "int3", "int8"]


def gelu_tanh(g):
    return F.gelu(g, approximate="tanh")


def _module(L, bits, gs, dtype):
    m = QuantLinear(bits, gs, L["qweight"].shape[0] * 32 // bits, L["qweight"].shape[1], L.get("bias") is not None, weight_dtype=dtype)
    m.qweight, m.qzeros, m.scales, m.g_idx = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone()
    if L.get("bias") is not None:
        m.bias = L["bias"].clone()
    return m


def _w64(L, bits, act):
    W = O.dequantize(L["qweight"], L["qzeros"], L["scales"], L["g_idx"], bits, O.reference_zero_mode(act, bits)).to(DEV).double()
    return W, (L["bias"].to(DEV).double() if L.get("bias") is not None else 0.0)


@functools.lru_cache(maxsize=None)
def _gate_up(K, I, gs, bits, dtype, act=False, mult=None):
    """Oracle layers of one [gate | up] pair (scales scaled up as the SiLU tests do: gate pre-activations beyond 1, the activation off its linear part)
    and their dequantised fp64 weights on the device.  Built once per shape; nothing in it is modified."""
    Lg = O.random_quant_layer(K, I, bits, gs, dtype=dtype, seed=K + I, bias=True, act_order=act)
    Lu = O.random_quant_layer(K, I, bits, gs, dtype=dtype, seed=K + I + 1, bias=True, act_order=act)
    Lu["g_idx"] = Lg["g_idx"].clone()                 # a fused pair shares its input permutation
    # 8-bit fields are 16 x the 4-bit ones: without the 1/16 the pre-activations reach 40, where tanh-GELU and SiLU are both the identity (or zero) and the
    # SiLU reference could not fail -- the two differ most around |g| = 2
    for L in (Lg, Lu):
        L["scales"] = (L["scales"].float() * (mult or (8 if K < 2048 else 4)) / (16 if bits == 8 else 1)).to(dtype)
    return Lg, Lu, _w64(Lg, bits, act), _w64(Lu, bits, act)


def _x(M, K, dtype, seed):
    return (torch.rand(M, K, generator=torch.Generator().manual_seed(seed)) - 0.5).to(dtype).to(DEV)


def _pre(x, Wb):
    return x.double() @ Wb[0] + Wb[1]


def _pair_bad(y, ref, dtype, margin=1.0):
    rtol, atol = PAIR_TOL[dtype]
    return (y.double() - ref).abs() > margin * (atol * float(ref.abs().max()) + rtol * ref.abs())


def _staged_bad(y, ref, dtype):
    return (y.double() - ref).abs() > STAGED_TOL[dtype] * (ref.abs() + 0.05 * float(ref.abs().max()))


def _check(bad_fn, y, g64, u64, dtype, what, **kw):
    """y is tanh-GELU(g) * u everywhere, and is NOT SiLU(g) * u (same check, same output)."""
    ref = gelu_tanh(g64) * u64
    bad = bad_fn(y, ref, dtype, **kw)
    worst = float(((y.double() - ref).abs() / (ref.abs() + 1e-3 * float(ref.abs().max()))).max())
    print(f"{what}: max|g| {float(g64.abs().max()):.3f}, worst relative error {worst:.2e}, {int(bad.sum())}/{bad.numel()} out of tolerance; "
          f"against SiLU: {int(bad_fn(y, F.silu(g64) * u64, dtype, **kw).sum())} out")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} outputs out of tolerance, first {torch.nonzero(bad)[0].tolist()}"
    assert bool(bad_fn(y, F.silu(g64) * u64, dtype, **kw).any()), f"{what}: the output also passes as SiLU * mul -- the activation argument is not exercised"


# ---- 1. the pair form of the decode-copy kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,I,gs,bits", PAIR_SHAPES, ids=PAIR_IDS)
def test_geglu_is_the_epilogue_of_the_decode_copy_kernel(K, I, gs, bits, dtype):
    """Decode rows of a 'gelu_tanh_mul' layer run the PAIR form of gemv_tiled_kernel (the plan of the same layer with 'silu_mul'), every output is
    gelu_tanh(x @ W_gate + b) * (x @ W_up + b), repeated calls give the same bits, the checkpoint tensors are untouched; 8 rows: the staged tail."""
    Lg, Lu, Wg, Wu = _gate_up(K, I, gs, bits, dtype)
    q = fuse_gate_up(_module(Lg, bits, gs, dtype), _module(Lu, bits, gs, dtype), act="gelu_tanh").to(DEV)
    assert q.epilogue == "gelu_tanh_mul"
    q.post_init()
    assert q._qweight_tiled is not None and q._layer.epilogue == _lib.EPI_GELU_TANH_MUL
    before = {k: v.clone() for k, v in q.state_dict().items()}
    gmax = 0.0
    for M in (1, 2, 3, 4):
        x = _x(M, K, dtype, M)
        d = _lib.describe_plan(q._layer, M)
        assert (d["kernel"], int(d["pair"]), d["epilogue"]) == ("strips", 1, "fused") and int(d["strips"]) == I // 16, d
        with torch.no_grad():
            y, y2 = q(x), q(x)
        assert tuple(y.shape) == (M, I) and y.dtype == dtype and torch.equal(y, y2)
        g64, u64 = _pre(x, Wg), _pre(x, Wu)
        gmax = max(gmax, float(g64.abs().max()))
        _check(_pair_bad, y, g64, u64, dtype, f"pair form {K}x2x{I} int{bits} M={M}")
    assert gmax > 1.0, gmax
    for k, v in q.state_dict().items():
        assert torch.equal(v, before[k]), k
    x8 = _x(8, K, dtype, 8)
    with torch.no_grad():
        y8 = q(x8)
    assert _lib.describe_plan(q._layer, 8)["epilogue"] == "separate"
    _check(_pair_bad, y8, _pre(x8, Wg), _pre(x8, Wu), dtype, f"staged tail {K}x2x{I} int{bits} M=8", margin=3.0)


# ---- 2. SiLU: the bits it gave before the activation became an argument ---------------------------------------------------------------------------
def _raw_mlp(fn, gate, up, down, x, *act):
    lib = _lib.load()
    M = x.shape[0]
    out = torch.empty((M, down.outfeatures), dtype=x.dtype, device=x.device)
    need = int(lib.gptq_workspace_bytes_mlp(gate._layer_ref, up._layer_ref, down._layer_ref, M))
    ws = qm.reserve_workspace(x.device, max(need, 1))
    _lib.check(getattr(lib, fn)(gate._layer_ref, up._layer_ref, down._layer_ref, *act, x.data_ptr(), out.data_ptr(), M, ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,I,gs,bits", PAIR_SHAPES, ids=PAIR_IDS)
def test_silu_keeps_its_bits(K, I, gs, bits, dtype):
    """gptq_mlp_forward and gptq_mlp_forward_act(SILU_MUL) return equal tensors (the former is a call of the latter) and differ from the GELU_TANH_MUL call;
    a 'silu_mul' layer is T(silu(g) * u) formed in fp32 from its own plain product to within one ulp of T (1.01 * 2^-10 / 2^-7 of the value: the bound
    test_mlp_forward_act_order_down_reads_the_permuted_activations_of_the_silu_pass puts on the same arithmetic) at the rows whose epilogue is a pass over
    that product (8, 130).  At the rows of the pair form (1, 4) the product is NOT what the kernel reads, and the literal one-ulp bound is missed by a
    few outputs -- measured on this build, whose SiLU bits are the parent's (the golden test below): 1 of 128 (160 -> 2x32, fp16, 1.09 ulp), 10 of 2816
    (1024 -> 2x704, bf16, 1.15 ulp), 2 of 384 (2112 -> 2x96, fp16, 1.04 ulp); there the bound carries the two half-ulp roundings of the product itself."""
    Lg, Lu, _, _ = _gate_up(K, I, gs, bits, dtype)
    Ld = O.random_quant_layer(I, 64, 4, 32, dtype=dtype, seed=K + I + 2, bias=True)
    gate, up, down = (_module(L, b, g, dtype).to(DEV) for L, b, g in ((Lg, bits, gs), (Lu, bits, gs), (Ld, 4, 32)))
    for m in (gate, up, down):
        m.post_init()
    q = fuse_gate_up(_module(Lg, bits, gs, dtype), _module(Lu, bits, gs, dtype)).to(DEV)
    q.post_init()
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    for M in (1, 4, 8, 130):
        x = _x(M, K, dtype, 100 + M)
        a = _raw_mlp("gptq_mlp_forward", gate, up, down, x)
        b = _raw_mlp("gptq_mlp_forward_act", gate, up, down, x, _lib.EPI_SILU_MUL)
        c = _raw_mlp("gptq_mlp_forward_act", gate, up, down, x, _lib.EPI_GELU_TANH_MUL)
        with torch.no_grad():
            d = mlp_forward(gate, up, down, x)
        assert torch.equal(a, b) and torch.equal(a, d) and not torch.equal(a, c), M
        with torch.no_grad():
            y = q(x)
            p = q._plain_product(x).float()
        g32, u32 = p[:, :I], p[:, I:]
        want = g32 / (1 + torch.exp(-g32)) * u32
        fused = _lib.describe_plan(q._layer, M)["epilogue"] == "fused"
        # rows of the pair form: the kernel never sees the plain product -- it works on the fp32 sums, of which g32 and u32 are roundings to T (half an ulp
        # each); through silu (condition number |1 + g (1 - sigmoid(g))|) and the product they move `want` by that many half ulps on top of the one rounding
        kappa = (1 + g32 * (1 - torch.sigmoid(g32))).abs()
        allow = 1.01 * ulp * want.abs() * (1 + (0.5 * (kappa + 1) if fused else 0)) + 1e-7
        over = (y.float() - want).abs() - allow
        one = (y.float() - want).abs() - (1.01 * ulp * want.abs() + 1e-7)
        print(f"silu_mul layer {K}x2x{I} int{bits} M={M} ({'fused' if fused else 'separate'}): worst |y - want| / |want| = "
              f"{float(((y.float() - want).abs() / (want.abs() + 1e-7)).max()):.3e} (ulp {ulp:.3e}), {int((one > 0).sum())}/{one.numel()} beyond one ulp")
        assert not bool((over > 0).any()), (M, float(over.max()))


def test_silu_outputs_are_the_bits_of_the_commit_before():
    """tests/golden/silu_mul_bits.npz: what the five sites returned for SiLU, on seeded layers and inputs, before the activation became their argument
    (tests/_silu_bits.py run on that commit) -- the same expression with c = g must give the same bits."""
    import os
    import numpy as np
    import _silu_bits as SB
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "silu_mul_bits.npz"))
    got = dict(SB.cases())
    assert sorted(got) == sorted(want.files) and len(got) == 29
    diff = [k for k in want.files if got[k].numel() != want[k].size or not np.array_equal(SB.to_numpy(got[k]), want[k])]
    assert not diff, diff


# ---- 3. the checkpoint-row family: fused GEMV epilogue (gemv.hip) and silu_mul_kernel behind the staged y ----------------------------------------
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("M,dtype,bits", [(1, torch.float16, 4), (2, torch.float16, 4), (7, torch.float16, 4), (16, torch.float16, 4), (130, torch.float16, 4),
                                         (3, torch.float16, 8), (40, torch.bfloat16, 3)])
def test_geglu_on_layers_without_a_decode_copy(M, dtype, bits, act):
    K, N = 1024, 704
    saved = QuantLinear.TILED_DECODE
    QuantLinear.TILED_DECODE = False
    try:
        Lg, Lu, Wg, Wu = _gate_up(K, N, 128, bits, dtype, act, 4)
        q = fuse_gate_up(_module(Lg, bits, 128, dtype), _module(Lu, bits, 128, dtype), act="gelu_tanh").to(DEV)
        q.post_init()
        assert q._qweight_tiled is None
        x = _x(M, K, dtype, 4)
        with torch.no_grad():
            y, y2 = q(x), q(x)
        assert tuple(y.shape) == (M, N) and torch.equal(y, y2)
        d = _lib.describe_plan(q._layer, M)
        qs = fuse_gate_up(_module(Lg, bits, 128, dtype), _module(Lu, bits, 128, dtype)).to(DEV)      # the same layer with 'silu_mul': the same plan
        qs.post_init()
        sd = _lib.describe_plan(qs._layer, M)
    finally:
        QuantLinear.TILED_DECODE = saved
    g64, u64 = _pre(x, Wg), _pre(x, Wu)
    assert float(g64.abs().max()) > 1.0
    _check(_staged_bad, y, g64, u64, dtype, f"checkpoint rows int{bits} act={act} M={M} ({d['path']}/{d['kernel']}, epilogue={d['epilogue']})")
    assert sd == d


# ---- 4. mlp_forward(act='gelu_tanh'): silu_mul2_kernel and the one-pass activation + permute -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mlp(H, I, gs, down_act):
    dtype = torch.float16
    Lg = O.random_quant_layer(H, I, 4, gs, dtype=dtype, seed=H + I, bias=True)
    Lu = O.random_quant_layer(H, I, 4, gs, dtype=dtype, seed=H + I + 1, bias=True)
    Ld = O.random_quant_layer(I, H, 4, gs, dtype=dtype, seed=H + I + 2, bias=True, act_order=down_act)
    Lg["scales"] = (Lg["scales"].float() * 8).to(dtype)             # gate pre-activations beyond 1
    Lu["scales"] = (Lu["scales"].float() * 2).to(dtype)
    mods = [_module(L, 4, gs, dtype).to(DEV) for L in (Lg, Lu, Ld)]
    for m in mods:
        m.post_init()
    return mods, _w64(Lg, 4, False), _w64(Lu, 4, False), _w64(Ld, 4, down_act)


def _mlp_check(mods, Wg, Wu, Wd, M, what):
    """Against fp64 of the same expression, the activation rounded to the layer dtype where the library rounds it (the oracle of test_mlp_forward_one_call)."""
    dtype = torch.float16
    x = _x(M, Wg[0].shape[0], dtype, 200 + M)
    with torch.no_grad():
        y, y2 = mlp_forward(*mods, x, act="gelu_tanh"), mlp_forward(*mods, x, act="gelu_tanh")
        ys = mlp_forward(*mods, x)
    assert tuple(y.shape) == (M, mods[2].outfeatures) and y.dtype == dtype and torch.equal(y, y2)
    g64, u64 = _pre(x, Wg), _pre(x, Wu)
    assert float(g64.abs().max()) > 1.0
    rtol, atol = MLP_TOL[dtype]
    outs = {}
    for name, fn in (("gelu_tanh", gelu_tanh), ("silu", F.silu)):
        ref = (fn(g64) * u64).to(dtype).double() @ Wd[0] + Wd[1]
        outs[name] = lambda t, ref=ref: (t.double() - ref).abs() > rtol * ref.abs() + atol * float(ref.abs().max())
    bad = outs["gelu_tanh"](y)
    print(f"{what} M={M}: {int(bad.sum())}/{bad.numel()} out of tolerance; against the SiLU expression {int(outs['silu'](y).sum())} out")
    assert not bool(bad.any()), (what, M, int(bad.sum()))
    assert bool(outs["silu"](y).any()), "the output also passes as the SiLU MLP"
    assert not bool(outs["silu"](ys).any())                           # ... and act='silu' is still the SiLU MLP


@pytest.mark.parametrize("down_act", [False, True], ids=["down-seq", "down-act"])
def test_mlp_forward_gelu_tanh(down_act):
    mods, Wg, Wu, Wd = _mlp(256, 704, 64, down_act)
    for M in (1, 4, 40):
        _mlp_check(mods, Wg, Wu, Wd, M, f"mlp_forward 256/704 down_act={down_act}")
    with pytest.raises(ValueError, match="act must be"):
        mlp_forward(*mods, _x(1, 256, torch.float16, 1), act="gelu")


def test_mlp_forward_gelu_tanh_through_the_one_pass_activation_and_permute():
    """The act-order `down` of 256 / 704 never runs a GEMM that reads x permuted in natural order (gptq_describe_mlp_plan reports down_permute=fused for no row
    count up to 8192 there: the width is no multiple of the decode-copy GEMMs' K step), so silu_mul2_permute_rows4_kernel is driven on the smallest shape of the
    project's own test of that kernel, 1024 / 2048, at the smallest row count whose plan says down_permute=fused."""
    mods, Wg, Wu, Wd = _mlp(1024, 2048, 128, True)
    small = _mlp(256, 704, 64, True)[0]
    assert all(_lib.describe_mlp_plan(small[0]._layer, small[1]._layer, small[2]._layer, M)["down_permute"] != "fused" for M in (1, 4, 5, 8, 40, 130, 768, 2048, 8192))
    plan = lambda M: _lib.describe_mlp_plan(mods[0]._layer, mods[1]._layer, mods[2]._layer, M)
    M = next(M for M in range(1, 65) if plan(M)["down_permute"] == "fused")
    p = plan(M)
    assert p["down_permute"] == "fused" and "silu_mul+permute" in p["steps"] and M == 5, (M, p)
    _mlp_check(mods, Wg, Wu, Wd, M, "mlp_forward 1024/2048, down_permute=fused")


# ---- 5. the host model's modules -------------------------------------------------------------------------------------------------------------------------
def _quantised_mlp(kind, seed):
    """A tiny Gemma-2 / Phi-3 MLP (hidden 256, intermediate 704) whose linears are QuantLinears packed from its own random weights (oracle min/max quantizer)."""
    from autogptq_amd.model_utils import find_layers, pack_model
    torch.manual_seed(seed)
    if kind == "gemma2":
        from transformers import Gemma2Config
        from transformers.models.gemma2.modeling_gemma2 import Gemma2MLP
        mlp = Gemma2MLP(Gemma2Config(hidden_size=256, intermediate_size=704))
    else:
        from transformers import Phi3Config
        from transformers.models.phi3.modeling_phi3 import Phi3MLP
        mlp = Phi3MLP(Phi3Config(hidden_size=256, intermediate_size=704))
    mlp = mlp.half()
    quantizers = {}
    for name, lin in find_layers(mlp).items():
        lin.weight.data.mul_(6.0)                                     # pre-activations beyond 1
        gi = torch.from_numpy(O.default_g_idx(lin.in_features, 64))
        s, z = O.minmax_quantize(lin.weight.data.float(), 4, 64, g_idx=gi.numpy())
        quantizers[name] = (None, s.half(), z.half(), gi)
    pack_model(mlp, quantizers, 4, 64)
    return mlp.to(DEV)


@pytest.mark.parametrize("kind", ["gemma2", "phi3"])
def test_injected_mlp_modules(kind):
    """inject_fused_llama on the host model's own MLP module: the injected forward against the module's own composition of the same QuantLinears, state_dict
    untouched; Phi-3's gate_up_proj runs the pair form at decode rows; remove_fused_mlp puts Phi-3 back, bit for bit.
    The forward ends in down's K = 704 matmul, so its outputs carry the bound of test_mlp_forward_one_call (rtol 4e-3 of the value + atol 2e-3 of the output
    scale).  The staged-path bound, rtol (|ref| + 0.05 max|ref|), is the bound of what the activation pass WRITES and is asserted there (Phi-3: the input of
    down_proj); on the outputs behind the matmul the two compositions' roundings of the [M, 704] activations add up over 704 terms to ~6e-4 of the output's rms,
    above that bound's floor of 2e-4 of the maximum for outputs near zero -- measured: 2 of 1024 (Gemma-2) and 9 of 1024 (Phi-3) outputs at 4 rows, worst
    difference 3.9e-3 on a scale of 7."""
    mlp = _quantised_mlp(kind, 11)
    for m in mlp.modules():
        if isinstance(m, QuantLinear):
            m.post_init()
    sd = {k: v.clone() for k, v in mlp.state_dict().items()}
    xs = {M: _x(M, 256, torch.float16, 300 + M) for M in (1, 4, 40)}
    seen = []                                                         # what down_proj reads: act(gate) * up, [M, 704]
    hook = mlp.down_proj.register_forward_pre_hook(lambda m, a: seen.append(a[0].detach().clone()))
    with torch.no_grad():
        plain = {M: mlp(x) for M, x in xs.items()}
    plain_h = dict(zip(xs, seen))
    hook.remove()
    assert inject_fused_llama(mlp) == 1
    if kind == "phi3":
        assert mlp.gate_up_proj.epilogue == "silu_mul" and mlp.gate_up_proj._layer is not None
        assert str(_lib.describe_plan(mlp.gate_up_proj._layer, 1)["pair"]) == "1"
    else:
        assert isinstance(mlp.__dict__["fused_mlp"], FusedGateUpMLP) and mlp.__dict__["fused_mlp"].act == "gelu_tanh"
    for M, x in xs.items():
        with torch.no_grad():
            y, y2 = mlp(x), mlp(x)
        assert y.shape == plain[M].shape and torch.equal(y, y2)
        ref = plain[M].double()
        rtol, atol = MLP_TOL[torch.float16]
        bad = (y.double() - ref).abs() > rtol * ref.abs() + atol * float(ref.abs().max())
        print(f"{kind} M={M}: worst |y - ref| {float((y.double() - ref).abs().max()):.3e} on scale {float(ref.abs().max()):.3e}; "
              f"{int(_staged_bad(y, ref, torch.float16).sum())}/{bad.numel()} outside the staged-path bound, {int(bad.sum())} outside the MLP bound")
        assert not bool(bad.any()), (kind, M, int(bad.sum()))
    if kind == "phi3":                                                # ... and what it hands down_proj against what the module's own chunk / act / mul handed it
        with torch.no_grad():
            for M, x in xs.items():
                assert not bool(_staged_bad(mlp.gate_up_proj(x), plain_h[M].double(), torch.float16).any()), M
    if kind == "gemma2":                                              # the injected forward is the GeGLU, not the SiLU, MLP
        with torch.no_grad():
            s = mlp.down_proj(F.silu(mlp.gate_proj(xs[40])) * mlp.up_proj(xs[40]))
        assert bool(_staged_bad(mlp(xs[40]), s.double(), torch.float16).any())
    assert set(mlp.state_dict()) == set(sd) and all(torch.equal(v, sd[k]) for k, v in mlp.state_dict().items())
    if kind == "phi3":
        assert remove_fused_mlp(mlp) == 1 and mlp.gate_up_proj.epilogue == "none"
        with torch.no_grad():
            assert all(torch.equal(mlp(x), plain[M]) for M, x in xs.items())


def test_tiny_gemma_decode_step_as_one_hipgraph():
    """A quantised tiny Gemma through autogptq_post_init + inject_fused_llama (q|k|v and the GeGLU MLP as gptq_mlp_forward_act) + capture_decode_step: the
    replayed graph gives the bits of the same step run eagerly; the injected model's logits stay with the uninjected model's."""
    import _tiny_gemma as TG
    from transformers import StaticCache
    from autogptq_amd.model_utils import autogptq_post_init, capture_decode_step

    qm_ = TG.fresh_model(3)
    TG.quantize_and_pack(qm_, False)
    qm_ = qm_.to(DEV)
    ids = torch.randint(0, 512, (1, 9), generator=torch.Generator().manual_seed(7)).to(DEV)
    qm_ = autogptq_post_init(qm_, use_act_order=False, max_input_length=64)
    with torch.no_grad():
        base = qm_(ids).logits.float()
    n = inject_fused_llama(qm_)
    assert n == 2 * 2                                                 # attention and MLP of both blocks
    assert all(m.__dict__["fused_mlp"].act == "gelu_tanh" for m in qm_.modules() if type(m).__name__ == "GemmaMLP")
    qm_.set_attn_implementation("sdpa")
    with torch.no_grad():
        fused = qm_(ids).logits.float()
        assert float((fused - base).abs().max()) <= 2e-2 * float(base.abs().max())
        cache = StaticCache(qm_.config, max_cache_len=32)
        logits = qm_(ids, past_key_values=cache, use_cache=True).logits
        step = capture_decode_step(qm_, cache)
        tok = logits[:, -1].argmax(-1)
        lg = step(tok.view(1, 1)).clone()
        c2 = StaticCache(qm_.config, max_cache_len=32)
        qm_(ids, past_key_values=c2, use_cache=True)
        le = qm_(tok.view(1, 1), past_key_values=c2, use_cache=True).logits
    assert torch.equal(lg, le), float((lg.float() - le.float()).abs().max())


# ---- 6. gradient -----------------------------------------------------------------------------------------------------------------------------------------
def test_geglu_layer_under_grad():
    """x.grad of a 'gelu_tanh_mul' layer (composed from its plain product and F.gelu(approximate='tanh'), dX through gptq_grad_input) against the fp64 gradient
    of the reference expression; the bound of test_gpu_grad_input.py::test_silu_mul_layer (relative Frobenius error 4e-3)."""
    M, K, N = 3, 256, 128
    I = N // 2
    Lg, Lu, Wg, Wu = _gate_up(K, I, 64, 4, torch.float16)
    q = fuse_gate_up(_module(Lg, 4, 64, torch.float16), _module(Lu, 4, 64, torch.float16), act="gelu_tanh").to(DEV)
    q.post_init()
    x = _x(M, K, torch.float16, 42).requires_grad_(True)
    dy = torch.randn(M, I, generator=torch.Generator().manual_seed(43)).half().to(DEV)
    y = q(x)
    y.backward(dy)
    x64 = x.detach().double().requires_grad_(True)
    ref = gelu_tanh(x64 @ Wg[0] + Wg[1]) * (x64 @ Wu[0] + Wu[1])
    ref.backward(dy.double())
    rel = float((x.grad.double() - x64.grad).norm() / x64.grad.norm())
    print(f"gelu_tanh_mul under grad: relative error of x.grad {rel:.3e}")
    assert rel <= 4e-3, rel
    with torch.no_grad():
        y0 = q(x)
    assert float((y.detach().double() - y0.double()).norm() / y0.double().norm()) <= 4e-3
    assert float((x64.detach() @ Wg[0] + Wg[1]).abs().max()) > 1.0
