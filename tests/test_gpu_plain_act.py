"""GPU: the ungated epilogues 'relu' / 'gelu' / 'gelu_tanh' -- act(x @ W + b), [M, N], rounded once.  Decode rows (1 - 4) of a plain 3- / 4- / 8-bit fp16 / bf16
layer with its decode copy run the PAIR form of gemv_tiled_kernel in split mode (two stores in place of the gated product: one launch); every other call runs the
layer without its epilogue into `out` and then silu_mul_kernel's in-place mode on it.

Bound per output, against the fp64 value a64 = act64(s64), s64 = x @ W64 + b:

    d = Lip * B_s + eps_act,      bound = (1/2 + 1/64) ulp_T(|a64| + d) + d

Lip = 1 (ReLU) / 1.13 (both GELUs: the slope maximum test_gpu_gated_act.py quotes).  B_s is the project's bound on the pre-activation (_error_model): the fused
form never rounds s, B_s = 4 sqrt(K) 2^-24 A with A = |x| @ |W|; the separate path rounds s to T (the y the pass reads), B_s = _error_model.bound() of the inner
plan.  eps_act = C_ACT[act] 2^-23 |s64| is the activation's own fp32 arithmetic (erff / __expf, two or three products): 0 for ReLU, and for the GELUs measured
by test_the_activation_alone below -- twice the worst error found there, rounded up.  Every case also requires the output to FAIL the same check against another
activation (an ignored argument would otherwise pass wherever the pre-activations are small)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import _error_model as EM
import _guarded as G
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = {"relu": torch.relu, "gelu": F.gelu, "gelu_tanh": lambda s: F.gelu(s, approximate="tanh")}
LIP = {"relu": 1.0, "gelu": 1.13, "gelu_tanh": 1.13}
# test_the_activation_alone, measured on MI355X: worst |err| / (2^-23 |g|) over 4096 g in [-12, 12] = 0.899 ('gelu') and 0.946 ('gelu_tanh') -> ceil(2 x) = 2 and 2
C_ACT = {"relu": 0, "gelu": 2, "gelu_tanh": 2}
SHAPES = [(160, 64, 32, 4), (1024, 1408, 128, 4), (2112, 192, 64, 4), (1024, 2816, 32, 3), (1024, 2816, 32, 8)]
IDS = ["tiny", "1024x1408", "ragged-k", "int3", "int8"]
# where the fp64 references of 'gelu' and 'gelu_tanh', rounded to T, already lie apart by more than the bound (counted on the CPU with C_ACT = 16: 19 / 186
# outputs at 1 / 4 rows of 1024x1408, int3 81 / 490, int8 136 / 410; the tiny and the ragged shape and all of bf16 separate none)
GELUS_APART = {(1024, 1408, 128, 4), (1024, 2816, 32, 3), (1024, 2816, 32, 8)}


@functools.lru_cache(maxsize=None)
def _layer(K, N, gs, bits, dtype, act_order=False, bias=True, device=DEV):
    """The oracle's random layer (scales scaled as test_gpu_gated_act._gate_up scales them: pre-activations beyond 1, where the three activations differ),
    its fp64 weights, |W| of the error model and the bias -- built once per shape, never modified."""
    L = O.random_quant_layer(K, N, bits, gs, dtype=dtype, seed=K + N, bias=True, act_order=act_order)
    L["scales"] = (L["scales"].float() * (8 if K < 2048 else 4) / (16 if bits == 8 else 1)).to(dtype)
    if not bias:
        L["bias"] = None
    W64 = EM.w64(L, bits, O.reference_zero_mode(act_order, bits), device)      # = the module's zero_mode='auto'
    b64 = L["bias"].to(device).double() if bias else torch.zeros(N, dtype=torch.float64, device=device)
    return L, W64, EM.abs_weights(L, bits, dtype, W64), b64


def _module(L, bits, gs, dtype, epilogue, copy=None):
    K, N = L["qweight"].shape[0] * 32 // bits, L["qweight"].shape[1]
    q = QuantLinear(bits, gs, K, N, L["bias"] is not None, weight_dtype=dtype, epilogue=epilogue)
    q.qweight, q.qzeros, q.scales, q.g_idx = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone()
    if L["bias"] is not None:
        q.bias = L["bias"].clone()
    q = q.to(DEV)
    q.post_init(tiled=copy)
    return q


def _x(M, K, dtype, device=DEV):
    return (torch.rand(M, K, generator=torch.Generator().manual_seed(M)) - 0.5).to(dtype).to(device)


def _pre_bound(plan, x64, s64, W64, Wabs, K, gs, dtype):
    """B_s: the bound on the pre-activation the activation is applied to.  Fused: the fp32 sum itself.  Separate: the inner plan's output, rounded to T."""
    A = x64.abs() @ Wabs
    if plan["epilogue"] == "fused":
        assert plan["kernel"] in EM.DECODE_KERNELS
        return 4.0 * math.sqrt(K) * 2.0 ** -24 * A
    C = EM.constant_for(plan, dtype, -1 if gs >= K else gs)
    return EM.bound(s64, A, K, dtype, C, ((x64, W64),) if EM.rounds_each_weight(plan, dtype) else ())


def _bound(act, s64, Bs, dtype):
    a64 = ACTS[act](s64)
    d = LIP[act] * Bs + C_ACT[act] * 2.0 ** -23 * s64.abs()
    return a64, (0.5 + 1.0 / 64) * EM.ulp(a64.abs() + d, dtype) + d


def _outside(y, act, s64, Bs, dtype):
    a64, bnd = _bound(act, s64, Bs, dtype)
    return (y.double() - a64).abs() > bnd


def _others(act, dtype, shape, fused):
    """The activations the output must NOT pass as."""
    if act == "relu":
        return ["gelu", "gelu_tanh"]
    twin = "gelu_tanh" if act == "gelu" else "gelu"
    return ["relu"] + ([twin] if fused and dtype == torch.float16 and shape in GELUS_APART else [])


def _check(y, act, s64, Bs, dtype, shape, fused, what):
    bad = _outside(y, act, s64, Bs, dtype)
    a64, bnd = _bound(act, s64, Bs, dtype)
    ratio = float(((y.double() - a64).abs() / bnd).max())
    msg = f"{what}: max|s| {float(s64.abs().max()):.2f}, worst err / bound {ratio:.3f}, {int(bad.sum())}/{bad.numel()} outside"
    for o in _others(act, dtype, shape, fused):
        msg += f"; as '{o}': {int(_outside(y, o, s64, Bs, dtype).sum())} outside"
    print(msg)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} outputs outside the bound (worst err / bound {ratio:.3f}), first {torch.nonzero(bad)[0].tolist()}"
    for o in _others(act, dtype, shape, fused):
        assert bool(_outside(y, o, s64, Bs, dtype).any()), f"{what}: the output also passes as '{o}' -- the activation argument is not exercised"


# ---- 0. the activation alone: what C_ACT is ---------------------------------------------------------------------------------------------------------
def test_the_activation_alone():
    """An fp32 layer (it runs the separate pass) with x = 0: its sum is exactly 0, so its output is plain_act(bias[n]) in fp32.  4096 values g evenly over
    [-12, 12] in the bias, against fp64.  Measured on MI355X: worst |err| / (2^-23 |g|) = 0.899 for 'gelu' (erff) and 0.946 for 'gelu_tanh' (__expf), ReLU exact
    (0.000); C_ACT = twice that, rounded up = 2 and 2.  The 'gelu' output must fail as 'gelu_tanh' and the reverse: the two differ by up to 4.7e-4, which fp32
    resolves -- the one place a swapped GELU cannot hide behind the width of fp16 / bf16."""
    K, N = 32, 4096
    L = O.random_quant_layer(K, N, 4, 32, dtype=torch.float32, seed=K + N, bias=True)
    g = torch.linspace(-12, 12, N, dtype=torch.float64).float()
    L["bias"] = g.clone()
    x = torch.zeros(1, K, dtype=torch.float32, device=DEV)
    g64 = g.to(DEV).double()[None]
    zero = torch.zeros_like(g64)
    outs = {}
    for act in ACTS:
        q = _module(L, 4, 32, torch.float32, act)
        plan = _lib.describe_plan(q._layer, 1)
        assert plan["epilogue"] == "separate", plan
        with torch.no_grad():
            y = q(x)
        assert tuple(y.shape) == (1, N) and y.dtype == torch.float32
        outs[act] = y
        err = (y.double() - ACTS[act](g64)).abs()
        worst = float((err / (2.0 ** -23 * g64.abs()).clamp_min(1e-300)).max())
        print(f"plain_act '{act}' alone: worst |err| / (2^-23 |g|) = {worst:.3f} -> C_ACT {math.ceil(2 * worst)} (in use: {C_ACT[act]})")
        assert math.ceil(2 * worst) <= C_ACT[act], (act, worst)
        assert not bool(_outside(y, act, g64, zero, torch.float32).any())
    assert torch.equal(outs["relu"], g.to(DEV).clamp_min(0)[None])
    assert bool(_outside(outs["gelu"], "gelu_tanh", g64, zero, torch.float32).any()) and bool(_outside(outs["gelu_tanh"], "gelu", g64, zero, torch.float32).any())
    assert float((outs["gelu"].double() - outs["gelu_tanh"].double()).abs().max()) > 4e-4


# ---- 1. the fused form ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,N,gs,bits", SHAPES, ids=IDS)
def test_decode_rows_run_the_pair_form_in_split_mode(K, N, gs, bits, dtype, act):
    L, W64, Wabs, b64 = _layer(K, N, gs, bits, dtype)
    q = _module(L, bits, gs, dtype, act)
    assert q._qweight_tiled is not None and q._layer.epilogue == _lib.EPILOGUE_ENUM[act] and q.out_width == N
    before = {k: v.clone() for k, v in q.state_dict().items()}
    smax = 0.0
    for M in (1, 2, 3, 4):
        plan = _lib.describe_plan(q._layer, M)
        assert (plan["kernel"], int(plan["pair"]), plan["epilogue"], int(plan["strips"])) == ("strips", 1, "fused", N // 32), plan
        x = _x(M, K, dtype)
        with torch.no_grad():
            y, y2 = q(x), q(x)
        assert tuple(y.shape) == (M, N) and y.dtype == dtype and torch.equal(y, y2)
        x64 = x.double()
        s64 = x64 @ W64 + b64
        smax = max(smax, float(s64.abs().max()))
        _check(y, act, s64, _pre_bound(plan, x64, s64, W64, Wabs, K, gs, dtype), dtype, (K, N, gs, bits), True, f"fused '{act}' {K}x{N} int{bits} {EM.NAMES[dtype]} M={M}")
    assert smax > 1.0, smax
    for k, v in q.state_dict().items():
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("act", list(ACTS))
def test_fused_form_without_a_bias(act):
    K, N, gs, bits, dtype = 1024, 1408, 128, 4, torch.float16
    L, W64, Wabs, b64 = _layer(K, N, gs, bits, dtype, bias=False)
    q = _module(L, bits, gs, dtype, act)
    assert q.bias is None
    for M in (1, 4):
        plan = _lib.describe_plan(q._layer, M)
        assert plan["epilogue"] == "fused" and int(plan["pair"]) == 1
        x = _x(M, K, dtype)
        with torch.no_grad():
            y = q(x)
        x64 = x.double()
        s64 = x64 @ W64
        _check(y, act, s64, _pre_bound(plan, x64, s64, W64, Wabs, K, gs, dtype), dtype, (K, N, gs, bits), True, f"fused '{act}' no bias M={M}")


# ---- 2. the separate path -------------------------------------------------------------------------------------------------------------------------------
def _separate_case(K, N, gs, bits, dtype, act, M, act_order=False, copy=None, what=""):
    L, W64, Wabs, b64 = _layer(K, N, gs, bits, dtype, act_order)
    q = _module(L, bits, gs, dtype, act, copy)
    plan = _lib.describe_plan(q._layer, M)
    assert plan["epilogue"] == "separate" and int(plan.get("pair", 0)) == 0, plan
    p0 = _lib.GptqLayer()
    ctypes.pointer(p0)[0] = q._layer
    p0.epilogue = 0
    inner = _lib.describe_plan(p0, M)
    assert {k: v for k, v in inner.items() if k != "epilogue"} == {k: v for k, v in plan.items() if k != "epilogue"}
    lib = _lib.load()
    assert lib.gptq_workspace_bytes(ctypes.byref(p0), M) == lib.gptq_workspace_bytes(ctypes.byref(q._layer), M)      # in place: nothing staged
    x = _x(M, K, dtype)
    with torch.no_grad():
        y, y2 = q(x), q(x)
    assert tuple(y.shape) == (M, N) and torch.equal(y, y2)
    x64 = x.double()
    s64 = x64 @ W64 + b64
    assert float(s64.abs().max()) > 0.5                       # (2-bit fields are small: 0.94 there; 2.5 - 4 on the 4-bit layers)
    _check(y, act, s64, _pre_bound(plan, x64, s64, W64, Wabs, K, gs, dtype), dtype, (K, N, gs, bits), False,
           f"separate '{act}' {what} {K}x{N} int{bits} M={M} ({plan['path']}/{plan['kernel']})")
    return q


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("M", [5, 8, 40, 130])
def test_more_rows_run_the_pass_in_place(M, act):
    _separate_case(1024, 1408, 128, 4, torch.float16, act, M, what="rows")


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("twin", ["act-order", "int2", "no-copy"])
def test_layers_the_pair_form_does_not_take(twin, act):
    """Two rows of an act-order twin, a 2-bit twin, and the same layer without a decode copy.  (The N = 80 case of the plan: no such layer exists -- widths are
    multiples of 32 in the packed layout; the refusal is pinned by tests/test_plain_act_host.py.)"""
    if twin == "act-order":
        q = _separate_case(1024, 1408, 128, 4, torch.float16, act, 2, act_order=True, what=twin)
        assert q._qweight_tiled is not None                  # the copy of its re-sequenced rows: the inner call is the act-order decode form
    elif twin == "int2":
        q = _separate_case(1024, 1408, 128, 2, torch.float16, act, 2, what=twin)
        assert q._qweight_tiled is not None
    else:
        q = _separate_case(1024, 1408, 128, 4, torch.float16, act, 2, copy=False, what=twin)
        assert q._qweight_tiled is None


# ---- 3. memory ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["relu", "gelu"])
@pytest.mark.parametrize("M", [1, 4, 5])
def test_every_store_stays_inside_out(M, act):
    """x, out [M, N] and the workspace inside guard bands, out's body 0xFF: the fused form (1, 4 rows) stores columns n and n + N/2 with the row stride N --
    the gated form's N/2 stride would leave the upper rows unwritten (NaN), the reverse would run past the end; 5 rows: the pass in place."""
    K, N, gs, bits, dtype = 160, 64, 32, 4, torch.float16
    L, W64, Wabs, b64 = _layer(K, N, gs, bits, dtype)
    q = _module(L, bits, gs, dtype, act)
    lib = _lib.load()
    plan = _lib.describe_plan(q._layer, M)
    assert plan["epilogue"] == ("fused" if M <= 4 else "separate"), plan
    need = int(lib.gptq_workspace_bytes(q._layer_ref, M))
    x = _x(M, K, dtype)
    gx, _ = G.guarded_like(x, G.guard_for(K * 2))
    go = G.Guarded(M * N * 2, G.guard_for(N * 2), 0xFF, G.OUT_GUARD, DEV)
    ws = G.Guarded(need, max(64 << 10, (need + 255) // 256 * 256), 0x00, G.OUT_GUARD, DEV) if need else None
    _lib.check(lib.gptq_forward_ex(q._layer_ref, gx.ptr, go.ptr, M, ws.ptr if ws else None, need, torch.cuda.current_stream(DEV).cuda_stream, None))
    torch.cuda.synchronize()
    what = f"'{act}' {K}x{N} M={M} ({plan['kernel']}, {plan['epilogue']})"
    gx.assert_intact(f"{what}: x")
    go.assert_intact(f"{what}: out")
    if ws:
        ws.assert_intact(f"{what}: workspace")
    y = go.view(dtype, (M, N))
    assert not bool(y.isnan().any()), f"{what}: {int(y.isnan().sum())} outputs left unwritten"
    with torch.no_grad():
        assert torch.equal(y, q(x))


# ---- 4. gated layers through the changed code objects ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["silu_mul", "gelu_tanh_mul"])
def test_gated_layers_keep_their_values(epi):
    """The pair form's product store shares its code objects with the new branch: a 'silu_mul' and a 'gelu_tanh_mul' layer against fp64 within PAIR_TOL of
    test_gpu_gated_act.py (the golden-bits test there stays the authority for SiLU's bits)."""
    import test_gpu_gated_act as GA
    from autogptq_amd.fused import fuse_gate_up
    K, I, gs, bits, dtype = 1024, 704, 128, 4, torch.float16
    Lg, Lu, Wg, Wu = GA._gate_up(K, I, gs, bits, dtype)
    q = fuse_gate_up(GA._module(Lg, bits, gs, dtype), GA._module(Lu, bits, gs, dtype), act="silu" if epi == "silu_mul" else "gelu_tanh").to(DEV)
    q.post_init()
    fn = F.silu if epi == "silu_mul" else GA.gelu_tanh
    for M in (1, 4):
        plan = _lib.describe_plan(q._layer, M)
        assert (int(plan["pair"]), plan["epilogue"]) == (1, "fused")
        x = GA._x(M, K, dtype, M)
        with torch.no_grad():
            y = q(x)
        assert tuple(y.shape) == (M, I)
        ref = fn(GA._pre(x, Wg)) * GA._pre(x, Wu)
        assert not bool(GA._pair_bad(y, ref, dtype).any())


# ---- 5. capture -----------------------------------------------------------------------------------------------------------------------------------------
def test_fused_form_under_graph_capture():
    K, N, gs, bits, dtype = 1024, 1408, 128, 4, torch.float16
    L, _, _, _ = _layer(K, N, gs, bits, dtype)
    q = _module(L, bits, gs, dtype, "gelu")
    assert _lib.describe_plan(q._layer, 1)["epilogue"] == "fused"
    xs = _x(1, K, dtype)
    with torch.no_grad():
        eager = q(xs).clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        q(xs)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            yg = q(xs)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, eager)


# ---- 6. gradient ----------------------------------------------------------------------------------------------------------------------------------------
def test_gelu_layer_under_grad():
    """x.grad of a 'gelu' layer (composed from its plain product and F.gelu, dX through gptq_grad_input) against the fp64 gradient of the reference
    expression: relative Frobenius error 4e-3, the bound of test_geglu_layer_under_grad."""
    M, K, N = 3, 256, 128
    L, W64, _, b64 = _layer(K, N, 64, 4, torch.float16)
    q = _module(L, 4, 64, torch.float16, "gelu")
    x = (torch.rand(M, K, generator=torch.Generator().manual_seed(42)) - 0.5).half().to(DEV).requires_grad_(True)
    dy = torch.randn(M, N, generator=torch.Generator().manual_seed(43)).half().to(DEV)
    y = q(x)
    assert tuple(y.shape) == (M, N)
    y.backward(dy)
    x64 = x.detach().double().requires_grad_(True)
    ref = F.gelu(x64 @ W64 + b64)
    ref.backward(dy.double())
    rel = float((x.grad.double() - x64.grad).norm() / x64.grad.norm())
    print(f"'gelu' under grad: relative error of x.grad {rel:.3e}")
    assert rel <= 4e-3, rel
    with torch.no_grad():
        y0 = q(x)
    assert float((y.detach().double() - y0.double()).norm() / y0.double().norm()) <= 4e-3
    assert float(ref.detach().abs().max()) > 0.5


# ---- 7. whole models ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,want", [("opt", "relu"), ("phi", "gelu_tanh"), ("neox", "gelu")])
def test_tiny_model_with_the_activation_in_fc1(kind, want):
    """A quantised 2-block OPT (ReLU, biases) / Phi (gelu_new) / GPT-NeoX (erf GELU) through autogptq_post_init + inject_fused_act: every first linear plans
    the fused form at one row, the logits stay with the uninjected model's (2e-2 of their maximum, the bound of the tiny-Gemma test), and remove_fused_act
    gives the uninjected model's bits back.  Phi and GPT-NeoX: one decode step captured by capture_decode_step replays to the bits of the same step run eagerly.
    (OPT is not captured: transformers' OPTDecoder.forward builds its attention mask with torch.ones on every call, which the runtime refuses under capture --
    with or without this change.)"""
    import _tiny_opt as TO
    from autogptq_amd.fused import PLAIN_ACT_SITES, inject_fused_act, remove_fused_act
    from autogptq_amd.model_utils import autogptq_post_init
    m = TO.fresh_model(kind, 3)
    TO.quantize_and_pack(m)
    m = m.to(DEV)
    ids = torch.randint(0, 512, (1, 9), generator=torch.Generator().manual_seed(7)).to(DEV)
    m = autogptq_post_init(m, use_act_order=False, max_input_length=64)
    with torch.no_grad():
        base = m(ids).logits.clone()
        base1 = m(ids[:, :1]).logits.clone()
    assert inject_fused_act(m) == 2
    firsts = [getattr(mod, PLAIN_ACT_SITES[type(mod).__name__][0]) for mod in m.modules() if type(mod).__name__ in PLAIN_ACT_SITES]
    assert len(firsts) == 2 and all(isinstance(f, QuantLinear) and f.epilogue == want and f._layer is not None for f in firsts)
    for f in firsts:
        plan = _lib.describe_plan(f._layer, 1)
        assert (plan["kernel"], int(plan["pair"]), plan["epilogue"]) == ("strips", 1, "fused"), plan
    with torch.no_grad():
        fused, fused1 = m(ids).logits, m(ids[:, :1]).logits
    scale = float(base.float().abs().max())
    print(f"tiny {kind}: max |fused - base| {float((fused.float() - base.float()).abs().max()):.3e} (9 rows), "
          f"{float((fused1.float() - base1.float()).abs().max()):.3e} (1 row: the fused form) on scale {scale:.3e}")
    assert float((fused.float() - base.float()).abs().max()) <= 2e-2 * scale
    assert float((fused1.float() - base1.float()).abs().max()) <= 2e-2 * float(base1.float().abs().max())
    if kind != "opt":
        from transformers import StaticCache
        from autogptq_amd.model_utils import capture_decode_step
        m.set_attn_implementation("sdpa")
        with torch.no_grad():
            cache = StaticCache(m.config, max_cache_len=32)
            logits = m(ids, past_key_values=cache, use_cache=True).logits
            step = capture_decode_step(m, cache)
            tok = logits[:, -1].argmax(-1)
            lg = step(tok.view(1, 1)).clone()
            c2 = StaticCache(m.config, max_cache_len=32)
            m(ids, past_key_values=c2, use_cache=True)
            le = m(tok.view(1, 1), past_key_values=c2, use_cache=True).logits
        assert torch.equal(lg, le), float((lg.float() - le.float()).abs().max())
        m.set_attn_implementation("eager")
    assert remove_fused_act(m) == 2 and all(f.epilogue == "none" for f in firsts)
    with torch.no_grad():
        assert torch.equal(m(ids).logits, base) and torch.equal(m(ids[:, :1]).logits, base1)
