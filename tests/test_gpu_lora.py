"""GPU: LoRA adapters on QuantLinear -- the adapter kernels (gptq_lora_down / _up / _apply, csrc/lora.hip), LoraQuantLinear and its autograd wiring, the
model helpers and graph capture (autogptq_amd/lora.py).

Arithmetic contract: u = T(x . A^T) and out = T(out + scale * u . B^T), fp32 products and sums, one rounding each.  Against fp64 every output obeys the
error model of tests/test_gpu_error_model.py, with the reduction over K (down) or r (up):

    |u - u64|      <=  (1/2 + 1/64) ulp(u64)    +  C * sqrt(K) * 2^-24 * (|x| @ |A|^T)
    |out - out64|  <=  (1/2 + 1/64) ulp(out64)  +  C * sqrt(r) * 2^-24 * |scale| * (|u| @ |B|^T)        out64 = y + scale * u @ B^T on the u, y fed in

C = 16, the model's value for one unbroken matrix-core chain.  Both row regimes stay inside it: the 1..8-row forms are fp32 FMA chains of K / 512 * 8 (down)
or r (up) terms plus a 6-level butterfly and 8 partial sums met in LDS, the 9+ row forms are matrix-core chains of K / 256 steps plus the same 8 partial sums --
at most 22 + K / 64 roundings of 2^-24 relative each, which 16 sqrt(K) exceeds for every K >= 32.  The module prints the worst err / bound per dtype and regime at its
end; DESIGN.md section 4.9 records it once measured."""
import ctypes
import math

import pytest
import torch

import _tiny_llama as TL
import autogptq_amd as A
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 16.0
KS = (96, 256, 352)                  # tails of the wave split; 352 = 11 * 32 stands in for 11008
NS = (48, 64, 512)                   # a partial column block
RS = (8, 24, 40, 64)                 # padding to the matrix core's k, the full width
MS = (1, 2, 4, 5, 8, 9, 15, 16, 17, 33, 64, 129)      # both regimes, every partial tile
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nlora error model: worst err / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})


def _ql(K, N, bits, gs, dtype=torch.float16, act=False, seed=0, bias=False):
    L = O.random_quant_layer(K, N, bits, gs, dtype=dtype, seed=seed, act_order=act, bias=bias)
    q = QuantLinear(bits, gs, K, N, bias, weight_dtype=dtype)
    q.qweight, q.qzeros, q.scales = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone()
    q.g_idx = L["g_idx"].clone().to(torch.int32)
    if bias:
        q.bias = L["bias"].clone()
    q = q.to(DEV)
    q.post_init()
    return q


def _ulp(v64, dtype):
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dtype]
    e = torch.floor(torch.log2(v64.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v64.device), e - mant)


def _randn(*shape, dtype=torch.float16, seed=0, mul=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * mul).to(dtype).to(DEV)


def _structs(As, Bs, scales):
    out = []
    for a, b, s in zip(As, Bs, scales):
        L = _lib.GptqLora()
        L.A, L.B = a.data_ptr(), b.data_ptr()
        L.K, L.N, L.r = a.shape[1], b.shape[0], a.shape[0]
        L.dtype, L.scale = _lib.DTYPE_ENUM[a.dtype], s
        out.append(L)
    arr = (ctypes.POINTER(_lib.GptqLora) * len(out))(*[ctypes.pointer(L) for L in out])
    return out, arr


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _down(As, Bs, x):
    keep, arr = _structs(As, Bs, [1.0] * len(As))
    us = [torch.full((x.shape[0], a.shape[0]), float("nan"), dtype=x.dtype, device=DEV) for a in As]
    _lib.check(_lib.load().gptq_lora_down(arr, len(As), x.data_ptr(), _ptrs(us), x.shape[0], _stream()))
    return us


def _up(As, Bs, scales, us, outs):
    keep, arr = _structs(As, Bs, scales)
    _lib.check(_lib.load().gptq_lora_up(arr, len(As), _ptrs(us), _ptrs(outs), us[0].shape[0], _stream()))
    return outs


def _apply(As, Bs, scales, x, outs):
    keep, arr = _structs(As, Bs, scales)
    us = [torch.empty((x.shape[0], a.shape[0]), dtype=x.dtype, device=DEV) for a in As]
    _lib.check(_lib.load().gptq_lora_apply(arr, len(As), x.data_ptr(), _ptrs(us), _ptrs(outs), x.shape[0], _stream()))
    return outs, us


def _down_bound(x, a, dtype):
    """fp64 product and its per-output bound for u = T(x . A^T)."""
    u64 = x.double() @ a.double().t()
    return u64, (0.5 + 1 / 64) * _ulp(u64, dtype) + C * math.sqrt(a.shape[1]) * 2.0 ** -24 * (x.double().abs() @ a.double().abs().t())


def _up_bound(y, u, b, scale, dtype):
    """fp64 value and bound of out = T(y + scale * u . B^T) for the u, y actually fed in; also the adapter term."""
    term = scale * (u.double() @ b.double().t())
    out64 = y.double() + term
    bound = (0.5 + 1 / 64) * _ulp(out64, dtype) + C * math.sqrt(b.shape[1]) * 2.0 ** -24 * abs(scale) * (u.double().abs() @ b.double().abs().t())
    return out64, bound, term


def _assert_within(got, want64, bound, key):
    err = (got.double() - want64).abs()
    ratio = float((err / bound).max())
    print(f"  {key}: worst err / bound {ratio:.3f}")
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= 1.0, (key, ratio, int((err > bound).sum()))


# ---------------------------------------------------------------- 1. down: per-output error model
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_down_error_model(dtype, K):
    dummy_b = torch.zeros(16, 64, dtype=dtype, device=DEV)
    for r in RS:
        a = _randn(r, K, dtype=dtype, seed=K + r, mul=1.0 / math.sqrt(K))
        for M in MS:
            x = _randn(M, K, dtype=dtype, seed=1000 + M)
            (u,) = _down([a], [dummy_b[:, :r].contiguous()], x)
            assert u.shape == (M, r) and not bool(torch.isnan(u).any())
            u64, bound = _down_bound(x, a, dtype)
            _assert_within(u, u64, bound, f"down {IDS[DTYPES.index(dtype)]} {'gemv' if M <= 8 else 'mfma'}")


# ---------------------------------------------------------------- 2. up: per-output error model
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_up_error_model(dtype, N):
    scale = 2.0
    for r in RS:
        b = _randn(N, r, dtype=dtype, seed=N + r, mul=0.05)
        dummy_a = torch.zeros(r, 32, dtype=dtype, device=DEV)
        for M in MS:
            u = _randn(M, r, dtype=dtype, seed=2000 + M)
            y = _randn(M, N, dtype=dtype, seed=3000 + M)
            out64, bound, term = _up_bound(y, u, b, scale, dtype)
            assert float(term.norm()) >= 0.1 * float(y.double().norm())            # a wrong adapter term cannot hide under y's rounding
            (out,) = _up([dummy_a], [b], [scale], [u], [y.clone()])
            _assert_within(out, out64, bound, f"up {IDS[DTYPES.index(dtype)]} {'gemv' if M <= 8 else 'mfma'}")


# ---------------------------------------------------------------- 3. exact identities
def _adapter(q, r, alpha, seed, zero_b=False, **kw):
    lq = A.LoraQuantLinear(q, r, alpha, **kw)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        lq.lora_A.weight.copy_(torch.randn(r, q.infeatures, generator=g) / math.sqrt(q.infeatures))
        if not zero_b:
            lq.lora_B.weight.copy_(torch.randn(q.outfeatures, r, generator=g) * 0.05)
    return lq.eval()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fresh_adapter_and_zero_scale_leave_the_base_output(dtype):
    q = _ql(256, 64, 4, 32, dtype, seed=1, bias=True)
    fresh = A.LoraQuantLinear(q, 24, 16)                                  # B = 0 as constructed
    zero = _adapter(q, 24, 0.0, seed=2)                                   # scale = 0, B random
    assert float(fresh.lora_A.weight.detach().abs().max()) > 0 and not bool(fresh.lora_B.weight.any())
    for M in (1, 4, 8, 9, 64, 129):
        x = _randn(M, 256, dtype=dtype, seed=M)
        with torch.no_grad():
            base = q(x)
            assert torch.equal(fresh(x), base) and torch.equal(zero(x), base), M


def test_two_calls_give_identical_results():
    q = _ql(352, 64, 4, 32, seed=3)          # (a QuantLinear's N is a multiple of 32: the 48-wide partial block is covered by the direct up calls above)
    lq = _adapter(q, 40, 80.0, seed=4)
    for M in (1, 5, 17, 129):
        x = _randn(M, 352, seed=M)
        with torch.no_grad():
            a, b = lq(x), lq(x)
        assert torch.equal(a, b) and not torch.equal(a, q(x)), M


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_multi_apply_equals_single_calls(dtype):
    K = 352
    shapes = ((512, 64), (64, 24), (48, 8))                               # q|k|v-like: (N, r) per adapter
    As = [_randn(r, K, dtype=dtype, seed=10 + i, mul=1 / math.sqrt(K)) for i, (_, r) in enumerate(shapes)]
    Bs = [_randn(N, r, dtype=dtype, seed=20 + i, mul=0.05) for i, (N, r) in enumerate(shapes)]
    scales = [2.0, 0.5, 1.0]
    for M in (1, 5, 8, 9, 33, 129):
        x = _randn(M, K, dtype=dtype, seed=M)
        ys = [_randn(M, N, dtype=dtype, seed=30 + i) for i, (N, _) in enumerate(shapes)]
        multi, mu = _apply(As, Bs, scales, x, [y.clone() for y in ys])
        for i in range(3):
            (single,), (su,) = _apply(As[i:i + 1], Bs[i:i + 1], scales[i:i + 1], x, [ys[i].clone()])
            assert torch.equal(mu[i], su) and torch.equal(multi[i], single), (M, i)
            assert not torch.equal(single, ys[i])


def test_lora_forward_multi_equals_per_layer_calls():
    K = 256
    layers = [_adapter(_ql(K, n, 4, 32, seed=40 + i), r, 2.0 * r, seed=50 + i) for i, (n, r) in enumerate(((512, 64), (64, 8), (64, 24)))]
    for shape in ((1, K), (4, K), (64, K), (2, 9, K)):
        x = _randn(*shape, seed=shape[0])
        with torch.no_grad():
            multi = A.lora_forward_multi(layers, x)
            single = [l(x) for l in layers]
        assert all(torch.equal(m, s) and m.shape == s.shape for m, s in zip(multi, single)), shape


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_values_under_grad_equal_values_under_no_grad(dtype):
    q = _ql(256, 64, 4, 32, dtype, seed=5)
    lq = _adapter(q, 24, 48.0, seed=6)
    for M in (3, 64):
        x = _randn(M, 256, dtype=dtype, seed=M)
        with torch.no_grad():
            y0 = lq(x)
        y1 = lq(x.clone().requires_grad_(True))
        y2 = lq(x)                                                       # only the parameters require grad
        assert y1.grad_fn is not None and y2.grad_fn is not None and y0.grad_fn is None
        assert torch.equal(y1.detach(), y0) and torch.equal(y2.detach(), y0)


# ---------------------------------------------------------------- 4. the module against the fp64 composition
CONFIGS = [(4, 32, False), (4, 32, True), (8, 32, False), (3, 32, False)]


@pytest.mark.parametrize("KN", [(256, 64), (1024, 512)], ids=["256x64", "1024x512"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=["int4", "int4-act", "int8", "int3"])
def test_module_against_the_composition(cfg, KN):
    """Bound: the layer's forward tolerance (__graft_entry__.smoke: 4e-3 * max(1, |ref|max)) for the base term, plus the up bound on the exact u, plus what
    the ONE rounding of u to the layer dtype (and the down kernel's fp32 error: the down bound) can move the output by: |scale| * down_bound @ |B|^T."""
    bits, gs, act = cfg
    K, N = KN
    dtype = torch.float16
    q = _ql(K, N, bits, gs, dtype, act, seed=K + bits, bias=True)
    r, alpha = 24, 48.0
    lq = _adapter(q, r, alpha, seed=7)
    scale = alpha / r
    W64 = q.dequantize().double()
    a16, b16 = lq.lora_A.weight.detach().to(dtype), lq.lora_B.weight.detach().to(dtype)

    def check(x, tag):
        with torch.no_grad():
            y = lq(x)
        xT = x.to(dtype).reshape(-1, K)
        assert y.dtype == x.dtype and y.shape == x.shape[:-1] + (N,)
        base64 = xT.double() @ W64 + q.bias.double()
        u64, dbound = _down_bound(xT, a16, dtype)
        term = scale * (u64 @ b16.double().t())
        ref = base64 + term
        bound = 4e-3 * max(1.0, float(ref.abs().max())) + (0.5 + 1 / 64) * _ulp(ref, dtype) \
            + C * math.sqrt(r) * 2.0 ** -24 * scale * (u64.abs() @ b16.double().abs().t()) + scale * (dbound @ b16.double().abs().t())
        err = (y.double().reshape(-1, N) - ref).abs()
        assert bool((err <= bound).all()), (tag, float((err / bound).max()))
        # and the adapter is really in there: without it the output would be off by the whole term
        assert float((y.double().reshape(-1, N) - base64).norm()) >= 0.5 * float(term.norm()) > 0, tag

    for M in (1, 4, 64):
        check(_randn(M, K, dtype=dtype, seed=M), f"M={M}")
    check(_randn(2, 5, K, dtype=dtype, seed=11), "3-D")
    check(_randn(4, K, dtype=torch.float32, seed=12), "fp32 input")


# ---------------------------------------------------------------- 5. gradients
def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _dense_grads(q, lq, x, g, mask=None, base_mask=None):
    """fp64 autograd of the dense composition on the fp32 master weights; mask / base_mask: a dropout mask (already scaled) on the adapter branch's / the
    base term's input."""
    W64 = q.dequantize().double()
    x64 = x.detach().double().requires_grad_(True)
    a64 = lq.lora_A.weight.detach().double().requires_grad_(True)
    b64 = lq.lora_B.weight.detach().double().requires_grad_(True)
    xl = x64 if mask is None else x64 * mask
    xb = x64 if base_mask is None else x64 * base_mask
    y = xb @ W64 + lq.scaling * ((xl @ a64.t()) @ b64.t())
    y.backward(g.double())
    return x64.grad, a64.grad, b64.grad


@pytest.mark.parametrize("M", [3, 64, 129])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gradients_against_fp64_autograd(dtype, M):
    K, N = 256, 64
    q = _ql(K, N, 4, 32, dtype, seed=8)
    lq = _adapter(q, 24, 48.0, seed=9)
    x = _randn(M, K, dtype=dtype, seed=M).requires_grad_(True)
    g = _randn(M, N, dtype=dtype, seed=100 + M)
    lq(x).backward(g)
    dx, da, db = _dense_grads(q, lq, x, g)
    assert lq.lora_A.weight.grad.dtype == torch.float32 and x.grad.dtype == dtype
    for name, got, want in (("x", x.grad, dx), ("A", lq.lora_A.weight.grad, da), ("B", lq.lora_B.weight.grad, db)):
        assert _rel(got, want) <= 1e-2, (name, _rel(got, want))
    assert all(getattr(q, n).grad is None for n in ("qweight", "qzeros", "scales", "g_idx"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dropout_acts_on_the_adapter_branch_only(dtype):
    K, N, M = 256, 64, 64
    q = _ql(K, N, 4, 32, dtype, seed=12)
    lq = _adapter(q, 24, 48.0, seed=13, lora_dropout=0.5).train()
    x = _randn(M, K, dtype=dtype, seed=14).requires_grad_(True)
    g = _randn(M, N, dtype=dtype, seed=15)
    torch.manual_seed(77)
    y = lq(x)
    y.backward(g)
    torch.manual_seed(77)
    dropped = torch.nn.functional.dropout(x.detach(), 0.5, True)         # the same generator state, shape and dtype: the same mask
    mask = (dropped != 0).double() * 2.0
    assert 0.3 < float((mask != 0).double().mean()) < 0.7
    dx, da, db = _dense_grads(q, lq, x, g, mask)
    for name, got, want in (("x", x.grad, dx), ("A", lq.lora_A.weight.grad, da), ("B", lq.lora_B.weight.grad, db)):
        assert _rel(got, want) <= 1e-2, (name, _rel(got, want))
    assert _rel(x.grad, _dense_grads(q, lq, x, g, mask, mask)[0]) > 1e-2     # the base term saw the UNdropped x: a dropped base input is another gradient ...
    assert _rel(x.grad, _dense_grads(q, lq, x, g)[0]) > 1e-2                 # ... and so is an undropped adapter input
    lq.eval()
    with torch.no_grad():
        assert torch.equal(lq(x), lq(x))                                 # no dropout outside training


def test_tiny_llama_training_step(tmp_path):
    from autogptq_amd.model_utils import autogptq_post_init
    from test_gpu_grad_input import _adapt
    m = TL.fresh_model(1)
    twin_w = TL.quantize_and_pack(m, False)
    TL.save_checkpoint(m, str(tmp_path), False)
    twin = TL.make_twin({k: v.cpu() for k, v in m.state_dict().items()}, twin_w).to(DEV)
    del m
    qm, _, _ = TL.load_checkpoint(str(tmp_path))
    qm = autogptq_post_init(qm.to(DEV), use_act_order=False, max_input_length=64)
    names = sorted(twin_w)
    for p in twin.parameters():
        p.requires_grad_(False)
    at = _adapt(twin, names)                                             # the existing twin: base(x) + B(A(x)), rank 8, fp32 masters
    aq = A.inject_lora(qm, sorted({n.rsplit(".", 1)[1] for n in names}), r=8, lora_alpha=8)
    assert sorted(aq) == names
    A.mark_only_lora_trainable(qm)
    with torch.no_grad():
        for n in names:
            aq[n].lora_A.weight.copy_(at[n].A)
            aq[n].lora_B.weight.copy_(at[n].B)
    ids = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(5)).to(DEV)

    def loss_of(model):
        logits = model(ids).logits.float()
        return torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))

    loss_of(qm).backward()
    loss_of(twin).backward()
    for n in names:
        for w, tw in (("lora_A", "A"), ("lora_B", "B")):
            gq, gt = getattr(aq[n], w).weight.grad, getattr(at[n], tw).grad
            assert gq is not None and float(gt.norm()) > 0, (n, w)
            assert _rel(gq, gt) <= 1e-2, (n, w, _rel(gq, gt))
    params = [p for p in qm.parameters() if p.requires_grad]
    assert len(params) == 2 * len(names)
    opt = torch.optim.SGD(params, lr=0.1)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = loss_of(qm)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    losses.append(float(loss_of(qm).detach()))
    assert len(losses) == 6 and all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses


# ---------------------------------------------------------------- 6. graph capture
def test_decode_step_with_adapters_as_one_graph(tmp_path):
    from transformers import StaticCache
    from autogptq_amd.model_utils import autogptq_post_init, capture_decode_step
    m = TL.fresh_model(2)
    TL.quantize_and_pack(m, False)
    TL.save_checkpoint(m, str(tmp_path), False)
    del m
    qm, _, _ = TL.load_checkpoint(str(tmp_path))
    qm = autogptq_post_init(qm.to(DEV), use_act_order=False, max_input_length=64)
    qm.set_attn_implementation("sdpa")
    targets = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
    layers = A.inject_lora(qm, targets, r=16, lora_alpha=32)
    assert len(layers) == 7 * 2
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for l in layers.values():
            l.lora_B.weight.copy_(torch.randn(l.lora_B.weight.shape, generator=gen) * 0.05)
    qm.eval()
    P, L = 9, 32
    ids = torch.randint(0, 512, (1, P), generator=torch.Generator().manual_seed(7)).to(DEV)
    with torch.no_grad():
        cache, c2 = StaticCache(qm.config, max_cache_len=L), StaticCache(qm.config, max_cache_len=L)
        logits = qm(ids, past_key_values=cache, use_cache=True).logits
        qm(ids, past_key_values=c2, use_cache=True)
        step = capture_decode_step(qm, cache)
        tok = logits[:, -1].argmax(-1)
        lg = step(tok.view(1, 1)).clone()
        le = qm(tok.view(1, 1), past_key_values=c2, use_cache=True).logits
        assert torch.equal(lg, le)                                       # replay == eager, bit for bit
        before = lg.clone()
        for l in layers.values():                                        # an optimiser-style in-place update ...
            l.lora_B.weight.add_(torch.randn(l.lora_B.weight.shape, generator=gen).to(DEV) * 0.05)
        A.refresh_lora(qm)                                               # ... and the documented refresh: no re-capture
        tok = lg[:, -1].argmax(-1)
        lg2 = step(tok.view(1, 1)).clone()
        le2 = qm(tok.view(1, 1), past_key_values=c2, use_cache=True).logits
        assert torch.equal(lg2, le2)
        assert not torch.equal(lg2, before)
