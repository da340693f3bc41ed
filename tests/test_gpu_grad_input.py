"""GPU: the input gradient of QuantLinear (gptq_grad_input, csrc/grad_input.hip) and its autograd wiring.

The kernel computes dX = dY . W^T with W = QuantLinear.dequantize() exactly, products and sums in fp32, one rounding at the store.  Against the fp64
product of the same W every output obeys the error model of tests/test_gpu_error_model.py, with the reduction over N:

    |dX - dX64|  <=  (1/2 + 1/64) ulp(dX64)  +  C * sqrt(N) * 2^-24 * A,        A = |dY| @ |W64|^T

C = 16, the model's value for one unbroken matrix-core chain.  fp32 layers (v_mfma_f32_16x16x4_f32) keep C = 16: their worst measured err / bound was
0.05 on this grid, against 0.94 / 0.97 for fp16 / bf16 (profiles/grad_input_gpu_suite.log; the module prints it at the end)."""
import math

import numpy as np
import pytest
import torch

import _tiny_llama as TL
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear, forward_multi, mlp_forward
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 16.0


def _ql(K, N, bits, gs, dtype=torch.float16, act=False, zero_mode="auto", seed=0, bias=False, g_idx=None, release=False, epilogue="none"):
    L = O.random_quant_layer(K, N, bits, gs, dtype=dtype, seed=seed, act_order=act, bias=bias)
    q = QuantLinear(bits, gs, K, N, bias, weight_dtype=dtype, zero_mode=zero_mode, epilogue=epilogue)
    q.qweight, q.qzeros, q.scales = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone()
    q.g_idx = (L["g_idx"] if g_idx is None else g_idx).clone().to(torch.int32)
    if bias:
        q.bias = L["bias"].clone()
    q = q.to(DEV)
    q.post_init(release_checkpoint_layout=release)
    return q


def _ulp(v64, dtype):
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dtype]
    e = torch.floor(torch.log2(v64.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v64.device), e - mant)


def _check(dx, dx64, A, n_red, dtype, partials=()):
    """dx against dx64 within the model; ``partials``: fp64 running sums of earlier accumulate = 1 steps, each rounded once more."""
    bound = (0.5 + 1 / 64) * _ulp(dx64, dtype) + C * math.sqrt(n_red) * 2.0 ** -24 * A
    for p in partials:
        bound = bound + (0.5 + 1 / 64) * _ulp(p, dtype)
    err = (dx.double() - dx64).abs()
    bad = err > bound
    assert not bool(bad.any()), (int(bad.sum()), float((err / bound).max()))
    r = float((err / bound).max())
    WORST[dtype] = max(WORST.get(dtype, 0.0), r)
    return r


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\ngrad_input error model: worst err / bound per dtype:", {str(k): round(v, 3) for k, v in WORST.items()})


def _dense(dy, q):
    W64 = q.dequantize().double()
    dy64 = dy.reshape(-1, dy.shape[-1]).double()
    return dy64 @ W64.t(), dy64.abs() @ W64.abs().t()


def _randn(*shape, dtype=torch.float16, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(DEV)


# ---------------------------------------------------------------- 1. per-output error model
ROWS = (1, 3, 64, 127, 128, 129, 1000)


@pytest.mark.parametrize("KN", [(256, 64), (1024, 512)], ids=["256x64", "1024x512"])
@pytest.mark.parametrize("zero_mode", ["wrap", "nowrap"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_grad_input_error_model_small(bits, dtype, act, zero_mode, KN):
    K, N = KN
    q = _ql(K, N, bits, 32, dtype, act, zero_mode, seed=K + N + bits)
    for M in ROWS:
        dy = _randn(M, N, dtype=dtype, seed=M)
        dx = q.grad_input(dy)
        assert dx.shape == (M, K) and dx.dtype == dtype
        dx64, A = _dense(dy, q)
        _check(dx, dx64, A, N, dtype)


@pytest.mark.parametrize("gs", [32, 128, -1, "nonuniform"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("bits", [3, 4, 8])
def test_grad_input_error_model_groups(bits, dtype, gs):
    K, N = 1024, 512
    g_idx = None
    if gs == "nonuniform":          # groups of unequal sizes in a scrambled order: no re-sequenced copy, every k looks its group up
        gen = torch.Generator().manual_seed(3)
        g_idx = torch.randint(0, K // 128, (K,), generator=gen).to(torch.int32)
        gs = 128
    q = _ql(K, N, bits, gs, dtype, seed=11, g_idx=g_idx)
    for M in (64, 129):
        dy = _randn(M, N, dtype=dtype, seed=M)
        dx64, A = _dense(dy, q)
        _check(q.grad_input(dy), dx64, A, N, dtype)


@pytest.mark.parametrize("KN", [(4096, 11008), (11008, 4096), (5120, 13824)], ids=["4096x11008", "11008x4096", "5120x13824"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_grad_input_error_model_llama_shapes(dtype, act, KN):
    K, N = KN
    q = _ql(K, N, 4, 128, dtype, act, seed=5)
    for M in (512, 2048):
        dy = _randn(M, N, dtype=dtype, seed=M)
        dx64, A = _dense(dy, q)
        _check(q.grad_input(dy), dx64, A, N, dtype)


# ---------------------------------------------------------------- 2. autograd
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
def test_autograd_matches_direct_call_and_dense(dtype, act):
    K, N = 1024, 512
    q = _ql(K, N, 4, 128, dtype, act, bias=True, seed=2)
    x = _randn(3, 43, K, dtype=dtype, seed=1).requires_grad_(True)
    y = q(x)
    assert y.grad_fn is not None and y.shape == (3, 43, N)
    g = _randn(3, 43, N, dtype=dtype, seed=2)
    y.backward(g)
    assert x.grad.dtype == dtype and x.grad.shape == x.shape
    assert torch.equal(x.grad.reshape(-1, K), q.grad_input(g))                   # bit for bit the direct call
    dx64, A = _dense(g, q)
    _check(x.grad.reshape(-1, K), dx64, A, N, dtype)                              # and the dense x @ W + b reference
    with torch.no_grad():
        y0 = q(x)
    assert torch.equal(y.detach(), y0)                                           # forward values under grad: bit-identical
    for name in ("qweight", "qzeros", "scales", "g_idx", "bias"):
        assert getattr(q, name).grad is None                                     # frozen buffers


def test_no_node_without_grad():
    K, N = 1024, 512
    q = _ql(K, N, 4, 128, seed=3)
    x = _randn(8, K, seed=3).requires_grad_(True)
    with torch.no_grad():
        assert q(x).grad_fn is None
    with torch.inference_mode():
        assert q(x).grad_fn is None
    xd = x.detach()
    assert q(xd).grad_fn is None and not q(xd).requires_grad
    for M in (1, 2, 4):                                   # rows the C++ fast path serves once seen: it declines when a node is due
        xs = _randn(M, K, seed=M)
        q(xs)
        q(xs)
        xs.requires_grad_(True)
        ys = q(xs)
        assert ys.grad_fn is not None
        ys.sum().backward()                               # an expanded (stride-0) gradient
        dx64, A = _dense(torch.ones(M, N, dtype=torch.float16, device=DEV), q)
        _check(xs.grad, dx64, A, N, torch.float16)


def test_fp32_input_on_fp16_layer_and_empty_rows():
    K, N = 1024, 512
    q = _ql(K, N, 4, 128, seed=4)
    x = _randn(5, K, dtype=torch.float32, seed=4).requires_grad_(True)
    y = q(x)
    assert y.dtype == torch.float32
    g = _randn(5, N, dtype=torch.float32, seed=5)
    y.backward(g)
    assert x.grad.dtype == torch.float32
    assert torch.equal(x.grad, q.grad_input(g.half()).float())
    x0 = torch.empty(0, K, dtype=torch.float16, device=DEV, requires_grad=True)
    q(x0).sum().backward()
    assert x0.grad.shape == (0, K)


# ---------------------------------------------------------------- 3. fused callers
def test_accumulate():
    K, N = 1024, 512
    q1, q2 = _ql(K, N, 4, 128, seed=6), _ql(K, N, 3, 32, act=True, seed=7)
    d1, d2 = _randn(64, N, seed=1), _randn(64, N, seed=2)
    dx = q1.grad_input(d1)
    p1, A1 = _dense(d1, q1)
    q2.grad_input(d2, dx)
    p2, A2 = _dense(d2, q2)
    _check(dx, p1 + p2, A1 + A2, 2 * N, torch.float16, partials=(p1,))


def test_forward_multi_qkv():
    K = 1024
    layers = [_ql(K, n, 4, 128, act=True, seed=10 + i) for i, n in enumerate((1024, 256, 256))]
    for l in layers:
        l.g_idx.copy_(layers[0].g_idx)
        l._invalidate()
        l.post_init()
    x = _randn(2, 100, K, seed=9).requires_grad_(True)
    outs = forward_multi(layers, x)
    assert len({o.grad_fn for o in outs}) == 1                       # one node
    gs = [_randn(*o.shape, seed=20 + i) for i, o in enumerate(outs)]
    torch.autograd.backward(outs, gs)
    parts = [_dense(g, l) for g, l in zip(gs, layers)]
    run = [parts[0][0], parts[0][0] + parts[1][0]]
    _check(x.grad.reshape(-1, K), sum(p for p, _ in parts), sum(a for _, a in parts), 1536, torch.float16, partials=run)


def test_fused_qkv_g_idx_parts():
    K = 256
    Ls = [O.random_quant_layer(K, K, 4, 64, seed=30 + i, act_order=True) for i in range(3)]
    q = QuantLinear(4, 64, K, 3 * K, False)
    q.qweight = torch.cat([L["qweight"] for L in Ls], 1)
    q.qzeros = torch.cat([L["qzeros"] for L in Ls], 1)
    q.scales = torch.cat([L["scales"] for L in Ls], 1)
    q.g_idx = torch.cat([L["g_idx"] for L in Ls]).to(torch.int32)
    q = q.to(DEV)
    q.post_init()
    assert q._parts is not None
    x = _randn(70, K, seed=31).requires_grad_(True)
    y = q(x)
    g = _randn(70, 3 * K, seed=32)
    y.backward(g)
    full, A = _dense(g, q)
    p = [_dense(g[:, i * K:(i + 1) * K], part)[0] for i, part in enumerate(q._parts)]
    _check(x.grad, full, A, 3 * K, torch.float16, partials=(p[0], p[0] + p[1]))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _close(a, b):
    """Compositions whose forward products may round differently (a fused launch against single ones): dY differs by forward rounding only."""
    assert _rel(a, b) <= 4e-3, _rel(a, b)


def test_silu_mul_layer():
    K, I = 1024, 512
    gate, up = _ql(K, I, 4, 128, seed=40, bias=True), _ql(K, I, 4, 128, seed=41, bias=True)
    from autogptq_amd.fused import fuse_gate_up
    f = fuse_gate_up(gate, up).to(DEV)
    f.post_init()
    x = _randn(96, K, seed=42).requires_grad_(True)
    g = _randn(96, I, seed=43)
    f(x).backward(g)
    xu = x.detach().clone().requires_grad_(True)
    (torch.nn.functional.silu(gate(xu)) * up(xu)).backward(g)
    _close(x.grad, xu.grad)
    with torch.no_grad():
        y0 = f(x)
    _close(f(x).detach(), y0)


def test_mlp_forward_and_fused_gate_up_mlp():
    from autogptq_amd.fused import FusedGateUpMLP
    K, I = 512, 1024
    gate, up, down = _ql(K, I, 4, 128, seed=50), _ql(K, I, 4, 128, seed=51), _ql(I, K, 4, 128, seed=52)
    g = _randn(2, 33, K, seed=53)
    ref_x = _randn(2, 33, K, seed=54).requires_grad_(True)
    down(torch.nn.functional.silu(gate(ref_x)) * up(ref_x)).backward(g)
    x = ref_x.detach().clone().requires_grad_(True)
    mlp_forward(gate, up, down, x).backward(g)
    _close(x.grad, ref_x.grad)
    x2 = ref_x.detach().clone().requires_grad_(True)
    FusedGateUpMLP(gate, up, down)(x2).backward(g)
    _close(x2.grad, ref_x.grad)
    lin = torch.nn.Linear(I, K, bias=False).half().to(DEV)            # non-quantized down: the [gate | up] layer with the fused epilogue
    m = FusedGateUpMLP(gate, up, lin)
    assert m.gate_up is not None
    x3 = ref_x.detach().clone().requires_grad_(True)
    m(x3).backward(g)
    x4 = ref_x.detach().clone().requires_grad_(True)
    lin(torch.nn.functional.silu(gate(x4)) * up(x4)).backward(g)
    _close(x3.grad, x4.grad)


@pytest.mark.parametrize("M", [3, 64, 300])
def test_released_layer_same_gradient(M):
    K, N = 1024, 1024
    a, b = _ql(K, N, 4, 128, seed=60), _ql(K, N, 4, 128, seed=60, release=True)
    assert b._released
    other = _ql(K, N, 4, 128, seed=61, release=True)           # shares the rows scratch
    g = _randn(M, N, seed=62)
    xa = _randn(M, K, seed=63).requires_grad_(True)
    xb = xa.detach().clone().requires_grad_(True)
    a(xa).backward(g)
    yb = b(xb)
    other(xb.detach())
    yb.backward(g)
    assert torch.equal(xa.grad, xb.grad)


# ---------------------------------------------------------------- 4. memory
def test_backward_allocates_no_dense_weight():
    K, N, M = 4096, 11008, 64
    q = _ql(K, N, 4, 128, seed=70)
    x = _randn(M, K, seed=71).requires_grad_(True)
    g = _randn(M, N, seed=72)
    y = q(x)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y.backward(g)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    assert grew <= M * K * 2 + M * N * 2 + 2 ** 20, grew          # a dense K x N copy alone would be 90 MB


# ---------------------------------------------------------------- 5. a training step
class _Adapted(torch.nn.Module):
    """base(x) + B(A(x)): a rank-8 adapter with fp32 master weights beside a (quantized or dense) projection."""

    def __init__(self, base, K, N, seed):
        super().__init__()
        self.base = base
        gen = torch.Generator().manual_seed(seed)
        self.A = torch.nn.Parameter(torch.randn(8, K, generator=gen) / math.sqrt(K))
        self.B = torch.nn.Parameter(torch.randn(N, 8, generator=gen) * 0.05)

    def forward(self, x):
        return self.base(x) + ((x.float() @ self.A.t()) @ self.B.t()).to(x.dtype)


def _adapt(model, names):
    out = {}
    for i, name in enumerate(names):
        parent, attr = name.rsplit(".", 1)
        p = model.get_submodule(parent)
        base = getattr(p, attr)
        K = base.infeatures if isinstance(base, QuantLinear) else base.in_features
        N = base.outfeatures if isinstance(base, QuantLinear) else base.out_features
        ad = _Adapted(base, K, N, seed=100 + i).to(DEV)
        setattr(p, attr, ad)
        out[name] = ad
    return out


def test_lora_style_training_step(tmp_path):
    from autogptq_amd.model_utils import autogptq_post_init
    m = TL.fresh_model(1)
    twin_w = TL.quantize_and_pack(m, False)
    TL.save_checkpoint(m, str(tmp_path), False)
    twin = TL.make_twin({k: v.cpu() for k, v in m.state_dict().items()}, twin_w).to(DEV)
    del m
    qm, _, _ = TL.load_checkpoint(str(tmp_path))
    qm = autogptq_post_init(qm.to(DEV), use_act_order=False, max_input_length=64)
    names = sorted(twin_w)
    for mod in (qm, twin):
        for p in mod.parameters():
            p.requires_grad_(False)
    aq, at = _adapt(qm, names), _adapt(twin, names)
    ids = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(5)).to(DEV)

    def loss_of(model):
        logits = model(ids).logits.float()
        return torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))

    loss_of(qm).backward()
    loss_of(twin).backward()
    for n in names:
        for w in ("A", "B"):
            gq, gt = getattr(aq[n], w).grad, getattr(at[n], w).grad
            assert gq is not None and float(gt.norm()) > 0, (n, w)
            assert _rel(gq, gt) <= 1e-2, (n, w, _rel(gq, gt))
    params = [p for a in aq.values() for p in (a.A, a.B)]
    opt = torch.optim.SGD(params, lr=0.1)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = loss_of(qm)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    losses.append(float(loss_of(qm).detach()))
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0], losses
