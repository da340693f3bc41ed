"""GPU: the fused LoRA backward -- gptq_lora_backward (csrc/adapter_grad.hip plus lora.hip's kernels on the transposed copies) and the opt-in
``fused_backward`` switch of LoraQuantLinear / lora_forward_multi (autogptq_amd/lora.py).

Arithmetic contract (include/gptq_mi355x.h): du = T(dY . Bt^T) and dX += s du . At^T are gptq_lora_down / gptq_lora_up on the transposed copies, bit for
bit.  dA = s du^T x and dB = s dY^T u are fp32 outputs of wgrad_kernel; against fp64 on the 16-bit operands actually fed (du as produced) every output obeys

    |out - out64|  <=  2^-23 |out64|  +  C * sqrt(M) * 2^-24 * |s| * (|lhs|^T @ |rhs|)          C = 16, one matrix-core chain (tests/test_gpu_error_model.py)

Roundings of the kernel as built, counted as tests/test_gpu_lora.py counts them (one per matrix-core step): an output element is ONE accumulator chain over
the 32-row steps of its slice -- the four waves of a workgroup own different columns, so there is no meeting of waves --, then S - 1 additions of the
slices in wgrad_sum_kernel and one multiplication by s: ceil(M / 32) + S roundings of 2^-24 relative each at most, with S <= min(64, max(1, M / 128)).
That is 2 for M <= 32 (16 sqrt(M) >= 16), 6 at M = 129 (181), 40 at M = 1000 (505) and 160 at M = 4096 (1024): below 16 sqrt(M) for every M tested.  The
2^-23 |out64| term is the rounding of the final product with s and of the fp64 -> fp32 comparison.  The module prints the worst err / bound per dtype at
its end; DESIGN.md section 4.9 records it."""
import ctypes
import math

import pytest
import torch

import _tiny_llama as TL
import autogptq_amd as A
from _guarded import Guarded, guard_for, guarded_like
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 16.0
KS = (96, 256, 352)
NS = (64, 96, 512)
RS = (8, 24, 40, 64)
MS = (1, 5, 8, 9, 31, 32, 33, 64, 129)       # row tails, both regimes of the reused kernels, partial 64-blocks
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nlora backward error model: worst err / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})


def _randn(*shape, dtype=torch.float16, seed=0, mul=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * mul).to(dtype).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lora(K, N, r, dtype, scale, A=0, B=0):
    L = _lib.GptqLora()
    L.A, L.B, L.K, L.N, L.r, L.dtype, L.scale = A, B, K, N, r, _lib.DTYPE_ENUM[dtype], scale
    return L


def _arr(structs, typ):
    return (ctypes.POINTER(typ) * len(structs))(*[ctypes.pointer(s) for s in structs])


def _plan(K, Ns, rs, M, dtype=torch.float16):
    return _lib.describe_lora_backward_plan([_lora(K, N, r, dtype, 1.0) for N, r in zip(Ns, rs)], M)


class Problem:
    """The operands of one call: n adapters that share x [M, K]; adapter i has dY_i [M, N_i], u_i [M, r_i], At_i [K, r_i], Bt_i [r_i, N_i]."""

    def __init__(self, K, Ns, rs, M, dtype, scales, seed=0):
        self.K, self.Ns, self.rs, self.M, self.dtype, self.scales = K, list(Ns), list(rs), M, dtype, list(scales)
        self.x = _randn(M, K, dtype=dtype, seed=seed + 1)
        self.dY = [_randn(M, N, dtype=dtype, seed=seed + 10 + i) for i, N in enumerate(Ns)]
        self.u = [_randn(M, r, dtype=dtype, seed=seed + 20 + i) for i, r in enumerate(rs)]
        self.At = [_randn(K, r, dtype=dtype, seed=seed + 30 + i, mul=1 / math.sqrt(K)) for i, r in enumerate(rs)]
        self.Bt = [_randn(r, N, dtype=dtype, seed=seed + 40 + i, mul=0.05) for i, (N, r) in enumerate(zip(Ns, rs))]

    def pick(self, i):
        p = Problem.__new__(Problem)
        p.K, p.Ns, p.rs, p.M, p.dtype, p.scales = self.K, [self.Ns[i]], [self.rs[i]], self.M, self.dtype, [self.scales[i]]
        p.x, p.dY, p.u, p.At, p.Bt = self.x, [self.dY[i]], [self.u[i]], [self.At[i]], [self.Bt[i]]
        return p

    def loras(self):
        return [_lora(self.K, N, r, self.dtype, s) for N, r, s in zip(self.Ns, self.rs, self.scales)]


def _run(p, dX=None, want_a=True, want_b=True, bufs=None, ws=None):
    """One gptq_lora_backward.  Returns (du, dA, dB) lists; outputs start as NaN so an unwritten element shows.  bufs: {name: [tensor per adapter]} to
    write into instead (guarded buffers)."""
    lib = _lib.load()
    n = len(p.Ns)
    nan = float("nan")
    bufs = bufs or {}
    du = bufs.get("du") or [torch.full((p.M, r), nan, dtype=p.dtype, device=DEV) for r in p.rs]
    dA = bufs.get("dA") or [torch.full((r, p.K), nan, dtype=torch.float32, device=DEV) for r in p.rs]
    dB = bufs.get("dB") or [torch.full((N, r), nan, dtype=torch.float32, device=DEV) for N, r in zip(p.Ns, p.rs)]
    loras = p.loras()
    grads = []
    for i in range(n):
        G = _lib.GptqLoraGrad()
        G.At, G.Bt, G.u, G.dY, G.du = p.At[i].data_ptr(), p.Bt[i].data_ptr(), p.u[i].data_ptr(), p.dY[i].data_ptr(), du[i].data_ptr()
        G.dA = dA[i].data_ptr() if want_a else None
        G.dB = dB[i].data_ptr() if want_b else None
        grads.append(G)
    la, ga = _arr(loras, _lib.GptqLora), _arr(grads, _lib.GptqLoraGrad)
    need = lib.gptq_lora_backward_workspace_bytes(la, n, p.M)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
        wptr, wbytes = (ws.data_ptr() if need else None), need
    else:
        wptr, wbytes = ws
    _lib.check(lib.gptq_lora_backward(la, ga, n, p.x.data_ptr(), dX.data_ptr() if dX is not None else None, p.M, wptr, wbytes, _stream()))
    return du, dA, dB


def _down(bt, dy):
    """gptq_lora_down with A := Bt [r, N], K := N."""
    r, N = bt.shape
    L = _lora(N, N, r, dy.dtype, 1.0, bt.data_ptr(), bt.data_ptr())
    u = torch.full((dy.shape[0], r), float("nan"), dtype=dy.dtype, device=DEV)
    ptr = (ctypes.c_void_p * 1)(u.data_ptr())
    _lib.check(_lib.load().gptq_lora_down(_arr([L], _lib.GptqLora), 1, dy.data_ptr(), ptr, dy.shape[0], _stream()))
    return u


def _up(at, du, out, scale):
    """gptq_lora_up with B := At [K, r], N := K, in place on out."""
    K, r = at.shape
    L = _lora(K, K, r, du.dtype, scale, at.data_ptr(), at.data_ptr())
    up, op = (ctypes.c_void_p * 1)(du.data_ptr()), (ctypes.c_void_p * 1)(out.data_ptr())
    _lib.check(_lib.load().gptq_lora_up(_arr([L], _lib.GptqLora), 1, up, op, du.shape[0], _stream()))
    return out


def _check_wgrad(got, lhs, rhs, scale, M, key):
    """got [P, Q] fp32 against s * lhs^T @ rhs in fp64, every output."""
    assert got.dtype == torch.float32 and not bool(torch.isnan(got).any()), key
    l64, r64 = lhs.double(), rhs.double()
    want = scale * (l64.t() @ r64)
    bound = 2.0 ** -23 * want.abs() + C * math.sqrt(M) * 2.0 ** -24 * abs(scale) * (l64.abs().t() @ r64.abs())
    err = (got.double() - want).abs()
    ok = err <= bound
    ratio = float((err / bound.clamp_min(1e-300)).max())
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert bool(ok.all()), (key, ratio, int((~ok).sum()))


def _check_problem(p, tag):
    du, dA, dB = _run(p)
    for i in range(len(p.Ns)):
        assert torch.equal(du[i], _down(p.Bt[i], p.dY[i])), (tag, i)
        _check_wgrad(dA[i], du[i], p.x, p.scales[i], p.M, f"dA {tag}")
        _check_wgrad(dB[i], p.dY[i], p.u[i], p.scales[i], p.M, f"dB {tag}")
    return du, dA, dB


# ---------------------------------------------------------------- 1. dA / dB: per-output error model
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wgrad_error_model(dtype, K):
    tag = IDS[DTYPES.index(dtype)]
    for N in NS:
        for r in RS:
            for M in MS:
                assert _plan(K, [N], [r], M, dtype)["S_dA"] == [1]
                _check_problem(Problem(K, [N], [r], M, dtype, [2.0], seed=K + N + r + M), tag)
    print(f"  {tag} K={K}: worst err / bound dA {WORST['dA ' + tag]:.3f}  dB {WORST['dB ' + tag]:.3f}")


SLICED = [(128, 1, 1), (256, 2, 2), (1000, 8, 8), (2100, 14, 14), (4090, 32, 32)]      # M, S of dA (K = 96), S of dB (N = 96)


@pytest.mark.parametrize("M,sa,sb", SLICED)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wgrad_error_model_across_slices(dtype, M, sa, sb):
    """Row counts chosen from the plan: S = 1, S = 2 and S >= 3 with a ragged last slice (1000 = 7 slices of 128 rows + 104; 2100 = 13 slices of 160
    rows + 20; 4090 = 31 slices of 128 + 122)."""
    K, N, r = 96, 96, 24
    pl = _plan(K, [N], [r], M, dtype)
    assert pl["path"] == "lora_backward" and pl["S_dA"] == [sa] and pl["S_dB"] == [sb], pl
    assert pl["launches"] == 3 + (1 if sa > 1 else 0) and (pl["workspace"] > 0) == (sa > 1)
    if sa >= 3:
        steps = -(-M // 32)
        assert M % (32 * -(-steps // sa)) != 0                        # the last slice is short
    _check_problem(Problem(K, [N], [r], M, dtype, [0.5], seed=M), IDS[DTYPES.index(dtype)] + " sliced")
    # a wider shape where the two outputs slice differently
    K2, N2, r2 = 352, 512, 40
    pl2 = _plan(K2, [N2], [r2], M, dtype)
    _check_problem(Problem(K2, [N2], [r2], M, dtype, [0.5], seed=M + 1), IDS[DTYPES.index(dtype)] + " sliced")
    assert pl2["S_dA"][0] >= 1 and pl2["S_dB"][0] >= 1


# ---------------------------------------------------------------- 2. du and dX are the reused kernels, bit for bit
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_du_and_dx_equal_the_direct_calls(dtype):
    for K, N, r in ((96, 64, 8), (352, 96, 40), (256, 512, 64)):
        for M in (1, 8, 9, 33, 129, 256):
            p = Problem(K, [N], [r], M, dtype, [2.0], seed=K + M)
            start = _randn(M, K, dtype=dtype, seed=77 + M)                   # a gradient to add to
            dX = start.clone()
            du, _, _ = _run(p, dX=dX)
            ref_du = _down(p.Bt[0], p.dY[0])
            assert torch.equal(du[0], ref_du), (K, N, r, M)
            assert torch.equal(dX, _up(p.At[0], ref_du, start.clone(), 2.0)), (K, N, r, M)
            assert not torch.equal(dX, start)
            zero = torch.zeros_like(start)
            _run(p, dX=zero)
            assert torch.equal(zero, _up(p.At[0], ref_du, torch.zeros_like(start), 2.0))


# ---------------------------------------------------------------- 3. groups, repeatability, skipped outputs
@pytest.mark.parametrize("M", [5, 33, 129, 1000])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_group_equals_single_calls(dtype, M):
    K = 352
    p = Problem(K, [512, 64, 96], [64, 24, 8], M, dtype, [2.0, 0.5, 1.0], seed=M)
    start = _randn(M, K, dtype=dtype, seed=5)
    dX = start.clone()
    du, dA, dB = _run(p, dX=dX)
    seq = start.clone()
    for i in range(3):
        sdu, sdA, sdB = _run(p.pick(i))
        assert torch.equal(du[i], sdu[0]) and torch.equal(dA[i], sdA[0]) and torch.equal(dB[i], sdB[0]), (M, i)
        _up(p.At[i], sdu[0], seq, p.scales[i])
    assert torch.equal(dX, seq)
    dX2 = start.clone()
    du2, dA2, dB2 = _run(p, dX=dX2)
    assert torch.equal(dX2, dX) and all(torch.equal(a, b) for a, b in zip(du + dA + dB, du2 + dA2 + dB2))
    one = _plan(K, p.Ns, p.rs, M, dtype)
    parts = [_plan(K, [N], [r], M, dtype) for N, r in zip(p.Ns, p.rs)]
    for k in ("wg_down", "wg_wgrad", "wg_sum", "wg_up", "workspace"):
        assert one[k] == sum(q[k] for q in parts), k


def test_null_outputs_are_skipped():
    p = Problem(256, [96], [24], 300, torch.float16, [2.0], seed=3)
    full_du, full_dA, full_dB = _run(p)
    for want_a, want_b in ((False, True), (True, False), (False, False)):
        du, dA, dB = _run(p, want_a=want_a, want_b=want_b)                    # outputs start as NaN: the sentinel
        assert torch.equal(du[0], full_du[0])
        assert torch.equal(dA[0], full_dA[0]) if want_a else bool(torch.isnan(dA[0]).all())
        assert torch.equal(dB[0], full_dB[0]) if want_b else bool(torch.isnan(dB[0]).all())


# ---------------------------------------------------------------- 4. guard bands
@pytest.mark.parametrize("M", [33, 129, 300])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_guard_bands(dtype, M):
    """Inputs in NaN-guarded buffers, outputs and the workspace in guarded buffers, an odd tile (K = 352, N = 96, r = 40): a pad row read from memory instead
    of zero-filled brings a NaN into dA / dB, a stray store damages a guard.  M = 300 adds the sliced path and its workspace."""
    K, N, r = 352, 96, 40
    p = Problem(K, [N], [r], M, dtype, [2.0], seed=M)
    es = p.x.element_size()
    keep = []
    g, p.x = guarded_like(p.x, guard_for(K * es))
    keep.append((g, "x"))
    for name, row in (("dY", N), ("u", r), ("At", r), ("Bt", N)):
        g, v = guarded_like(getattr(p, name)[0], guard_for(row * es))
        keep.append((g, name))
        getattr(p, name)[0] = v
    outs = {}
    for name, shape, dt in (("du", (M, r), dtype), ("dA", (r, K), torch.float32), ("dB", (N, r), torch.float32), ("dX", (M, K), dtype)):
        nbytes = shape[0] * shape[1] * torch.empty(0, dtype=dt).element_size()
        g = Guarded(nbytes, guard_for(nbytes // shape[0]), 0xFF, device=DEV)
        keep.append((g, name))
        outs[name] = g.view(dt, shape)
    outs["dX"].zero_()
    need = _lib.load().gptq_lora_backward_workspace_bytes(_arr(p.loras(), _lib.GptqLora), 1, M)
    assert (need > 0) == (M == 300)
    wg = Guarded(max(need, 256), max(64 << 10, need), 0x00, device=DEV)
    keep.append((wg, "workspace"))
    du, dA, dB = _run(p, dX=outs["dX"], bufs={k: [outs[k]] for k in ("du", "dA", "dB")}, ws=(wg.ptr, need))
    torch.cuda.synchronize()
    for g, name in keep:
        g.assert_intact(name)
    for name in ("du", "dA", "dB", "dX"):
        assert not bool(torch.isnan(outs[name]).any()), name
    _check_wgrad(dA[0], du[0], p.x, 2.0, M, "dA guarded")
    _check_wgrad(dB[0], p.dY[0], p.u[0], 2.0, M, "dB guarded")


# ---------------------------------------------------------------- 5. capture
def test_captured_call_replays_to_the_eager_bits():
    p = Problem(352, [96, 512], [24, 64], 300, torch.float16, [2.0, 0.5], seed=9)
    start = _randn(300, 352, seed=4)
    eager_dX = start.clone()
    e_du, e_dA, e_dB = _run(p, dX=eager_dX)
    torch.cuda.synchronize()
    lib = _lib.load()
    need = lib.gptq_lora_backward_workspace_bytes(_arr(p.loras(), _lib.GptqLora), 2, 300)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    nan = float("nan")
    bufs = {"du": [torch.full((300, r), nan, dtype=p.dtype, device=DEV) for r in p.rs],
            "dA": [torch.full((r, 352), nan, dtype=torch.float32, device=DEV) for r in p.rs],
            "dB": [torch.full((N, r), nan, dtype=torch.float32, device=DEV) for N, r in zip(p.Ns, p.rs)]}
    dX = start.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _run(p, dX=dX, bufs=bufs, ws=(ws.data_ptr(), need))
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        dX.copy_(start)
        for t in bufs["du"] + bufs["dA"] + bufs["dB"]:
            t.fill_(nan)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dX, eager_dX)
        for got, want in zip(bufs["du"] + bufs["dA"] + bufs["dB"], e_du + e_dA + e_dB):
            assert torch.equal(got, want)


# ---------------------------------------------------------------- 6. the module: gradients against fp64 autograd
def _ql(K, N, bits, gs, dtype=torch.float16, seed=0):
    L = O.random_quant_layer(K, N, bits, gs, dtype=dtype, seed=seed, act_order=False, bias=False)
    q = QuantLinear(bits, gs, K, N, False, weight_dtype=dtype)
    q.qweight, q.qzeros, q.scales = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone()
    q.g_idx = L["g_idx"].clone().to(torch.int32)
    q = q.to(DEV)
    q.post_init()
    return q


def _adapter(q, r, alpha, seed, **kw):
    lq = A.LoraQuantLinear(q, r, alpha, **kw)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        lq.lora_A.weight.copy_(torch.randn(r, q.infeatures, generator=g) / math.sqrt(q.infeatures))
        lq.lora_B.weight.copy_(torch.randn(q.outfeatures, r, generator=g) * 0.05)
    return lq.eval()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _dense_grads(q, lq, x, g, mask=None):
    """fp64 autograd of the dense composition on the master weights; mask: a dropout mask (already scaled) on the adapter branch's input."""
    W64 = q.dequantize().double()
    x64 = x.detach().double().requires_grad_(True)
    a64 = lq.lora_A.weight.detach().double().requires_grad_(True)
    b64 = lq.lora_B.weight.detach().double().requires_grad_(True)
    xl = x64 if mask is None else x64 * mask
    y = x64 @ W64 + lq.scaling * ((xl @ a64.t()) @ b64.t())
    y.backward(g.double())
    return x64.grad, a64.grad, b64.grad


def _spy(monkeypatch):
    """Counts the gptq_lora_backward calls the module makes (the entry point must really run: no quiet torch path)."""
    from autogptq_amd import lora as LR
    calls = []
    real = LR._fused_backward

    def wrapped(x2, items, need_x, dx=None):
        res = real(x2, items, need_x, dx)
        calls.append((x2.shape[0], len(items), res is not None))
        return res

    monkeypatch.setattr(LR, "_fused_backward", wrapped)
    return calls


@pytest.mark.parametrize("M", [3, 64, 129, 300])                      # 300 rows: S = 2 for both outputs of this layer
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_module_gradients_against_fp64_autograd(dtype, M, monkeypatch):
    """tests/test_gpu_lora.py::test_gradients_against_fp64_autograd with the switch on, the same 1e-2 rel-norm bound.  The fused path rounds du once to the
    layer dtype; simulated on the CPU with that rounding the reference gave dA / dB <= 2.5e-3 (bf16), 3.2e-4 (fp16) and dX <= 3.5e-3 / 4.4e-4.  Measured
    on the MI355X: dA / dB 2.8e-3 (bf16), 3.0e-4 (fp16), dX 3.8e-3 / 4.5e-4."""
    K, N = 256, 64
    assert (_plan(K, [N], [24], M, dtype)["S_dA"][0] > 1) == (M == 300)
    q = _ql(K, N, 4, 32, dtype, seed=8)
    lq = _adapter(q, 24, 48.0, seed=9, fused_backward=True)
    calls = _spy(monkeypatch)
    x = _randn(M, K, dtype=dtype, seed=M).requires_grad_(True)
    g = _randn(M, N, dtype=dtype, seed=100 + M)
    y = lq(x)
    with torch.no_grad():
        assert torch.equal(y.detach(), lq(x))                            # outputs under grad equal outputs under no_grad
    y.backward(g)
    assert calls == [(M, 1, True)]
    dx, da, db = _dense_grads(q, lq, x, g)
    assert lq.lora_A.weight.grad.dtype == torch.float32 and lq.lora_B.weight.grad.dtype == torch.float32 and x.grad.dtype == dtype
    for name, got, want in (("x", x.grad, dx), ("A", lq.lora_A.weight.grad, da), ("B", lq.lora_B.weight.grad, db)):
        print(f"  {IDS[DTYPES.index(dtype)]} M={M} {name}: rel {_rel(got, want):.2e}")
        assert _rel(got, want) <= 1e-2, (name, _rel(got, want))
    assert all(getattr(q, n).grad is None for n in ("qweight", "qzeros", "scales", "g_idx"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_frozen_masters_frozen_input_master_dtype_and_odd_dy(dtype, monkeypatch):
    K, N, M = 256, 64, 64
    q = _ql(K, N, 4, 32, dtype, seed=8)
    calls = _spy(monkeypatch)
    # frozen B and an x without grad: only dA is asked for
    lq = _adapter(q, 24, 48.0, seed=9, fused_backward=True)
    lq.lora_B.weight.requires_grad_(False)
    x = _randn(M, K, dtype=dtype, seed=1)
    g = _randn(M, N, dtype=dtype, seed=2)
    lq(x).backward(g)
    _, da, _ = _dense_grads(q, lq, x, g)
    assert lq.lora_B.weight.grad is None and _rel(lq.lora_A.weight.grad, da) <= 1e-2
    # frozen A, x with grad
    lq = _adapter(q, 24, 48.0, seed=9, fused_backward=True)
    lq.lora_A.weight.requires_grad_(False)
    x = x.clone().requires_grad_(True)
    lq(x).backward(g)
    dx, _, db = _dense_grads(q, lq, x, g)
    assert lq.lora_A.weight.grad is None and _rel(lq.lora_B.weight.grad, db) <= 1e-2 and _rel(x.grad, dx) <= 1e-2
    # masters in the layer dtype get gradients in their dtype
    lq = _adapter(q, 24, 48.0, seed=9, fused_backward=True, adapter_dtype=dtype)
    x = x.detach().clone().requires_grad_(True)
    lq(x).backward(g)
    dx, da, db = _dense_grads(q, lq, x, g)
    assert lq.lora_A.weight.grad.dtype == dtype and lq.lora_B.weight.grad.dtype == dtype
    assert _rel(lq.lora_A.weight.grad, da) <= 1e-2 and _rel(lq.lora_B.weight.grad, db) <= 1e-2 and _rel(x.grad, dx) <= 1e-2
    # a non-contiguous dY (a transposed view) is copied first
    lq = _adapter(q, 24, 48.0, seed=9, fused_backward=True)
    x = x.detach().clone().requires_grad_(True)
    gt = _randn(N, M, dtype=dtype, seed=3)
    (lq(x).t() * 1.0).backward(gt)
    dx, da, db = _dense_grads(q, lq, x, gt.t())
    assert _rel(lq.lora_A.weight.grad, da) <= 1e-2 and _rel(lq.lora_B.weight.grad, db) <= 1e-2 and _rel(x.grad, dx) <= 1e-2
    assert calls == [(M, 1, True)] * 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dropout_in_training_mode(dtype, monkeypatch):
    """The node sees the dropped x (the mask construction of tests/test_gpu_lora.py::test_dropout_acts_on_the_adapter_branch_only)."""
    K, N, M = 256, 64, 64
    q = _ql(K, N, 4, 32, dtype, seed=12)
    lq = _adapter(q, 24, 48.0, seed=13, lora_dropout=0.5, fused_backward=True).train()
    calls = _spy(monkeypatch)
    x = _randn(M, K, dtype=dtype, seed=14).requires_grad_(True)
    g = _randn(M, N, dtype=dtype, seed=15)
    torch.manual_seed(77)
    lq(x).backward(g)
    torch.manual_seed(77)
    dropped = torch.nn.functional.dropout(x.detach(), 0.5, True)         # the same generator state, shape and dtype: the same mask
    mask = (dropped != 0).double() * 2.0
    assert 0.3 < float((mask != 0).double().mean()) < 0.7
    dx, da, db = _dense_grads(q, lq, x, g, mask)
    for name, got, want in (("x", x.grad, dx), ("A", lq.lora_A.weight.grad, da), ("B", lq.lora_B.weight.grad, db)):
        assert _rel(got, want) <= 1e-2, (name, _rel(got, want))
    assert _rel(x.grad, _dense_grads(q, lq, x, g)[0]) > 1e-2             # an undropped adapter input is another gradient
    assert calls == [(M, 1, True)]


# ---------------------------------------------------------------- 7. the group node
def _group(dtype, flag):
    K = 256
    return [_adapter(_ql(K, n, 4, 32, dtype, seed=40 + i), r, 2.0 * r, seed=50 + i, fused_backward=flag) for i, (n, r) in enumerate(((512, 64), (64, 8), (64, 24)))]


@pytest.mark.parametrize("M", [5, 64, 300])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_group_node(dtype, M, monkeypatch):
    K = 256
    layers = _group(dtype, True)
    calls = _spy(monkeypatch)
    x = _randn(M, K, dtype=dtype, seed=M).requires_grad_(True)
    outs = A.lora_forward_multi(layers, x)
    assert len({id(o.grad_fn) for o in outs}) == 1 and "LoraGroupApply" in type(outs[0].grad_fn).__name__      # ONE adapter node
    with torch.no_grad():
        single = [l(x) for l in layers]
    assert all(torch.equal(o.detach(), s) and o.shape == s.shape for o, s in zip(outs, single))
    gs = [_randn(M, l.out_features, dtype=dtype, seed=70 + i) for i, l in enumerate(layers)]
    torch.autograd.backward(outs, gs)
    assert calls == [(M, 3, True)]                                      # one gptq_lora_backward for the group
    want_dx = 0
    for l, g in zip(layers, gs):
        dx, da, db = _dense_grads(l.base, l, x, g)
        want_dx = want_dx + dx
        assert l.lora_A.weight.grad.dtype == torch.float32
        assert _rel(l.lora_A.weight.grad, da) <= 1e-2 and _rel(l.lora_B.weight.grad, db) <= 1e-2
    assert x.grad.dtype == dtype and _rel(x.grad, want_dx) <= 1e-2


def test_group_of_more_than_four_is_split_and_the_switch_off_keeps_per_layer_nodes(monkeypatch):
    K, M = 256, 33
    dtype = torch.float16
    calls = _spy(monkeypatch)
    six = _group(dtype, True) + _group(dtype, True)
    x = _randn(M, K, dtype=dtype, seed=1).requires_grad_(True)
    outs = A.lora_forward_multi(six, x)
    assert len({id(o.grad_fn) for o in outs}) == 2
    with torch.no_grad():
        assert all(torch.equal(o.detach(), l(x)) for o, l in zip(outs, six))
    gs = [_randn(M, l.out_features, dtype=dtype, seed=70 + i) for i, l in enumerate(six)]
    torch.autograd.backward(outs, gs)
    assert sorted(calls) == [(M, 2, True), (M, 4, True)]
    assert _rel(x.grad, sum(_dense_grads(l.base, l, x, g)[0] for l, g in zip(six, gs))) <= 1e-2
    # off: as today, one _LoraApply node per layer and no gptq_lora_backward
    del calls[:]
    off = _group(dtype, False)
    x2 = x.detach().clone().requires_grad_(True)
    outs = A.lora_forward_multi(off, x2)
    assert len({id(o.grad_fn) for o in outs}) == 3 and all("LoraApplyBackward" in type(o.grad_fn).__name__ for o in outs)
    torch.autograd.backward(outs, gs[:3])
    assert calls == []
    # mixed flags: per-layer nodes too
    off[0].fused_backward = True
    outs = A.lora_forward_multi(off, x2)
    assert len({id(o.grad_fn) for o in outs}) == 3


# ---------------------------------------------------------------- 8. a tiny Llama
def test_tiny_llama_step_with_the_switch_on(tmp_path, monkeypatch):
    from autogptq_amd.model_utils import autogptq_post_init
    m = TL.fresh_model(1)
    TL.quantize_and_pack(m, False)
    TL.save_checkpoint(m, str(tmp_path), False)
    del m
    qm, _, _ = TL.load_checkpoint(str(tmp_path))
    qm = autogptq_post_init(qm.to(DEV), use_act_order=False, max_input_length=64)
    targets = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
    layers = A.inject_lora(qm, targets, r=8, lora_alpha=8)
    A.mark_only_lora_trainable(qm)
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for l in layers.values():
            l.lora_B.weight.copy_(torch.randn(l.lora_B.weight.shape, generator=gen) * 0.05)
    ids = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(5)).to(DEV)

    def loss_of(model):
        logits = model(ids).logits.float()
        return torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))

    params = [p for p in qm.parameters() if p.requires_grad]
    assert len(params) == 2 * len(layers)
    loss_of(qm).backward()                                              # the switch-off step (tests/test_gpu_lora.py checks it against the fp32 twin)
    ref = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    calls = _spy(monkeypatch)
    A.set_lora_fused_backward(qm)
    first = loss_of(qm)
    first.backward()
    assert len(calls) == len(layers) and all(ok for _, _, ok in calls)
    for p, want in zip(params, ref):
        assert float(want.norm()) > 0 and _rel(p.grad, want) <= 1e-2, _rel(p.grad, want)
    torch.optim.SGD(params, lr=0.1).step()
    after = float(loss_of(qm).detach())
    assert math.isfinite(after) and after < float(first.detach()), (float(first.detach()), after)
