"""GPU: the input gradient of 2-, 3- and 8-bit layers on the decode copy (gptq_grad_input_ex with GPTQ_GRAD_ON_COPY | GPTQ_GRAD_COPY_ANY_BITS: the other
weight front-ends of grad_copy_kernel, csrc/grad_input_copy.hip; opt-in through QuantLinear.post_init(grad_on_copy="any_bits")).

Reference and bound: those of tests/test_gpu_grad_copy.py, restated --  dX64 = dy.double() @ q.dequantize().double().T,
    |dX - dX64|  <=  (1/2 + 1/64) ulp_T(dX64)  +  16 * sqrt(N) * 2^-24 * (|dY| @ |W64|^T)        (+ (1/2 + 1/64) ulp_T of a preloaded dX when accumulating)"""
import ctypes
import math

import pytest
import torch

from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
ACT = pytest.mark.parametrize("act", [False, True], ids=["plain", "act"])
BITS = pytest.mark.parametrize("bits", [2, 3, 8])


def _ql(K, N, gs, dtype, act, bits, on_copy="any_bits", release=False, seed=0):
    L = O.random_quant_layer(K, N, bits, gs, dtype=dtype, seed=seed, act_order=act)
    q = QuantLinear(bits, gs, K, N, False, weight_dtype=dtype)
    q.qweight, q.qzeros, q.scales, q.g_idx = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone().to(torch.int32)
    return q.to(DEV).post_init(release_checkpoint_layout=release, grad_on_copy=on_copy)


def _ulp(v64, dtype):
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dtype]
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v64.device), torch.floor(torch.log2(v64.abs().clamp_min(2.0 ** emin))) - mant)


def _check(dx, dy, q, dtype, dx0=None):
    W64, dy64 = q.dequantize().double(), dy.double()
    dx64 = dy64 @ W64.t()
    bound = 16.0 * math.sqrt(dy.shape[1]) * 2.0 ** -24 * (dy64.abs() @ W64.abs().t())
    if dx0 is not None:
        dx64 = dx64 + dx0.double()
        bound = bound + (0.5 + 1 / 64) * _ulp(dx0.double(), dtype)
    bound = bound + (0.5 + 1 / 64) * _ulp(dx64, dtype)
    ratio = float(((dx.double() - dx64).abs() / bound).max())
    print(f"worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


def _randn(*shape, dtype, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


# one tile and a short stage | a partial last tile (8 bits: one chunk inside K) | three k tiles, 2 1/2 stages | the 128-row form and its partial tile (one width)
SHAPES = [(b, K, N, rows) for b in (2, 3, 8) for K, N, rows in ((128, 32, (1, 65)), (160, 32, (65,)), (384, 160, (1, 64, 65, 129)))] + [(8, 16384, 32, (129,))]


@pytest.mark.parametrize("bits,K,N,rows", SHAPES, ids=[f"{b}bit-{K}x{N}" for b, K, N, _ in SHAPES])
@pytest.mark.parametrize("gs", [32, 64, 128, -1])
@ACT
@DTYPES
def test_error_model_at_the_edges(dtype, act, gs, bits, K, N, rows):
    q = _ql(K, N, gs, dtype, act, bits, seed=K + N)
    for M in rows:
        plan = q.describe_grad_plan(M)
        assert plan.startswith("kernel=grad_copy") and f"bm={128 if K == 16384 else 64} " in plan and plan.endswith(f"act={int(q.act_order)} bits={bits}"), plan
        dy = _randn(M, N, dtype=dtype, seed=M)
        dx = q.grad_input(dy)
        _check(dx, dy, q, dtype)
        assert torch.equal(dx, q.grad_input(dy))


@ACT
@DTYPES
@BITS
def test_one_hot_rows_are_exact(bits, dtype, act):
    """The k order of every decoder, the two-run 8-bit slots and perm: row e_n of dY gives column n of the dequantised weight, bit for bit."""
    K, N = 384, 160
    q = _ql(K, N, 64, dtype, act, bits, seed=5)
    cols = [0, 15, 16, N - 1]
    dy = torch.zeros(len(cols), N, dtype=dtype, device=DEV)
    for i, n in enumerate(cols):
        dy[i, n] = 1.0
    dx, W = q.grad_input(dy), q.dequantize()
    for i, n in enumerate(cols):
        assert torch.equal(dx[i], W[:, n]), (i, n)


@ACT
@DTYPES
@BITS
def test_same_bits_as_the_rows_kernel(bits, dtype, act):
    """Both kernels sum n in ascending order in one fp32 chain on the same instruction."""
    K, N, M = 384, 160, 65
    q, p = _ql(K, N, 128, dtype, act, bits, seed=7), _ql(K, N, 128, dtype, act, bits, on_copy=False, seed=7)
    assert p.describe_grad_plan(M) == "kernel=grad_rows reason=flag_off"
    dy = _randn(M, N, dtype=dtype, seed=1)
    assert torch.equal(q.grad_input(dy), p.grad_input(dy))


@DTYPES
@BITS
def test_accumulate_and_guard_band(bits, dtype):
    K, N, M, PAD = 384, 160, 65, 4096
    q = _ql(K, N, 32, dtype, True, bits, seed=13)
    dyb, dxb = torch.full((2 * PAD + M * N,), 7.0, dtype=dtype, device=DEV), torch.full((2 * PAD + M * K,), -3.0, dtype=dtype, device=DEV)
    dy, dx = dyb[PAD:PAD + M * N].view(M, N), dxb[PAD:PAD + M * K].view(M, K)
    dy.copy_(_randn(M, N, dtype=dtype, seed=6))
    dx0 = _randn(M, K, dtype=dtype, seed=7)
    dx.copy_(dx0)
    assert q.describe_grad_plan(M).startswith("kernel=grad_copy") and q.grad_input(dy, dx) is dx
    _check(dx, dy, q, dtype, dx0=dx0)
    for buf, n, v in ((dyb, M * N, 7.0), (dxb, M * K, -3.0)):
        assert bool((buf[:PAD] == v).all()) and bool((buf[PAD + n:] == v).all())


@DTYPES
@BITS
def test_released_layer_runs_on_the_copy_alone(bits, dtype):
    K, N, M = 384, 160, 65
    q, qr = _ql(K, N, 128, dtype, False, bits, seed=9), _ql(K, N, 128, dtype, False, bits, release=True, seed=9)
    assert qr._released and qr.describe_grad_plan(M).startswith("kernel=grad_copy")
    dy = _randn(M, N, dtype=dtype, seed=3)
    want = q.grad_input(dy)
    assert torch.equal(qr.grad_input(dy), want)
    L = _lib.GptqLayer()
    ctypes.pointer(L)[0] = qr._layer
    L.qweight = None
    dx = torch.empty_like(want)
    assert _lib.load().gptq_grad_input_ex(ctypes.byref(L), dy.data_ptr(), dx.data_ptr(), M, 0, 5, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx, want)


@BITS
def test_autograd_reaches_the_copy_and_the_old_flag_keeps_the_rows_kernel(bits):
    K, N, M = 384, 160, 65
    q = _ql(K, N, 128, torch.float16, True, bits, seed=11)
    x, dy = _randn(M, K, dtype=torch.float16, seed=4).requires_grad_(), _randn(M, N, dtype=torch.float16, seed=5)
    q(x).backward(dy)
    assert q.describe_grad_plan(M).endswith(f"bits={bits}") and torch.equal(x.grad, q.grad_input(dy))
    assert _ql(K, N, 128, torch.float16, True, 3, on_copy=True, seed=12).describe_grad_plan(M) == "kernel=grad_rows reason=bits"
