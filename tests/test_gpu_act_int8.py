"""GPU (-m gpu): the opt-in int8-activation path (csrc/act_int8.hip, gptq_forward_a8).  Integer accumulation is exact, so the bounds are derived: with
I_g = sum_{k in g} xq (q - z) and y = sx sum_g s_g I_g + b in fp64,  |out - y| <= ulp_T(|y|) / 2 + (G + 16) 2^-24 (sx sum_g |s_g I_g| + |b|); against the
unquantised x W + b the same plus (sx / 2) sum_k |W[k][n]|.  N = 16 / 48 / 144 are legal for the decode copy (strips of 16 columns) but not for a checkpoint
(N % 32): those layers go to the C ABI as the oracle's restatement of the copy; the switch itself is tested through QuantLinear."""
import ctypes

import numpy as np
import pytest
import torch

from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear, forward_multi, unpack_act_int8_workspace
from autogptq_amd.tensor_parallel import ColumnParallelQuantLinear
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(K, N, M, gs, act, zero_mode, bias, dtype):
    """The one reference: a 4-bit layer as gptq_forward_a8 reads it (decode copy, perm, bias; random packed words as O.random_quant_layer draws them), x with an
    all-zero row and the dtype's largest finite value, the library's own xq / sx read back from its workspace, and the two derived bounds on every output."""
    gen = torch.Generator().manual_seed(K + 7 * N + M)
    g = K if gs == -1 else gs
    G = K // g
    qweight = torch.randint(-2**31, 2**31 - 1, (K // 8, N), dtype=torch.int64, generator=gen).to(torch.int32)
    qzeros = torch.randint(-2**31, 2**31 - 1, (G, N // 8), dtype=torch.int64, generator=gen).to(torch.int32)
    s16 = (0.002 * (1 + 0.1 * torch.rand(G, N, generator=gen))).to(dtype)
    b16 = (0.1 * torch.randn(N, generator=gen)).to(dtype) if bias else None
    g_idx = torch.from_numpy(O.default_g_idx(K, g)).long()
    qw = O.unpack_weights(qweight, 4).astype(np.int64)            # [K, N]
    rows, perm = qweight, None
    if act:                                                       # random g_idx; the copy is made of the re-sequenced rows, the kernel reads x through perm
        g_idx = g_idx[torch.randperm(K, generator=gen)]
        perm = torch.from_numpy(O.sequential_permutation(g_idx)).to(DEV)
        rows = torch.from_numpy(O.pack_rows(qw[perm.cpu().numpy()], 4))
    tiled, consts = O.decode_copy_weights(rows, 4).to(DEV), O.decode_copy_consts(qzeros, s16, zero_mode, 4).to(DEV)
    bdev, gdev = (b16.to(DEV) if bias else None), g_idx.int().to(DEV)
    L = _lib.GptqLayer()
    L.qweight_tiled, L.qconst_tiled, L.tiled_cols = tiled.data_ptr(), consts.data_ptr(), _lib.STRIP_COLS
    L.perm, L.bias, L.g_idx = _lib.ptr(perm), _lib.ptr(bdev), gdev.data_ptr() if act else None
    L.K, L.N, L.bits, L.group_size, L.dtype = K, N, 4, g, _lib.DTYPE_ENUM[dtype]
    x = (torch.rand(M, K, generator=gen) - 0.5).to(dtype)
    if M > 1:
        x[M // 2] = 0
    x[-1, K // 3] = torch.finfo(dtype).max
    lib = _lib.load()
    need = lib.gptq_act_int8_workspace_bytes(ctypes.byref(L), M)
    ws, xd = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV), x.to(DEV)
    out = torch.full((M, N), float("nan"), dtype=dtype, device=DEV)
    _lib.check(lib.gptq_forward_a8(ctypes.byref(L), xd.data_ptr(), out.data_ptr(), M, ws.data_ptr(), need, _lib.current_stream_handle(DEV)))
    torch.cuda.synchronize()
    xq, sx = (t.cpu() for t in unpack_act_int8_workspace(ws, M, K, g, perm))      # the library's own, natural k order
    xf = x.float()                                                                # ... and they are the documented formula, bit for bit
    assert torch.equal(sx, xf.abs().amax(dim=1) / 127.0)
    assert torch.equal(xq, torch.where(sx[:, None] == 0, torch.zeros_like(xf), torch.round(xf / sx[:, None])).to(torch.int8))
    z = torch.from_numpy(O.unpack_zeros(qzeros, 4, zero_mode).astype(np.int64))   # [G, N] as used
    qw, s, b = torch.from_numpy(qw), s16.double(), (b16.double() if bias else torch.zeros(N, dtype=torch.float64))
    y, mag = torch.zeros(M, N, dtype=torch.float64), torch.zeros(M, N, dtype=torch.float64)
    for gi in range(G):
        ks = g_idx == gi
        term = s[gi] * (xq[:, ks].long() @ (qw[ks] - z[gi])).double()             # s_g I_g, I_g an exact integer
        y, mag = y + term, mag + term.abs()
    sxd = sx.double()[:, None]
    y, mag = sxd * y + b, sxd * mag + b.abs()
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dtype]     # explicit mantissa bits, least normal exponent
    ulp = torch.exp2(torch.floor(torch.log2(y.abs().clamp_min(2.0 ** emin))).clamp_min(emin) - mant)
    bound = ulp / 2 + (G + 16) * 2.0 ** -24 * mag
    err = (out.double().cpu() - y).abs()
    print(f"K={K} N={N} M={M} gs={gs} act={act} {zero_mode} bias={bias} {dtype}: max err/bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (err / bound).max().item()
    W = s[g_idx] * (qw - z[g_idx]).double()                                       # the dequantised weights, exact
    assert bool(((out.double().cpu() - (x.double() @ W + b)).abs() <= bound + sxd / 2 * W.abs().sum(dim=0)).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("gs,act", [(128, False), (32, True)])
def test_quantize_activations_is_the_fp32_formula_bit_for_bit(M, K, dtype, gs, act):
    L = O.random_quant_layer(K, 32, 4, gs, act_order=act, dtype=dtype, seed=3)
    q = QuantLinear(4, gs, K, 32, False, weight_dtype=dtype)
    q.qweight, q.qzeros, q.scales, q.g_idx = L["qweight"], L["qzeros"], L["scales"], L["g_idx"]
    q = q.to(DEV).post_init(act_int8=True, act_int8_min_rows=1)
    x = (torch.rand(M, K, generator=torch.Generator().manual_seed(10 * M + K)) - 0.5).to(dtype)
    if M > 1:
        x[M // 2] = 0                                            # an all-zero row: sx = 0, xq = 0
    x[-1, K // 3] = torch.finfo(dtype).max                       # the dtype's largest finite value
    xq, sx = q.quantize_activations(x.to(DEV))
    xf = x.float()                                               # torch CPU fp32: true division, round to nearest even
    rs = xf.abs().amax(dim=1) / 127.0
    assert torch.equal(sx.cpu(), rs)
    assert torch.equal(xq.cpu(), torch.where(rs[:, None] == 0, torch.zeros_like(xf), torch.round(xf / rs[:, None])).to(torch.int8))


@pytest.mark.parametrize("M", [1, 63, 128, 129])
@pytest.mark.parametrize("N", [16, 48, 144])                      # less than a tile, a partial wave tile, two column tiles with a partial one
@pytest.mark.parametrize("K", [128, 256, 384])                    # one chunk, both LDS buffers, an odd chunk count
def test_gemm_a8_against_fp64_shapes(K, N, M):
    _check(K, N, M, 128, False, O.ZERO_WRAP, True, torch.float16)


SWEEP = [([32, 64, 128, -1][2 * a + b], bool(c), [O.ZERO_WRAP, O.ZERO_NOWRAP][a ^ c], bool(b ^ c), [torch.float16, torch.bfloat16][a ^ b ^ c])
         for a in (0, 1) for b in (0, 1) for c in (0, 1)]      # group size x act-order x zero mode x bias x dtype: every pair of levels once (orthogonal array)


@pytest.mark.parametrize("gs,act,zero_mode,bias,dtype", SWEEP)
def test_gemm_a8_against_fp64_sweep(gs, act, zero_mode, bias, dtype):
    _check(384, 144, 129, gs, act, zero_mode, bias, dtype)


def test_selection_reproducibility_and_graph_replay():
    K, N = 256, 128
    L = O.random_quant_layer(K, N, 4, 128, seed=5, bias=True)

    def layer(**kw):
        q = QuantLinear(4, 128, K, N, True)
        q.qweight, q.qzeros, q.scales, q.g_idx, q.bias = L["qweight"], L["qzeros"], L["scales"], L["g_idx"], L["bias"]
        return q.to(DEV).post_init(**kw)

    plain, off, flagged, always = layer(), layer(act_int8=False), layer(act_int8=True), layer(act_int8=True, act_int8_min_rows=1)
    rnd = lambda M, seed: (torch.rand(M, K, generator=torch.Generator().manual_seed(seed)) - 0.5).half().to(DEV)  # noqa: E731
    x5, x64, x128 = rnd(5, 0), rnd(64, 1), rnd(128, 2)
    with torch.no_grad():
        # flag off = flag absent: no int8 rows, the same plans, the same bits, the same row counts handed to the C++ fast path
        assert plain._a8_rows == off._a8_rows == 0 and (flagged._a8_rows, always._a8_rows) == (128, 1)
        for M, x in ((5, x5), (64, x64), (128, x128)):
            assert _lib.describe_plan(off._layer, M) == _lib.describe_plan(plain._layer, M)
            assert torch.equal(off(x), plain(x)) and off._ws0_mask == plain._ws0_mask
        assert torch.equal(flagged(x5), plain(x5)) and torch.equal(flagged(x64), plain(x64))                                   # below the default 128 rows: the 16-bit kernels, bit for bit
        assert flagged._ws0_mask == plain._ws0_mask                                    # the C++ fast path learns the same row counts ...
        y8 = flagged(x128)
        assert torch.equal(y8, always(x128)) and not torch.equal(y8, plain(x128))      # from 128 rows: the int8 path's bits
        assert torch.equal(always(x5), always(x5)) and not torch.equal(always(x5), plain(x5))
        assert torch.equal(flagged(x128), y8)                                          # run to run
        assert always._ws0_mask == 0                                                   # ... and never one the int8 path owns
        # grouped calls and wrapped layers keep the 16-bit kernels
        assert all(torch.equal(a, b) for a, b in zip(forward_multi([always, flagged], x128), forward_multi([plain, off], x128)))
        shard = layer(act_int8=True, act_int8_min_rows=1)
        tp = ColumnParallelQuantLinear(shard, N)
        assert torch.equal(tp(x128), plain(x128)) and torch.equal(shard.post_init(act_int8=True, act_int8_min_rows=1)(x128), plain(x128))
    with torch.enable_grad():
        xg = x128.clone().requires_grad_(True)
        assert torch.equal(flagged(xg).detach(), plain(x128))                          # a call that records an autograd node: the existing path
    xs = x128.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        flagged(xs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.no_grad(), torch.cuda.graph(g, stream=s):      # the stream whose scratch the warm-up call reserved: nothing is allocated for it
        yg = flagged(xs)
    torch.cuda.current_stream().wait_stream(s)
    for r in range(3):
        xn = rnd(128, 20 + r)
        xs.copy_(xn)
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            assert torch.equal(yg, always(xn)), r
