"""CPU (-m "not gpu"): the C-ABI library loads and exports every declared symbol, argument
validation returns the documented status codes before any launch, and the host-side logic
(backend class surface, host pack, act-order permutation) matches the reference fixtures."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import autogptq_amd as A
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear
from oracle import gptq_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_exports_header_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    declared -= {"gptq_status_t", "gptq_dtype_t", "gptq_zero_mode_t", "gptq_layer_t", "gptq_tuning_t"}
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert lib.gptq_abi_version() == _lib.ABI_VERSION


def test_struct_layout_matches_header():
    # 5 pointers, 6 int32, 2 pointers, 2 int32  (include/gptq_mi355x.h: gptq_layer_t)
    assert ctypes.sizeof(_lib.GptqLayer) == 5 * 8 + 6 * 4 + 2 * 8 + 2 * 4 + 2 * 8
    assert _lib.GptqLayer.tiled_cols.offset == 84 and _lib.GptqLayer.qweight_tiled.offset == 88 and _lib.GptqLayer.qconst_tiled.offset == 96
    assert _lib.GptqLayer.epilogue.offset == 80
    assert _lib.GptqLayer.qweight_seq.offset == 64
    assert ctypes.sizeof(_lib.GptqTuning) == 8 * 4


def _layer(**kw):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000  # never dereferenced: validation fails first
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = 256, 256, 4, 128, 0, 0
    for k, v in kw.items():
        setattr(L, k, v)
    return L


@pytest.mark.parametrize("kw,code,frag", [
    (dict(bits=5), 3, "Only 2,3,4,8 bits are supported"),
    (dict(K=100), 2, "multiples of 32"),
    (dict(N=48), 2, "multiples of 32"),
    (dict(group_size=0), 2, "group_size"),
    (dict(dtype=7), 3, "dtype"),
    (dict(qweight=None), 1, "non-NULL"),
    (dict(perm=0x1000), 1, "together"),
])
def test_validation_status_codes(kw, code, frag):
    lib = _lib.load()
    L = _layer(**kw)
    rc = lib.gptq_forward(ctypes.byref(L), 0x1000, 0x1000, 1, None, 0, None)
    assert rc == code
    assert frag in lib.gptq_last_error().decode()
    with pytest.raises(_lib.GptqError) as ei:
        _lib.check(rc)
    assert ei.value.status == code and isinstance(ei.value, RuntimeError)


def test_validation_io_and_workspace_query():
    lib = _lib.load()
    L = _layer()
    assert lib.gptq_forward(ctypes.byref(L), None, 0x1000, 1, None, 0, None) == 1
    assert lib.gptq_forward(ctypes.byref(L), 0x1000, 0x1000, 0, None, 0, None) == 2
    assert lib.gptq_forward(None, 0x1000, 0x1000, 1, None, 0, None) == 1
    # tiny N forces a K split -> needs workspace -> refused without one (no launch happens)
    Ls = _layer(N=32, K=4096)
    need = lib.gptq_workspace_bytes(ctypes.byref(Ls), 1)
    assert need > 0
    assert lib.gptq_gemv(ctypes.byref(Ls), 0x1000, 0x1000, 1, None, 0, None, None) == 4
    assert "workspace too small" in lib.gptq_last_error().decode()
    assert lib.gptq_workspace_bytes(ctypes.byref(_layer(bits=5)), 1) == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_make_sequential_matches_oracle(seed):
    lib = _lib.load()
    rng = np.random.default_rng(seed)
    K, gs = 512, 64
    g = (np.arange(K) // gs).astype(np.int32)[rng.permutation(K)]
    gt = torch.from_numpy(g.copy())
    perm = torch.empty(K, dtype=torch.int32)
    uni = ctypes.c_int(-1)
    assert lib.gptq_make_sequential(gt.data_ptr(), K, gs, perm.data_ptr(), ctypes.byref(uni)) == 0
    assert np.array_equal(perm.numpy(), O.sequential_permutation(g))
    assert uni.value == 1
    # uneven groups -> not uniform
    g2 = g.copy(); g2[:3] = 0
    assert lib.gptq_make_sequential(torch.from_numpy(g2).data_ptr(), K, gs, perm.data_ptr(), ctypes.byref(uni)) == 0
    assert np.array_equal(perm.numpy(), O.sequential_permutation(g2))
    assert uni.value == int(np.array_equal(g2[perm.numpy()], np.arange(K) // gs))
    bad = g.copy(); bad[5] = -1
    assert lib.gptq_make_sequential(torch.from_numpy(bad).data_ptr(), K, gs, perm.data_ptr(), None) == 2


def test_class_surface_matches_reference_contract():
    q = QuantLinear(4, 128, 256, 64, True, use_cuda_fp16=True, trainable=False, weight_dtype=torch.float16,
                    some_unknown_kwarg=1)
    assert q.QUANT_TYPE == "mi355x"
    sd = q.state_dict()
    assert list(sd.keys()) == ["qweight", "qzeros", "scales", "g_idx", "bias"]   # checkpoint ABI
    assert sd["qweight"].shape == (32, 64) and sd["qweight"].dtype == torch.int32
    assert sd["qzeros"].shape == (2, 8) and sd["qzeros"].dtype == torch.int32
    assert sd["scales"].shape == (2, 64) and sd["scales"].dtype == torch.float16
    assert sd["g_idx"].tolist() == [i // 128 for i in range(256)]
    for attr in ("infeatures", "outfeatures", "bits", "group_size", "maxq", "trainable"):
        assert hasattr(q, attr)
    assert QuantLinear(4, -1, 64, 32, False).group_size == 64
    with pytest.raises(NotImplementedError, match="Only 2,3,4,8 bits"):
        QuantLinear(5, 128, 256, 64, False)
    with pytest.raises(NotImplementedError):
        QuantLinear(4, 128, 256, 64, False, trainable=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        q(torch.zeros(1, 256, dtype=torch.float16))
    assert A.dynamically_import_QuantLinear(False, True, 128, 4) is QuantLinear
    with pytest.raises(ValueError):
        A.dynamically_import_QuantLinear(use_triton=True, desc_act=False, group_size=128, bits=4)


@pytest.mark.skipif(torch.cuda.is_available(), reason="host pack path is taken only without a GPU")
def test_host_pack_bit_exact(ref_case):
    c = ref_case
    lin = torch.nn.Linear(c.K, c.N, bias=c.lin_bias is not None)
    lin.weight.data = c.W.to(c.dtype)
    if c.lin_bias is not None:
        lin.bias.data = c.lin_bias.clone()
    q = QuantLinear(c.bits, c.group_size, c.K, c.N, c.lin_bias is not None, weight_dtype=c.dtype)
    q.pack(lin, c.scale.to(c.qparams_dtype), c.zero.to(c.qparams_dtype), c.g_idx.clone())
    assert torch.equal(q.qweight, c.qweight)
    assert torch.equal(q.qzeros, c.qzeros)
    assert torch.equal(q.scales, c.scales)
    assert q.scales.dtype == c.dtype
    if c.bias is not None:
        assert torch.equal(q.bias, c.bias)
    # checkpoint round trip through state_dict
    q2 = QuantLinear(c.bits, c.group_size, c.K, c.N, c.lin_bias is not None, weight_dtype=c.dtype)
    q2.load_state_dict(q.state_dict())
    assert torch.equal(q2.qweight, c.qweight) and torch.equal(q2.g_idx, c.g_idx)


def test_fuse_quant_linears_host_logic():
    """fuse_qkv / fuse_gate_up only concatenate checkpoint tensors (CPU-checkable); the fused forward is in the GPU tests."""
    from autogptq_amd.fused import fuse_gate_up, fuse_qkv

    def mk(N, seed, act=False):
        L = O.random_quant_layer(256, N, 4, 64, act_order=act, seed=seed, bias=True)
        q = QuantLinear(4, 64, 256, N, True)
        q.qweight, q.qzeros, q.scales, q.g_idx, q.bias = L["qweight"], L["qzeros"], L["scales"], L["g_idx"], L["bias"]
        return q
    a, b, c = mk(128, 1), mk(64, 2), mk(64, 3)
    f = fuse_qkv(a, b, c)
    assert f.outfeatures == 256 and f.qweight.shape == (32, 256) and f.qzeros.shape == (4, 32) and f.scales.shape == (4, 256)
    assert torch.equal(f.qweight[:, 128:192], b.qweight) and torch.equal(f.qzeros[:, 16:24], b.qzeros)
    assert torch.equal(f.bias[192:], c.bias) and f.epilogue == "none"
    g = fuse_gate_up(b, c)
    assert g.epilogue == "silu_mul" and g.outfeatures == 128
    with pytest.raises(ValueError, match="g_idx"):
        fuse_qkv(a, mk(64, 4, act=True), c)
    with pytest.raises(ValueError, match="equal width"):
        fuse_gate_up(a, b)
    with pytest.raises(ValueError, match="64"):
        QuantLinear(4, 64, 256, 96, False, epilogue="silu_mul")


def test_make_quant_and_pack_model_host():
    """make_quant / pack_model mirrors (auto_gptq/modeling/_utils.py:69-147, 257-330) on a toy module: modules are swapped for
    the mi355x QuantLinear with the reference's constructor arguments and pack() fills the checkpoint tensors bit-exactly."""
    from autogptq_amd.model_utils import find_layers, make_quant, pack_model

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(64, 32, bias=True)
            self.blk = torch.nn.Sequential(torch.nn.Linear(32, 64, bias=False), torch.nn.ReLU())
            self.head = torch.nn.Linear(64, 32)

    torch.manual_seed(0)
    m = Toy().half()
    names = ["a", "blk.0"]
    quantizers = {}
    for nme in names:
        lin = dict(m.named_modules())[nme]
        s, z = O.minmax_quantize(lin.weight.data.float(), 4, 32)
        quantizers[nme] = (None, s.half(), z.half(), torch.from_numpy(O.default_g_idx(lin.in_features, 32)))
    ref = {nme: O.pack(dict(m.named_modules())[nme].weight.data.clone(), quantizers[nme][1], quantizers[nme][2],
                       quantizers[nme][3], 4, torch.float16) for nme in names}
    pack_model(m, quantizers, 4, 32)
    assert isinstance(m.a, QuantLinear) and isinstance(m.blk[0], QuantLinear) and isinstance(m.head, torch.nn.Linear)
    assert m.a.bias is not None and m.blk[0].bias is None and m.a.infeatures == 64 and m.a.outfeatures == 32
    for nme in names:
        ql = dict(m.named_modules())[nme]
        assert torch.equal(ql.qweight.cpu(), ref[nme][0]) and torch.equal(ql.qzeros.cpu(), ref[nme][1])
        assert torch.equal(ql.scales.cpu(), ref[nme][2])
    assert set(find_layers(m, [QuantLinear])) == set(names)


def test_awq_entry_points_validate_before_touching_memory():
    """gptq_awq_unpack / gptq_awq_repack: argument validation runs on the host (no GPU needed), the Python mirror refuses
    to run without a device (there is no host implementation of the ingest), and the bits != 4 assertion of the
    reference (auto_gptq/modeling/_utils.py:526,572,647) is kept."""
    import torch
    from autogptq_amd import awq
    lib = _lib.load()
    p = 0x1000
    assert lib.gptq_awq_repack(p, p, 100, 64, 32, p, p, None) == 2 and "multiples of 8" in lib.gptq_last_error().decode()
    assert lib.gptq_awq_repack(p, p, 128, 64, 48, p, p, None) == 2 and "group_size" in lib.gptq_last_error().decode()
    assert lib.gptq_awq_repack(None, p, 128, 64, 32, p, p, None) == 1
    assert lib.gptq_awq_unpack(p, p, None, 128, 64, 32, p, p, None) == 1
    assert lib.gptq_awq_unpack(p, p, p, 128, 60, 32, p, p, None) == 2
    with pytest.raises(AssertionError):
        awq.unpack_awq(torch.zeros(8, 1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), torch.ones(1, 8).half(), 8, 8)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no host implementation"):
            awq.repack_awq_to_gptq(torch.zeros(8, 1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), 8)
    t = torch.arange(16, dtype=torch.int8).reshape(16, 1)                     # [N, G] -> transposed inside
    assert awq.awq_reverse_reorder_int_tensor(t, 4).flatten().tolist() == [0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, 10, 14, 11, 15]


@pytest.mark.parametrize("fname", ["marlin_k128_n256_g128.npz", "marlin_k256_n256_g128.npz", "marlin_k512_n512_g128.npz"])
def test_marlin_format_conversion(golden_dir, fname):
    """autogptq_amd.marlin (index arithmetic on whole tensors): Marlin -> GPTQ equals the oracle, GPTQ -> Marlin gives back the
    reference's B and s bit for bit, the permutation tables equal the oracle's, and the guards of the reference's Marlin class
    (shape divisibility, group sizes, symmetric zero-points) raise."""
    import numpy as np
    import torch
    from autogptq_amd import marlin
    from oracle import marlin_oracle as M
    for a, b in zip(marlin.marlin_perms(), M.perms()):
        assert np.array_equal(a.numpy(), b)
    d = np.load(os.path.join(golden_dir, fname))
    gs = int(d["group_size"])
    qw, qz, sc = marlin.marlin_to_gptq(torch.from_numpy(d["B"]), torch.from_numpy(d["s"]), gs)
    eq, ez, es = M.to_gptq(d["B"], d["s"], gs)
    assert qw.dtype == torch.int32 and qz.dtype == torch.int32 and sc.dtype == torch.float16
    assert np.array_equal(qw.numpy(), eq) and np.array_equal(qz.numpy(), ez) and np.array_equal(sc.numpy().view(np.uint16), es.view(np.uint16))
    B2, s2 = marlin.gptq_to_marlin(qw, qz, sc, gs)
    assert np.array_equal(B2.numpy(), d["B"]) and np.array_equal(s2.numpy().view(np.uint16), d["s"].view(np.uint16))
    with pytest.raises(ValueError, match="symmetric"):
        marlin.gptq_to_marlin(qw, qz + 1, sc, gs)
    with pytest.raises(ValueError, match="divisible"):
        marlin.marlin_to_gptq(torch.zeros(4, 512, dtype=torch.int32), torch.zeros(1, 256).half(), 64)
    with pytest.raises(ValueError, match="group_size"):
        marlin.marlin_to_gptq(torch.zeros(16, 512, dtype=torch.int32), torch.zeros(4, 256).half(), 64)


def _plan(K, N, M, *, bits=4, gs=128, dtype=0, act=False, epilogue=0, tuning=None):
    L = _layer(K=K, N=N, bits=bits, group_size=gs, dtype=dtype, epilogue=epilogue)
    if act:
        L.g_idx = L.qweight_seq = L.perm = 0x1000        # re-sequenced act-order layer (never dereferenced by the planner)
    return _lib.describe_plan(L, M, tuning)


def test_dispatch_rules_are_the_measured_ones():
    """gptq_describe_plan (host only): the kernel / geometry gptq_forward_ex picks.  These are the crossovers DESIGN.md §4
    reports measurements for -- pinned here so a planner edit that moves one shows up without a GPU."""
    # decode, Llama-7B shapes: matrix-core GEMV, 16-column strips, one launch
    for K, N in ((4096, 4096), (11008, 4096)):
        p = _plan(K, N, 1)
        assert (p["path"], p["kernel"], p["ln"], p["ksplit"], p["waves"]) == ("gemv", "mfma", 4, 1, 16), p
    assert _plan(4096, 4096, 1)["strips"] == 256
    # 4096 x 11008: the streamed (LDS-DMA) kernel with 64-column strips, one pass of 16 waves x 8 rows (8.2 vs 9.6 us); M = 1..2 only
    p = _plan(4096, 11008, 1)
    assert (p["kernel"], p["ln"], p["waves"], p["u"], p["ksplit"], p["strips"]) == ("stream", 16, 16, 8, 1, 172), p
    assert _plan(4096, 11008, 3)["kernel"] == "stream64" and _plan(4096, 11008, 4)["kernel"] == "stream64"       # 3..4 rows, 160+ strips: batched-decode kernel, unsplit
    assert _plan(11008, 4096, 3)["kernel"] == "mfma" and _plan(4096, 4096, 3)["kernel"] == "mfma"               # (with K slices / small layers: GEMV)
    assert _plan(5120, 13824, 3)["kernel"] == "stream64" and _plan(13824, 5120, 3)["kernel"] == "stream"
    assert _plan(4096, 11008, 1, dtype=1)["kernel"] == "stream"
    # wider plain fp16 layers: 64- / 32-column strips with >= 160 workgroups; bf16 and act-order stay at 16 columns
    assert _plan(4096, 12288, 1)["ln"] == 16 and _plan(4096, 14336, 1)["ln"] == 16
    assert _plan(3584, 8192, 1)["ln"] == 8 and _plan(3584, 8192, 1)["kernel"] == "mfma"
    # K and N >= 5120 (13B / 33B / 70B projections): the streamed kernel, 32-column strips (64 from 16384 columns), 8 waves x 4 rows, M <= 4
    for (k, n), ln in (((5120, 5120), 8), ((13824, 5120), 8), ((8192, 8192), 8), ((5120, 13824), 8), ((8192, 28672), 16), ((28672, 8192), 8)):
        for m in (1, 4):
            p = _plan(k, n, m)
            if m == 4 and n >= 10240:                 # 160+ strips of 64 columns, 3..4 rows: the batched-decode kernel, unsplit
                assert (p["kernel"], p["ksplit"]) == ("stream64", 1), (k, n, m, p)
            else:
                assert (p["kernel"], p["ln"], p["waves"], p["u"], p["ksplit"]) == ("stream", ln, 8, 4, 1), (k, n, m, p)
    assert _plan(5120, 5120, 1, dtype=1)["kernel"] == "stream" and _plan(5120, 5120, 1, act=True)["kernel"] == "mfma"
    assert _plan(8192, 3584, 1)["kernel"] == "mfma" and _plan(8192, 1024, 1)["kernel"] == "mfma"
    assert _plan(4096, 12288, 1, dtype=1)["ln"] == 4 and _plan(4096, 12288, 1, act=True)["ln"] == 4
    assert _plan(4096, 12288, 1, act=True)["perm"] == 1
    # act-order with 2+ rows: x permuted once by a pre-pass (perm = 2), plain kernel on the re-sequenced rows
    p = _plan(4096, 11008, 2, act=True)
    assert (p["path"], p["kernel"], p["perm"]) == ("gemv", "stream", 2), p                               # = the plain layer's kernel at that M
    for m in (3, 4):
        assert _plan(4096, 11008, m, act=True)["kernel"] == "stream64"                                   # (which from 3 rows is the batched-decode kernel)
        p = _plan(11008, 4096, m, act=True)
        assert (p["path"], p["kernel"], p["perm"]) == ("gemv", "mfma", 2), p
    assert _plan(28672, 1024, 8, act=True)["perm"] == 2 and _plan(4096, 4096, 1, act=True, dtype=1)["perm"] == 1
    # one row: in-kernel gather (perm = 1), except from 33 MiB up on layers that stream (pre-pass + streamed kernel) and for K beyond the LDS row
    assert _plan(5120, 5120, 1, act=True)["perm"] == 1 and _plan(4096, 11008, 1, act=True)["perm"] == 1
    p = _plan(13824, 5120, 1, act=True)
    assert (p["kernel"], p["perm"], p["ln"]) == ("stream", 2, 8), p
    assert _plan(8192, 28672, 1, act=True)["kernel"] == "stream" and _plan(28672, 1024, 1, act=True)["perm"] == 2
    # small N: K split (second, fixed-order reduce launch)
    assert _plan(8192, 1024, 1)["ksplit"] > 1
    # fused gate/up epilogue lives in the GEMV for M <= 8, and is a separate elementwise pass behind the GEMM paths
    assert _plan(4096, 22016, 1, epilogue=1)["epilogue"] == "fused" and _plan(4096, 22016, 1, epilogue=1)["pair"] == 1
    assert _plan(4096, 22016, 64, epilogue=1)["epilogue"] == "separate"
    # other packings: matrix-core kernel with field extraction (fp16/bf16), fp32 -> generic
    assert _plan(4096, 4096, 1, bits=3, gs=32)["kernel"] == "mfma_generic" and _plan(4096, 4096, 1, bits=8, gs=32)["kernel"] == "mfma_generic"
    assert _plan(4096, 4096, 1, dtype=2)["kernel"] == "generic"
    # fp32 above 8 rows: exact-f32 matrix core (128 x 128 tiles), any bit width; the GEMV would re-stream the weights per 4 rows
    assert _plan(4096, 4096, 2048, dtype=2)["kernel"] == "f32_mfma" and _plan(4096, 11008, 65, dtype=2, bits=3, gs=32)["kernel"] == "f32_mfma"
    assert _plan(4096, 4096, 64, dtype=2)["path"] == "gemv"          # 32 tiles: the 4-rows-per-pass GEMV is faster
    assert _plan(4096, 4096, 8, dtype=2)["path"] == "gemv"
    # ... and up to 64 rows everywhere (4096 x 11008 M = 8: 517 us on the fp32 GEMM, 48 on the GEMV), beyond that from 64 tiles up
    assert _plan(4096, 11008, 8, dtype=2)["path"] == "gemv" and _plan(4096, 11008, 64, dtype=2)["path"] == "gemv"
    assert _plan(4096, 11008, 65, dtype=2)["kernel"] == "f32_mfma" and _plan(4096, 4096, 128, dtype=2)["path"] == "gemv"
    # 2/3/8-bit: the weight-streaming GEMMs take over from 5 rows (int8); int3 keeps the GEMV to 8.  Act-order layers with the re-sequenced
    # side copy run the SAME kernels on a permuted x (perm = 2: one pre-pass, GEMV and GEMM alike), so they share those crossovers
    assert _plan(4096, 11008, 4, bits=8, gs=32)["path"] == "gemv" and _plan(4096, 11008, 8, bits=8, gs=32)["path"] == "gemm"
    # int8, 5..128 rows: the 8-bit form of gemm_mid_kernel (a K-step = two weight DMAs; 11008x4096 M = 16: 32.8 -> 16.7 us), act-order through the
    # permuted-x pre-pass, bf16 too; 65+ rows on 172-strip layers and everything beyond 128 rows: tiled; int3 keeps skinny / tiled
    for K, N in ((4096, 4096), (4096, 11008), (11008, 4096)):
        for m in (5, 8, 16, 64):
            assert _plan(K, N, m, bits=8, gs=32)["kernel"] == "mid", (K, N, m)
    assert _plan(4096, 11008, 8, bits=8, gs=32, act=True)["kernel"] == "mid" and _plan(4096, 11008, 16, bits=8, gs=32, dtype=1)["kernel"] == "mid"
    assert _plan(4096, 11008, 128, bits=8, gs=32)["kernel"] == "tiled" and _plan(11008, 4096, 128, bits=8, gs=32)["kernel"] == "mid"
    # int3 (a K-step = three packed rows = one 48-lane DMA, 24-bit windows funnelled out of the 96-bit stream): from 9 rows, from 5 on 172-strip layers
    assert _plan(4096, 4096, 16, bits=3, gs=32)["kernel"] == "mid" and _plan(11008, 4096, 64, bits=3, gs=32)["kernel"] == "mid"
    assert _plan(4096, 11008, 8, bits=3, gs=32)["kernel"] == "mid" and _plan(4096, 4096, 8, bits=3, gs=32)["kernel"] == "mfma_generic"
    assert _plan(4096, 4128, 16, bits=3, gs=32)["kernel"] != "mid"
    # int2 decode: packed magic-number decode in the register kernel (4096x11008 13.0 -> 8.7 us), the streamed kernel from ~40 M weights (8.0 / 8.1 us)
    p = _plan(4096, 11008, 1, bits=2, gs=64)
    assert (p["kernel"], p["ln"], p["waves"], p["u"], p["ksplit"]) == ("stream", 8, 8, 4, 1), p
    p = _plan(11008, 4096, 2, bits=2, gs=64)
    assert (p["kernel"], p["ln"], p["waves"], p["u"], p["ksplit"], p["mt"]) == ("stream", 4, 8, 2, 1, 2), p
    p = _plan(4096, 4096, 1, bits=2, gs=64)
    assert (p["kernel"], p.get("deq")) == ("mfma_generic", "magic"), p
    assert _plan(4096, 11008, 1, bits=2, gs=64, dtype=1).get("deq") == "magic"               # bf16: the same exact fp16 w - z, pairs converted once (register kernel)
    # int2 (a K-step = two packed rows = one 32-lane DMA): from 5 rows everywhere (4096x11008 M = 8: 24.9 -> 13.3 us)
    assert _plan(4096, 4096, 5, bits=2, gs=64)["kernel"] == "mid" and _plan(4096, 11008, 128, bits=2, gs=64)["kernel"] == "mid"
    assert _plan(4096, 4096, 4, bits=2, gs=64)["path"] == "gemv" and _plan(4096, 4096, 129, bits=2, gs=64)["kernel"] == "tiled"
    for m in (1, 2, 4):                                   # int8 from ~40 M weights: the streamed 3- / 8-bit kernel (gemv_qx_stream_kernel) on a permuted x
        p = _plan(4096, 11008, m, bits=8, gs=32, act=True)
        assert (p["path"], p["kernel"], p["perm"], p["ln"]) == ("gemv", "stream", 2, 8), (m, p)
    p = _plan(4096, 4096, 2, bits=8, gs=32, act=True)
    assert (p["path"], p["kernel"], p["perm"], p.get("deq")) == ("gemv", "mfma_generic", 2, "magic"), p
    # int8 single layers: streamed from ~40 M weights (32-column strips, 4-wave workgroups, 2..4 in-launch K slices); int3 and small int8 layers: register kernel
    p = _plan(4096, 11008, 1, bits=8, gs=32)
    assert (p["kernel"], p["ln"], p["waves"], p["u"], p["ksplit"], p["strips"]) == ("stream", 8, 4, 2, 2, 344), p
    p = _plan(11008, 4096, 4, bits=8, gs=32)
    assert (p["kernel"], p["ln"], p["waves"], p["u"], p["ksplit"], p["mt"]) == ("stream", 8, 4, 4, 4, 4), p
    assert _plan(4096, 4096, 1, bits=8, gs=32)["kernel"] == "mfma_generic" and _plan(4096, 11008, 1, bits=3, gs=32)["kernel"] == "mfma_generic"
    assert _plan(4096, 11008, 1, bits=8, gs=32, dtype=1)["kernel"] == "mfma_generic"          # bf16: no packed magic-number decode
    assert _plan(4096, 11008, 8, bits=8, gs=32, act=True)["path"] == "gemm"
    p = _plan(4096, 11008, 8, bits=3, gs=32, act=True)
    assert _plan(4096, 11008, 8, bits=3, gs=32)["kernel"] == "mid" and (p["path"], p["kernel"], p["perm"]) == ("gemm", "mid", 1), p
    assert _plan(4096, 11008, 16, bits=3, gs=32, act=True)["path"] == "gemm"
    # 5..8 rows, 3-bit fp16, at most 256 strips: ONE pass of the 8-row matrix-core GEMV (8 waves); wider layers keep two 4-row passes
    # -- profiles/r02_nonq4_paths.log (int8 went to gemm_mid_kernel in round 3; its 8-row GEMV stays reachable through tuning.path = 5)
    for K, N in ((4096, 4096), (11008, 4096)):
        p = _plan(K, N, 8, bits=3, gs=32)
        assert (p["path"], p["kernel"], p["mt"], p["waves"]) == ("gemv", "mfma_generic", 8, 8), (K, N, p)
        assert _plan(K, N, 9, bits=8, gs=32)["path"] == "gemm" and _plan(K, N, 8, bits=8, gs=32, dtype=1)["path"] == "gemm"
    assert _plan(4096, 11008, 5, bits=8, gs=32)["path"] == "gemm"
    assert _plan(4096, 4096, 1, bits=3, gs=32, act=True, dtype=1)["perm"] == 2 and _plan(4096, 4096, 1, bits=3, gs=32, act=True, dtype=1).get("deq") == "magic"
    assert _plan(4096, 11008, 8, bits=2, gs=64)["path"] == "gemm" and _plan(4096, 4096, 8, bits=2, gs=64)["kernel"] == "mid"
    # rows of x: GEMV up to 4; 5..8 rows: one matrix-core pass over 16 rows (16-column strips on narrow layers, the streamed
    # 64-column-strip kernel elsewhere) unless the layer has a fused epilogue (the GEMV applies it) or K is long and N small
    assert _plan(4096, 4096, 4)["mt"] == 4 and _plan(4096, 4096, 4)["path"] == "gemv"
    assert _plan(4096, 4096, 8)["kernel"] == "strip16" and _plan(4096, 11008, 2)["path"] == "gemv" and _plan(11008, 4096, 4)["path"] == "gemv"
    assert _plan(28672, 1024, 8)["path"] == "gemv"
    # [gate | up] with the SiLU*mul epilogue: fused in the GEMV for 1..2 rows, streamed kernel + elementwise pass from 3 rows
    # (4096 x 22016, M = 4: 27.7 -> 19.5 us, M = 8: 50.8 -> 19.5 us)
    assert _plan(4096, 22016, 2, epilogue=1)["epilogue"] == "fused"
    for m in (3, 4, 5, 8, 16):
        p = _plan(4096, 22016, m, epilogue=1)
        assert (p["kernel"], p["epilogue"]) == ("stream64", "separate"), (m, p)
    # batched decode, 4 < M <= 64: the streamed 64-column-strip kernel when strips x K slices fill 160..256 workgroups
    p = _plan(4096, 11008, 8)
    assert (p["kernel"], p["ksplit"], p["tiles"], p["waves"], p["mt"]) == ("stream64", 1, "1x172", 16, 1), p
    p = _plan(11008, 4096, 16)
    assert (p["kernel"], p["ksplit"], p["tiles"]) == ("stream64", 4, "1x64"), p
    assert _plan(8192, 3584, 16)["ksplit"] == 4 and _plan(5120, 5120, 16)["ksplit"] == 3 and _plan(3584, 8192, 16)["ksplit"] == 2
    assert _plan(4096, 11008, 16, act=True)["kernel"] == "stream64" and _plan(4096, 11008, 16, dtype=1)["kernel"] == "stream64"
    # 17 .. 128 rows: gemm_mid_kernel (weights, x and group constants by LDS DMA; row tiles of 16: 2 / 4 / 6 / 8; in-launch K slices with flags)
    p = _plan(4096, 11008, 64)
    assert (p["kernel"], p["mt"], p["waves"], p["ksplit"], p["tiles"]) == ("mid", 4, 8, 1, "1x172"), p
    assert _plan(4096, 11008, 17)["kernel"] == "mid" and _plan(4096, 11008, 17)["u"] == 3 and _plan(4096, 11008, 32)["mt"] == 2
    p = _plan(11008, 4096, 96)
    assert (p["kernel"], p["mt"], p["ksplit"], p["u"], p["tiles"]) == ("mid", 6, 4, 2, "1x64"), p
    assert _plan(4096, 4096, 17)["kernel"] == "mid" and _plan(4096, 11008, 64, act=True)["kernel"] == "mid" and _plan(4096, 11008, 64, dtype=1)["kernel"] == "mid"
    # row blocks (workgroups along M, two row tiles each, the blocks of a strip on adjacent ids) instead of / next to K slices where they fill
    # 192..256 workgroups: 4096^2 M = 64: 2 blocks x 2 slices, M = 96 / 128: 3 / 4 blocks and no K split; 11008x4096 the same except at 96 rows
    for K in (4096, 11008):
        for m, tiles, ks in ((48, "2x64", 2), (64, "2x64", 2), (128, "4x64", 1)):
            p = _plan(K, 4096, m)
            assert (p["kernel"], p["tiles"], p["ksplit"], p["mt"]) == ("mid", tiles, ks, 2), (K, m, p)
    assert _plan(4096, 4096, 96)["tiles"] == "3x64" and _plan(11008, 4096, 96)["tiles"] == "1x64"
    assert _plan(5120, 5120, 64)["tiles"] == "1x80" and _plan(5120, 5120, 96)["tiles"] == "3x80" and _plan(3584, 8192, 64)["tiles"] == "2x128"
    assert _plan(8192, 8192, 64)["tiles"] == "2x128" and _plan(8192, 8192, 128)["kernel"] == "tiled"
    # 129 .. 256 rows: blocks of four row tiles on short-K layers that they fill (4096^2: 3 / 4 blocks; 5120^2 at 192 rows), else the tiled kernel
    p = _plan(4096, 4096, 256)
    assert (p["kernel"], p["tiles"], p["ksplit"], p["mt"]) == ("mid", "4x64", 1, 4), p
    assert _plan(4096, 4096, 192)["tiles"] == "3x64" and _plan(5120, 5120, 192)["kernel"] == "mid" and _plan(5120, 5120, 256)["kernel"] == "tiled"
    assert _plan(11008, 4096, 192)["kernel"] == "tiled" and _plan(4096, 4096, 257)["kernel"] == "tiled"
    # ... except: 65+ rows on layers of 160+ strips and 33+ rows on very wide layers (tiled kernel), 97+ rows off the 64-strip layers,
    # 33+ rows on layers of < 32 strips (skinny kernel), other bit widths, N % 64 != 0
    assert _plan(4096, 11008, 65)["kernel"] == "tiled" and _plan(8192, 28672, 64)["kernel"] == "tiled" and _plan(8192, 28672, 32)["kernel"] == "mid"
    assert _plan(5120, 5120, 96)["kernel"] == "mid" and _plan(5120, 5120, 128)["kernel"] == "tiled"
    assert _plan(8192, 1024, 32)["kernel"] == "mid" and _plan(8192, 1024, 64)["kernel"] == "skinny64"
    assert _plan(4096, 4128, 64)["kernel"] != "mid"
    # ... up to 16 rows small layers keep the 16-column strips
    assert _plan(4096, 4096, 9)["kernel"] == "strip16" and _plan(4096, 4096, 16)["kernel"] == "strip16"
    assert _plan(8192, 1024, 16)["kernel"] == "strip16"
    assert _plan(4096, 11008, 16, bits=2, gs=64, dtype=2)["path"] == "gemv"      # fp32 layers: none of the fp16 / bf16 kernels
    # prefill: 128 x 256 tiles, 64-deep K-steps; two K groups per workgroup when there is at most one tile per CU
    p = _plan(4096, 4096, 2048)
    assert (p["kernel"], p["mt"], p["bk"], p["kg"], p["ksplit"], p["tiles"]) == ("tiled", 4, 64, 2, 1, "16x16"), p
    assert _plan(4096, 4096, 4096)["kg"] == 1 and _plan(4096, 11008, 2048)["kg"] == 1 and _plan(11008, 4096, 2048)["kg"] == 2
    pa = _plan(4096, 4096, 2048, act=True)
    assert pa["perm"] == 1 and pa["dma"] == 1 and pa["kg"] == 2
    assert _plan(4096, 4096, 512)["ksplit"] > 1                                       # too few tiles to fill 256 CUs
    assert _plan(4096, 4096, 2048, gs=32)["bk"] == 32
    # forcing a path through tuning
    t = _lib.GptqTuning()
    t.path = 3
    assert _plan(4096, 4096, 1, tuning=t)["path"] == "gemm"
    t.path = 1
    assert _plan(4096, 4096, 1, tuning=t)["kernel"] == "generic"
    with pytest.raises(_lib.GptqError):
        _plan(4096, 4096, 0)


def test_balanced_tail_rule():
    """Tiled kernel, 4-bit fp16 / bf16, 128 x 256 x 64 tiles: the tiles past the last full round of 256 run as 2 / 4 / 8 K slices when the planner's
    time model says it pays (measured in profiles/r03_gemm_balanced_tail_ab.log).  Pinned decisions, the off knob, and the invariants a
    launch relies on: K steps divide over the slices, the flag words fit the ticket half of the header, the workspace covers the slabs."""
    lib = _lib.load()
    off = _lib.GptqTuning()
    off.path, off.reserved[_lib.LAB.GEMM_VARIANT] = 3, _lib.LAB.VARIANT_TAIL_OFF
    pinned = [  # K, N, M, act, dtype -> (tail, slices)
        (4096, 11008, 2048, True, 0, (0, 1)),        # 688 tiles: 176 left over, two slices would only move 45 MB around (measured 0.97 - 1.0x)
        (4096, 11008, 4096, True, 0, (0, 1)),        # 1376 tiles, 96 left over: 6.7 % predicted = noise level measured (+5 % / -5 % in two sessions)
        (4096, 11008, 3072, True, 0, (0, 1)),        # 1032 tiles: beyond ~4 rounds the gain is within the harness-to-harness spread
        (4096, 11008, 2304, False, 0, (6, 8)),       # 242 -> 221 us
        (4096, 4096, 4096, False, 0, (0, 1)),        # 512 tiles: nothing left over
        (4096, 4096, 2048, False, 0, (0, 1)),        # 256 tiles: the 8-wave form
        (4096, 11008, 768, False, 0, (2, 8)),        # 106 -> 85 us
        (4096, 11008, 1024, False, 0, (88, 2)),      # 120 -> 102 us
        (4096, 4096, 2176, False, 1, (16, 4)),       # 111 -> 87 us
        (11008, 4096, 2176, True, 0, (16, 4)),       # 172 K steps: 4 slices of 43
        (8192, 28672, 2048, False, 0, (0, 1)),
    ]
    for K, N, M, act, dt, want in pinned:
        d = _plan(K, N, M, act=act, dtype=dt)
        assert (d["tail"], d["tail_slices"]) == want, (K, N, M, act, dt, d)
        assert _plan(K, N, M, act=act, dtype=dt, tuning=off)["tail"] == 0
    rng = np.random.default_rng(40)
    seen = 0
    for _ in range(3000):
        K = int(rng.choice([512, 1024, 2048, 4096, 5120, 8192, 11008]))
        N = 256 * int(rng.integers(1, 120))
        M = int(rng.integers(65, 20000))
        act = bool(rng.integers(0, 2))
        dt = int(rng.integers(0, 2))
        L = _layer(K=K, N=N, bits=4, group_size=128, dtype=dt)
        if act:
            L.g_idx = L.qweight_seq = L.perm = 0x1000
        d = _lib.describe_plan(L, M, None)
        if d.get("kernel") != "tiled" or not d.get("tail"):
            continue
        seen += 1
        nbm, nbn = map(int, d["tiles"].split("x"))
        s = d["tail_slices"]
        assert s in (2, 4, 8) and d["tail"] == (nbm * nbn) % 256 and 256 < nbm * nbn <= 1024 and d["ksplit"] == 1 and d["kg"] == 1, d
        assert (K // 64) % s == 0 and K // 64 // s >= 4, (K, d)
        assert 16 * d["tail"] * 4 <= 32768, d
        need = int(lib.gptq_workspace_bytes(ctypes.byref(L), M))
        xperm = (M * K * 2 + 255) // 256 * 256 if act else 0
        assert need >= 65536 + xperm + d["tail"] * s * 131072, (K, N, M, act, d, need)
    assert seen > 100


def test_format_round_trips_random():
    """Random layers through the three checkpoint formats: GPTQ -> Marlin -> GPTQ is the identity on symmetric layers, and
    AWQ words -> GPTQ words unpack (oracle) to the integers that were packed, for several shapes and seeds."""
    import numpy as np
    import torch
    from autogptq_amd import marlin
    from oracle import awq_oracle as A
    from oracle import gptq_oracle as O
    rng = np.random.default_rng(0)
    for K, N, gs in ((128, 256, 128), (256, 512, 128), (384, 256, 384)):
        w = rng.integers(0, 16, size=(K, N))
        qw = torch.from_numpy(O.pack_rows(w.astype(np.uint32), 4).copy())
        G = K // gs
        qz = torch.full((G, N // 8), 0x77777777, dtype=torch.int32)
        sc = torch.from_numpy((0.001 * (1 + rng.random((G, N)))).astype(np.float16))
        B, s = marlin.gptq_to_marlin(qw, qz, sc, gs)
        assert tuple(B.shape) == (K // 16, 2 * N) and tuple(s.shape) == (G, N)
        qw2, qz2, sc2 = marlin.marlin_to_gptq(B, s, gs)
        assert torch.equal(qw2, qw) and torch.equal(qz2, qz) and torch.equal(sc2, sc)
    for K, N, gs in ((64, 64, 32), (128, 200, 64), (256, 8, 128)):
        w = rng.integers(0, 16, size=(K, N))
        z = rng.integers(0, 16, size=(K // gs, N))
        qw, qz = A.awq_to_gptq(A.awq_pack(w), A.awq_pack(z))
        assert np.array_equal(O.unpack_rows(qw, 4), w)
        zz = O.unpack_rows(np.ascontiguousarray(qz.T), 4).T            # stored fields: (z - 1) & 15
        assert np.array_equal(zz, (z - 1) & 15)


def test_load_packed_layers_from_gptq_and_marlin_state(tmp_path):
    """load_packed_layers: a model skeleton filled from (a) a GPTQ state dict written with safetensors and (b) the same layers
    serialised in the Marlin layout -- both must leave exactly the GPTQ tensors in the swapped QuantLinear modules, load the
    non-quantized rest, and refuse inconsistent inputs."""
    from safetensors.torch import load_file, save_file
    from autogptq_amd import marlin
    from autogptq_amd.model_utils import load_packed_layers

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.up = torch.nn.Linear(128, 256, bias=True)
            self.norm = torch.nn.LayerNorm(256)
            self.down = torch.nn.Linear(256, 256, bias=False)

    torch.manual_seed(1)
    src = Toy().half()
    gptq_state = {k: v.clone() for k, v in src.state_dict().items() if k.startswith("norm")}
    for name, lin in (("up", src.up), ("down", src.down)):
        K = lin.in_features
        G = K // 128
        W = lin.weight.data.float()
        s = (W.reshape(-1, G, 128).abs().amax(dim=2) / 7 + 1e-4).half()                  # symmetric: zero-point 8
        z = torch.full_like(s, 8)
        qw, qz, sc = O.pack(lin.weight.data.clone(), s, z, torch.from_numpy(O.default_g_idx(K, 128)), 4, torch.float16)
        gptq_state.update({f"{name}.qweight": qw, f"{name}.qzeros": qz, f"{name}.scales": sc,
                           f"{name}.g_idx": torch.from_numpy(O.default_g_idx(K, 128))})
        if lin.bias is not None:
            gptq_state[f"{name}.bias"] = lin.bias.data.clone()
    path = str(tmp_path / "model.safetensors")
    save_file({k: v.contiguous() for k, v in gptq_state.items()}, path)

    m1 = load_packed_layers(Toy().half(), load_file(path), 4, 128)
    assert isinstance(m1.up, QuantLinear) and isinstance(m1.down, QuantLinear) and isinstance(m1.norm, torch.nn.LayerNorm)
    for name in ("up", "down"):
        q = getattr(m1, name)
        for attr in ("qweight", "qzeros", "scales"):
            assert torch.equal(getattr(q, attr), gptq_state[f"{name}.{attr}"]), (name, attr)
    assert torch.equal(m1.up.bias, gptq_state["up.bias"]) and m1.down.bias is None
    assert torch.equal(m1.norm.weight, src.norm.weight)

    marlin_state = {k: v for k, v in gptq_state.items() if k.startswith("norm") or k.endswith(".bias")}
    for name in ("up", "down"):
        B, s = marlin.gptq_to_marlin(gptq_state[f"{name}.qweight"], gptq_state[f"{name}.qzeros"], gptq_state[f"{name}.scales"], 128)
        marlin_state.update({f"{name}.B": B, f"{name}.s": s, f"{name}.workspace": torch.zeros(32, dtype=torch.int32)})
    m2 = load_packed_layers(Toy().half(), marlin_state, 4, 128, checkpoint_format="marlin")
    for name in ("up", "down"):
        for attr in ("qweight", "qzeros", "scales"):
            assert torch.equal(getattr(getattr(m2, name), attr), gptq_state[f"{name}.{attr}"]), (name, attr)
    assert torch.equal(m2.up.bias, gptq_state["up.bias"])

    with pytest.raises(ValueError, match="not supported"):
        load_packed_layers(Toy().half(), gptq_state, 4, 128, quant_method="awq", checkpoint_format="marlin")
    with pytest.raises(KeyError):
        load_packed_layers(Toy().half(), {"nope.qweight": gptq_state["up.qweight"]}, 4, 128)
    bad = dict(gptq_state)
    bad["up.qweight"] = bad["up.qweight"][:, :128]
    with pytest.raises(ValueError, match="shape"):
        load_packed_layers(Toy().half(), bad, 4, 128)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no host implementation"):
            load_packed_layers(Toy().half(), {"up.qweight": torch.zeros(128, 32, dtype=torch.int32), "up.qzeros": torch.zeros(1, 32, dtype=torch.int32),
                                              "up.scales": torch.ones(1, 256).half()}, 4, 128, quant_method="awq", checkpoint_format="gemm")


def test_pack_accepts_conv1d_and_conv2d_modules():
    """pack() takes nn.Linear, HF Conv1D (weight stored [in, out] -> transposed) and nn.Conv2d (weight flattened to [out, in*kh*kw])
    exactly like the reference (qlinear_cuda.py:109-113), and make_quant sizes the replacement from the right attributes
    (auto_gptq/modeling/_utils.py:108-119)."""
    import transformers
    from autogptq_amd.model_utils import make_quant
    torch.manual_seed(3)
    K, N, gs = 64, 96, 32
    g_idx = torch.from_numpy(O.default_g_idx(K, gs))

    c1 = transformers.pytorch_utils.Conv1D(N, K)                       # nf = out, nx = in; weight [K, N]
    c1.weight.data = torch.randn(K, N) * 0.05
    c1.bias.data = torch.randn(N) * 0.1
    c1 = c1.half()
    c2 = torch.nn.Conv2d(K, N, kernel_size=1, bias=False).half()       # weight [N, K, 1, 1]
    for mod, W_nk in ((c1, c1.weight.data.t().contiguous()), (c2, c2.weight.data.flatten(1).contiguous())):
        s, z = O.minmax_quantize(W_nk.float(), 4, gs)
        q = QuantLinear(4, gs, K, N, mod.bias is not None)
        q.pack(mod, s.half(), z.half(), g_idx)
        qw, qz, sc = O.pack(W_nk.clone(), s.half(), z.half(), g_idx, 4, torch.float16)
        assert torch.equal(q.qweight, qw) and torch.equal(q.qzeros, qz) and torch.equal(q.scales, sc)
        if mod.bias is not None:
            assert torch.equal(q.bias, mod.bias.data)

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c1 = transformers.pytorch_utils.Conv1D(N, K)
            self.c2 = torch.nn.Conv2d(K, N, kernel_size=1)

    m = Toy().half()
    make_quant(m, ["c1", "c2"], 4, gs)
    assert (m.c1.infeatures, m.c1.outfeatures, m.c2.infeatures, m.c2.outfeatures) == (K, N, K, N)
    assert m.c1.bias is not None and m.c2.bias is not None


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float16], ids=["bf16", "fp32", "fp16"])
@pytest.mark.parametrize("gs", [16, 32, 128])
def test_host_pack_on_the_reference_value_patterns(gs, dtype):
    """The pack() half of the reference's backend grid (tests/test_hpu_linear.py:102-160: 13 scale/weight/zero value patterns,
    integer zero-points, zero-point 0 that wraps to an all-ones word) on the host implementation, against the oracle."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gpu_parity_helpers", os.path.join(ROOT, "tests", "test_gpu_parity.py"))
    # the pattern generator lives next to the GPU grid test; import only the two names (the module's GPU fixtures are lazy)
    src = open(spec.origin).read()
    start, end = src.index("HPU_PATTERNS = ["), src.index('@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])')
    ns = {"torch": torch}
    exec(src[start:end], ns)
    K = N = 128
    for pi, pattern in enumerate(ns["HPU_PATTERNS"]):
        lin, s, z = ns["_pattern_layer"](K, N, gs, pattern, dtype, bool(pi & 1), seed=pi + gs)
        q = QuantLinear(4, gs, K, N, bool(pi & 1), weight_dtype=dtype)
        q.pack(lin, s.clone(), z.clone(), g_idx=None)
        qw, qz, sc = O.pack(lin.weight.data.clone(), s.clone(), z.clone(), None, 4, dtype)
        assert torch.equal(q.qweight, qw) and torch.equal(q.qzeros, qz) and torch.equal(q.scales, sc), (pattern, gs, dtype)


def test_workspace_max_covers_every_m_and_g_idx_validation():
    """gptq_workspace_bytes_max = max over M of the per-M query (the need is not monotone: K splits come and go), and
    gptq_validate_g_idx rejects group indices the scales / qzeros tensors do not have (host-only, no device work)."""
    lib = _lib.load()
    for K, N, act in ((4096, 4096, False), (4096, 4096, True), (8192, 1024, False), (11008, 4096, True)):
        L = _layer(K=K, N=N)
        if act:
            L.g_idx = L.qweight_seq = L.perm = 0x1000
        per_m = [int(lib.gptq_workspace_bytes(ctypes.byref(L), m)) for m in range(1, 300)]
        assert int(lib.gptq_workspace_bytes_max(ctypes.byref(L), 299)) == max(per_m)
        assert int(lib.gptq_workspace_bytes_max(ctypes.byref(L), 16)) == max(per_m[:16])
    assert any(per_m[i] > per_m[i + 1] for i in range(len(per_m) - 1)), "expected a non-monotone need somewhere in 1..299"
    g = torch.arange(256, dtype=torch.int32) // 128
    assert lib.gptq_validate_g_idx(g.data_ptr(), 256, 2) == 0
    assert lib.gptq_validate_g_idx(g.data_ptr(), 256, 1) == 2 and b"outside [0, 1)" in lib.gptq_last_error()
    g[7] = -1
    assert lib.gptq_validate_g_idx(g.data_ptr(), 256, 2) == 2 and b"g_idx[7]" in lib.gptq_last_error()
    assert lib.gptq_validate_g_idx(None, 256, 2) == 1


def test_tensor_parallel_wrappers_refuse_fused_epilogue_layers():
    from autogptq_amd.tensor_parallel import ColumnParallelQuantLinear, RowParallelQuantLinear
    f = QuantLinear(4, 128, 256, 512, False, epilogue="silu_mul")
    with pytest.raises(ValueError, match="fused epilogue"):
        ColumnParallelQuantLinear.from_full(f, 0, 2)
    with pytest.raises(ValueError, match="fused epilogue"):
        RowParallelQuantLinear.from_full(f, 0, 2)


def test_planner_fuzz_every_configuration_plans_or_refuses_cleanly():
    """gptq_describe_plan / gptq_workspace_bytes[_max] over a few thousand random (bits, group size, K, N, M, dtype, act-order flavour,
    epilogue) configurations: a status code and a parsable plan or a clean refusal, never a crash (a division by zero for
    group_size < 32 on the fp32 GEMM path was found this way in round 2), a workspace need that covers the plan's K split, and
    gptq_workspace_bytes_max >= the need at every M it covers."""
    import random
    lib = _lib.load()
    rnd = random.Random(20260923)
    Ks = [32, 64, 96, 128, 160, 256, 320, 512, 1024, 1536, 2048, 4096, 5120, 8192, 11008, 13824, 28672]
    Ns = [32, 64, 96, 128, 256, 320, 512, 1024, 3584, 4096, 5120, 8192, 11008, 12288, 22016, 28672]
    Ms = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128, 200, 512, 2048, 4096]
    seen = set()
    for _ in range(6000):
        K, N, bits = rnd.choice(Ks), rnd.choice(Ns), rnd.choice((2, 3, 4, 8))
        gs = rnd.choice((16, 32, 64, 128, 256, 1024, K))
        L = _layer(K=K, N=N, bits=bits, group_size=gs, dtype=rnd.choice((0, 1, 2)), zero_mode=rnd.choice((0, 1)), epilogue=rnd.choice((0, 0, 0, 1)))
        act = rnd.choice((0, 0, 1, 2))
        if act:
            L.g_idx = 0x1000                              # raw act-order ...
            if act == 2:
                L.qweight_seq = L.perm = 0x1000           # ... or with the re-sequenced side copy
        M = rnd.choice(Ms)
        buf = ctypes.create_string_buffer(512)
        rc = lib.gptq_describe_plan(ctypes.byref(L), M, None, buf, len(buf))
        assert rc in (0, 2, 3), (rc, K, N, bits, gs, M)
        need = lib.gptq_workspace_bytes(ctypes.byref(L), M)
        if rc != 0:
            continue
        plan = dict(kv.split("=", 1) for kv in buf.value.decode().split())
        seen.add(plan["kernel"])
        assert plan["path"] in ("gemv", "gemm") and int(plan["ksplit"]) >= 1
        if int(plan["ksplit"]) > 1 and plan["kernel"] not in ("stream", "stream64", "mid"):      # fp32 slabs [ksplit, M, N] behind the header
            assert need >= int(plan["ksplit"]) * M * (N // (2 if L.epilogue and plan.get("pair") == "1" else 1)) * 4 // 2, (plan, need)
        if plan["kernel"] == "mid":
            # gemm_mid_kernel: the owner slices WAIT for the others, so a K-split launch must fit one workgroup per CU (256); (ksplit - 1) fp32 tiles
            # behind the header (and the permuted x of an act-order layer); row blocks x row tiles cover M
            rb, strips = map(int, plan["tiles"].split("x"))
            ks, rt = int(plan["ksplit"]), int(plan["mt"])
            assert bits in (2, 3, 4, 8) and N % 64 == 0 and strips == N // 64 and rt in (1, 2, 4, 6, 8) and rb * rt * 16 >= M and (rb - 1) * rt * 16 < M, plan
            assert ks == 1 or rb * strips * ks <= 256, plan
            assert need >= (ks - 1) * M * N * 4 + (65536 if ks > 1 else 0), (plan, need)
            assert 2 <= int(plan["u"]) <= 3 and 4 <= int(plan["waves"]) <= 8, plan
        assert need < (1 << 34)
        assert lib.gptq_workspace_bytes_max(ctypes.byref(L), M) >= need
    assert {"mfma", "mfma_generic", "generic", "tiled", "skinny64", "stream64", "strip16", "f32_mfma", "mid", "stream"} <= seen, seen



def test_planner_fuzz_layers_with_a_decode_copy():
    """The same over layers that carry the decode copy (round 4; pointers never dereferenced by the planner): gptq_prepack_decode_bytes agrees with the
    layouts' sizes or refuses; up to 4 rows the plan is the decode-copy kernel ("strips") whenever a copy can exist and its geometry fits -- with legal
    geometry (1..16 waves, 1 / 2 / 4 / 8 chunks per wave, <= 8 K slices, workspace = header + (ksplit - 1) M N 8 bytes of granules) -- act-order layers
    only with their re-sequenced rows; M = 4096 on wide layers takes the wide tiles from the copy ("wide_copy"), 4-bit layers only."""
    import random
    lib = _lib.load()
    rnd = random.Random(4)
    Ks = [32, 64, 96, 128, 160, 512, 1024, 2048, 4096, 4160, 8192, 11008, 28672]
    Ns = [16, 32, 64, 96, 256, 1024, 3584, 4096, 11008, 12288, 22016, 28672]
    seen = set()
    for _ in range(4000):
        K, N, bits = rnd.choice(Ks), rnd.choice(Ns), rnd.choice((2, 3, 4, 8))
        gs = rnd.choice((16, 32, 64, 96, 128, 256, K))
        L = _layer(K=K, N=N, bits=bits, group_size=gs, dtype=rnd.choice((0, 1, 2)), zero_mode=rnd.choice((0, 1)), epilogue=rnd.choice((0, 0, 0, 1)))
        act = rnd.choice((0, 0, 1, 2))
        if act:
            L.g_idx = 0x1000
            if act == 2:
                L.qweight_seq = L.perm = 0x1000
        tb, cb = ctypes.c_size_t(7), ctypes.c_size_t(7)
        rc = lib.gptq_prepack_decode_bytes(ctypes.byref(L), ctypes.byref(tb), ctypes.byref(cb))
        kpl = 16 if bits == 8 else 32
        # [gate | up] layers with the fused epilogue: plain ones get a copy too (round 5: the pair form of the decode kernel), act-order ones do not
        can = (L.dtype in (0, 1) and (L.epilogue == 0 or (bits != 2 and act == 0 and N % 64 == 0)) and K % 32 == 0 and N % 32 == 0 and gs % kpl == 0
               and act != 1 and (gs >= K or ((gs // kpl) & (gs // kpl - 1)) == 0))
        if not can:
            assert rc != 0 and tb.value == 0 and cb.value == 0, (rc, K, N, bits, gs, act)
            continue
        assert rc == 0, (lib.gptq_last_error(), K, N, bits, gs, act)
        cke = 4 * kpl
        assert tb.value == -(-K // cke) * (768 if bits == 3 else (512 if bits == 2 else 1024)) * (N // 16)
        assert cb.value == -(-K // gs) * (64 if bits == 8 else 48) * (N // 16)
        L.qweight_tiled = L.qconst_tiled = 0x2000
        L.tiled_cols = 16
        for M in (1, 2, 3, 4, 5, 8, 9, 4096):
            buf = ctypes.create_string_buffer(512)
            rc = lib.gptq_describe_plan(ctypes.byref(L), M, None, buf, len(buf))
            assert rc in (0, 2, 3), (rc, K, N, bits, gs, M)
            if rc:
                continue
            plan = dict(kv.split("=", 1) for kv in buf.value.decode().split())
            seen.add(plan["kernel"])
            need = lib.gptq_workspace_bytes(ctypes.byref(L), M)
            if plan["kernel"] == "strips":
                ks, waves, u = int(plan["ksplit"]), int(plan["waves"]), int(plan["u"])
                assert M <= 8 and 1 <= ks <= 8 and 1 <= waves <= 16 and u in (2, 4), plan
                # (a [gate | up] layer too deep for the pair form runs this kernel on the plain layer and SiLU * mul as a pass of its own: y [M, N] in front)
                y = -(-M * N * 2 // 256) * 256 if plan["epilogue"] == "separate" else 0
                assert y == 0 or (L.epilogue and plan["pair"] == "0"), plan
                assert need == (0 if ks == 1 and not y else 65536 + y + (ks - 1) * M * N * 8), (plan, need)
                if L.epilogue and not y:      # the pair form: strip s of gate and of up per workgroup, an even number of waves, no K slices, nothing staged in a workspace
                    assert plan["pair"] == "1" and plan["epilogue"] == "fused" and M <= 4 and ks == 1 and waves % 2 == 0 and int(plan["strips"]) == N // 32, plan
            if M > 4 and plan["kernel"] == "strips":      # 5..8 rows: only where the measured rule says it pays (a single plain 4-bit layer around 4096 x 4096)
                assert M <= 8 and bits == 4 and act == 0 and 2048 <= K <= 4096 and 2048 <= N <= 4096, plan
            if plan["kernel"] == "wide_copy":
                assert M >= 2048 and bits == 4 and act in (0, 2) and K % 128 == 0, plan      # act-order layers: with their re-sequenced rows (the copy is made of them)
            assert lib.gptq_workspace_bytes_max(ctypes.byref(L), M) >= need
    assert {"strips", "wide_copy"} <= seen, seen


def test_stream_k_prefill_rules_for_every_packing():
    """Round 5, host only: where the planner sends prefill rows of layers that carry a decode copy to the stream-K kernel (csrc/gemm_wide_sk.hip: wide_sk_ok /
    wide_sk_pays) -- 4-bit groups of 64 / 128 multiples from 768 rows (512 on large layers) unless whole rounds of 128 x 512 tiles fill the chip, and the 3-bit,
    8-bit and 32-wide-group forms (gemm_wide_sk_b38.hip) from 512 rows (384 / 256 on large layers: profiles/r05_wide_sk_b38_ab.log) -- and that the workspace
    query covers the published pieces (128 KiB per workgroup when any range boundary falls inside a tile) behind the permuted x of act-order layers."""
    lib = _lib.load()

    def plan(bits, gs, K, N, M, act=False, copy=True, dtype=0):
        L = _layer(K=K, N=N, bits=bits, group_size=gs, dtype=dtype)
        if act:
            L.g_idx = L.qweight_seq = L.perm = 0x1000
        if copy:
            L.qweight_tiled = L.qconst_tiled = 0x2000
            L.tiled_cols = 16
        buf = ctypes.create_string_buffer(512)
        assert lib.gptq_describe_plan(ctypes.byref(L), M, None, buf, len(buf)) == 0, lib.gptq_last_error()
        d = dict(kv.split("=", 1) for kv in buf.value.decode().split())
        return d, lib.gptq_workspace_bytes(ctypes.byref(L), M)

    for K, N in ((4096, 4096), (4096, 11008), (11008, 4096)):
        for act in (False, True):
            d, need = plan(4, 128, K, N, 2048, act)                                   # BASELINE config 3
            assert d["kernel"] == "wide_sk" and d["perm"] == str(int(act)) and d["tiles"] == f"16x{-(-N // 256)}", d
            cut = N == 11008                                                            # 688 tiles on 256 workgroups; 256 tiles = one each, nothing published
            xperm = 2048 * K * 2 if act else 0
            assert need == (65536 if (cut or act) else 0) + xperm + (256 * 131072 if cut else 0), (d, need)      # header + permuted x + 128 KiB per workgroup
        assert plan(4, 128, K, N, 4096)[0]["kernel"] == "wide_copy"                    # whole rounds of 128 x 512 tiles stay whole tiles
        assert plan(4, 128, K, N, 2048, copy=False)[0]["kernel"] != "wide_sk"          # no copy, no stream-K
        for bits in (3, 8):                                                            # BASELINE config 5
            for dtype in (0, 1):
                assert plan(bits, 32, K, N, 2048, dtype=dtype)[0]["kernel"] == "wide_sk"
            assert plan(bits, 32, K, N, 2048, act=True)[0]["kernel"] == "wide_sk"
            assert plan(bits, 128, K, N, 4096)[0]["kernel"] == "wide_sk"               # no 128 x 512 form for these widths
            # round 6: below ~512 rows the whole-K panel kernel takes these layers where its tiles fill the chip and its time model beats stream-K's
            # (profiles/r06_panel_b38.log): one round of 64 x 128 tiles at 512 rows on 4096^2 and (3 bits) 11008x4096, 256 rows everywhere
            assert plan(bits, 32, K, N, 512)[0]["kernel"] == ("panel" if (K, N) == (4096, 4096) or ((K, N) == (11008, 4096) and bits == 3) else "wide_sk")
            assert plan(bits, 32, K, N, 384)[0]["kernel"] == ("wide_sk" if K * N >= 32 << 20 else "panel")
            assert plan(bits, 32, K, N, 256)[0]["kernel"] == "panel"
            assert plan(bits, 32, K, N, 128)[0]["kernel"] != "wide_sk"
        assert plan(4, 32, K, N, 2048)[0]["kernel"] == "wide_sk"                       # 4 bits on 32-wide groups: each half of the wave on its own group
    assert plan(4, 96, 4032, 4096, 2048)[0]["kernel"] != "wide_sk"                     # groups of 96: not a group mode of the kernel
    assert plan(3, 32, 4096 + 128, 4096, 2048)[0]["kernel"] != "wide_sk"               # K % 256 != 0: the two K parts need whole 128-deep chunks
    assert plan(2, 32, 4096, 4096, 2048, copy=False)[0]["kernel"] != "wide_sk"         # 2 bits have no decode copy


def test_batched_decode_rows_kernel_rules():
    """Round 5, host only: 5 .. 128 rows of a layer that carries its decode copy go to the exchange-free kernel (csrc/gemm_rows.hip: rows_ok / rows_pays /
    plan_rows) -- 3-, 4- and 8-bit, 32- / 64-wide groups and power-of-two multiples of 128, layers of 1024+ rows and columns and at most 64 Mi weights, 65+ rows
    only up to 46 M weights and 8192 columns -- with a geometry the library is built for (RB in {1, 2}, S in {1, 2, 3, 4, 6}; 6 strips only at 4 bits with two row
    blocks), no workspace beyond the permuted x of act-order layers; decode rows keep the decode kernel, 129+ rows and layers without a copy the older ones."""
    lib = _lib.load()

    def plan(bits, gs, K, N, M, act=False, copy=True, dtype=0):
        L = _layer(K=K, N=N, bits=bits, group_size=gs, dtype=dtype)
        if act:
            L.g_idx = L.qweight_seq = L.perm = 0x1000
        if copy:
            L.qweight_tiled = L.qconst_tiled = 0x2000
            L.tiled_cols = 16
        buf = ctypes.create_string_buffer(512)
        assert lib.gptq_describe_plan(ctypes.byref(L), M, None, buf, len(buf)) == 0, lib.gptq_last_error()
        return dict(kv.split("=", 1) for kv in buf.value.decode().split()), lib.gptq_workspace_bytes(ctypes.byref(L), M)

    for bits in (3, 4, 8):
        for gs in (32, 64, 128, 256):
            for K, N in ((4096, 4096), (4096, 11008), (11008, 4096), (2048, 2048), (8192, 1024), (1024, 8192), (8192, 8192)):
                for M in (5, 8, 16, 33, 64):
                    for act in (False, True):
                        d, need = plan(bits, gs, K, N, M, act)
                        if M >= 33 and N >= 8192 and K <= 8192:      # round 6: 33 .. 64 rows of the wide layers = ONE (partial) row panel, 172+ tiles of the panel kernel (every packing of the copy)
                            assert d["kernel"] == "panel", (bits, gs, K, N, M, act, d)
                            continue
                        if act and K >= 8192 and M <= 16 and bits == 4:      # late round 6: act-order layers of K >= 8192 at up to 16 rows keep the 64-column-strip kernel (the permute pre-pass costs more than it saves)
                            assert d["kernel"] != "rows", (bits, gs, K, N, M, act, d)
                            continue
                        assert d["kernel"] == "rows", (bits, gs, K, N, M, act, d)
                        rb, s = int(d["mt"]), int(d["tiles"].split("x")[1])
                        assert rb in (1, 2) and int(d["tiles"].split("x")[0]) == -(-M // (16 * rb)), d      # (the 64-row form only from 129 rows)
                        per = -(-(N // 16) // s)                      # strips per workgroup
                        assert per in (1, 2, 3, 4, 6) and (per != 6 or (bits == 4 and rb == 2)) and not (bits == 8 and rb == 1 and per == 4), d
                        assert need == (65536 + (M * K * 2 + 255) // 256 * 256 if act else 0), (d, need)      # header + permuted x, or nothing
    for M in (96, 128):                                          # (round 6: the panel kernel takes 4096^2 from 96 rows; deep layers at few rows stay here)
        assert plan(4, 128, 4096, 4096, M)[0]["kernel"] == "panel" and plan(4, 128, 11008, 4096, M)[0]["kernel"] == "rows"
        assert plan(3, 128, 4096, 4096, M)[0]["kernel"] == "panel" and plan(8, 32, 4096, 4096, M)[0]["kernel"] == "panel"      # (3 / 8 bits and 32-wide groups too)
        assert plan(3, 32, 11008, 4096, M)[0]["kernel"] == "rows"
        assert plan(4, 128, 4096, 11008, M)[0]["kernel"] != "rows" and plan(4, 128, 8192, 8192, M)[0]["kernel"] != "rows"
    for M in (1, 2, 4):
        assert plan(4, 128, 4096, 4096, M)[0]["kernel"] == "strips"
    for M in (129, 192, 256):                                    # short prompts: the panel kernel (round 6); the 64-row form of this kernel where the panel kernel has no form (groups of 96)
        assert plan(4, 128, 4096, 4096, M)[0]["kernel"] == "panel" and plan(4, 32, 4096, 4096, M)[0]["kernel"] == "panel"
        assert plan(3, 128, 4096, 4096, M)[0]["kernel"] != "rows" and plan(4, 128, 4096, 11008, M)[0]["kernel"] != "rows"
    assert plan(4, 128, 4096, 4096, 257)[0]["kernel"] != "rows" and plan(4, 128, 4096, 4096, 16, copy=False)[0]["kernel"] != "rows"
    assert plan(4, 128, 8192, 28672, 16)[0]["kernel"] != "rows" and plan(4, 128, 512, 4096, 16)[0]["kernel"] != "rows"      # several rounds of workgroups / a small layer
    assert plan(2, 128, 4096, 4096, 16, copy=False)[0]["kernel"] != "rows"
    assert plan(4, 96, 4032, 4096, 16)[0]["kernel"] != "rows"                                                             # groups of 96


def test_decode_copy_restatement_matches_the_header_definition():
    """oracle.decode_copy_weights / decode_copy_consts restate gptq_prepack_decode (include/gptq_mi355x.h, gptq_layer_t.qweight_tiled / qconst_tiled): checked
    entry by entry against the header's formula on a small layer (ragged last chunk: K = 160), that the magic-number extraction order of a stored word is
    k0 k1 | k2 k3 | k4 k5 | k6 k7, that the inverse restores the checkpoint tensor (so the reference's integer unpack is unchanged), and that the constants are
    the reference's scales (bit copies) and zero-points as used (both conventions)."""
    import numpy as np

    K, N, gs = 160, 64, 32
    L = O.random_quant_layer(K, N, 4, gs, seed=1)
    q = L["qweight"].numpy().view(np.uint32)
    t = O.decode_copy_weights(L["qweight"])
    assert tuple(t.shape) == (N // 16, 2, 4, 16, 4)
    tn = t.numpy().view(np.uint32)
    w = O.unpack_weights(L["qweight"], 4)                                                    # the reference's unpack, [K, N]
    for s_ in range(N // 16):
        for c in range(2):
            for kb in range(4):
                for col in range(0, 16, 5):
                    for wi in range(4):
                        r = 16 * c + 4 * kb + wi
                        word = int(tn[s_, c, kb, col, wi])
                        if r >= K // 8:
                            assert word == 0
                            continue
                        got = [(word >> sh) & 15 for sh in (0, 16, 4, 20, 8, 24, 12, 28)]      # (q & 0x000f000f) lo / hi, (q & 0x00f000f0), then the same on q >> 8
                        assert got == [int(w[8 * r + j, 16 * s_ + col]) for j in range(8)]
                        assert sorted((word >> (4 * p)) & 15 for p in range(8)) == sorted((int(q[r, 16 * s_ + col]) >> (4 * p)) & 15 for p in range(8))
    back = O.decode_copy_weights_inverse(t, K)
    assert torch.equal(back, L["qweight"])
    assert np.array_equal(O.unpack_weights(back, 4), w)
    for mode in (O.ZERO_WRAP, O.ZERO_NOWRAP):
        cst = O.decode_copy_consts(L["qzeros"], L["scales"], mode).numpy()
        z = O.unpack_zeros(L["qzeros"], 4, mode)
        sb = L["scales"].view(torch.int16).numpy()
        for s_ in range(N // 16):
            for g in range(K // gs):
                rec = cst[s_, g]
                assert np.array_equal(rec[:32].view(np.int16), sb[g, 16 * s_:16 * s_ + 16])
                assert np.array_equal(rec[32:], z[g, 16 * s_:16 * s_ + 16].astype(np.uint8))


@pytest.mark.parametrize("bits", [2, 3, 8])
def test_decode_copy_restatement_3_and_8_bit(bits):
    """The 3- and 8-bit decode copies (include/gptq_mi355x.h): the masks the decode kernel applies to a stored word yield the reference's unpacked values
    (oracle.unpack_weights = qlinear_cuda.py:250-290) in k order -- 8-bit (q & 0x00ff00ff) = (k0, k1), (q >> 8 & ...) = (k2, k3); 3-bit five fields per 16-bit
    half at bits 0, 3, .. 12 with pair p = 5 j + i = (k 2p, k 2p + 1), and (k30, k31) from bits 15 / 31 of the three words -- with a ragged last chunk."""
    import numpy as np

    K, N, gs = (160, 32, 32) if bits in (2, 3) else (80 * 2, 32, 16)      # (2 bits, round 6: pair p of word w = (k 16w + 2p, k 16w + 2p + 1) at bit 2p of the halves)
    L = O.random_quant_layer(K, N, bits, gs, seed=3)
    w = O.unpack_weights(L["qweight"], bits)
    t = O.decode_copy_weights(L["qweight"], bits).numpy().view(np.uint32)
    kpl, wpl = (16, 4) if bits == 8 else (32, 3 if bits == 3 else 2)
    chunks = -(-K // (4 * kpl))
    assert t.shape == (N // 16, chunks, 4, 16, wpl)
    for s_ in range(N // 16):
        for c in range(chunks):
            for kb in range(4):
                for col in (0, 7, 15):
                    k0 = c * 4 * kpl + kb * kpl
                    words = [int(x) for x in t[s_, c, kb, col]]
                    if bits == 8:
                        got = []
                        for q in words:
                            got += [q & 0xFF, (q >> 16) & 0xFF, (q >> 8) & 0xFF, (q >> 24) & 0xFF]
                    elif bits == 2:
                        got = []
                        for q in words:                      # the kernel's masks: 0x00030003 << 2p on the word (p = 0..4) and on the word >> 10 (p = 5..7)
                            for p in range(8):
                                got += [(q >> (2 * p)) & 3, (q >> (16 + 2 * p)) & 3]
                    else:
                        pairs = []
                        for q in words:
                            for i in range(5):
                                pairs.append(((q >> (3 * i)) & 7, (q >> (16 + 3 * i)) & 7))
                        e_lo = sum(((words[j] >> 15) & 1) << j for j in range(3))
                        e_hi = sum(((words[j] >> 31) & 1) << j for j in range(3))
                        pairs.append((e_lo, e_hi))
                        got = [v for pr in pairs for v in pr]
                    want = [int(w[k0 + j, 16 * s_ + col]) if k0 + j < K else 0 for j in range(kpl)]
                    assert got == want, (s_, c, kb, col)
    for mode in (O.ZERO_WRAP, O.ZERO_NOWRAP):
        cst = O.decode_copy_consts(L["qzeros"], L["scales"], mode, bits).numpy()
        z = O.unpack_zeros(L["qzeros"], bits, mode)
        sb = L["scales"].view(torch.int16).numpy()
        G = K // gs
        assert cst.shape == (N // 16, G, 64 if bits == 8 else 48)
        for s_ in range(N // 16):
            for g in range(G):
                rec = cst[s_, g]
                assert np.array_equal(rec[:32].view(np.int16), sb[g, 16 * s_:16 * s_ + 16])
                zz = rec[32:].view(np.uint16) if bits == 8 else rec[32:]
                assert np.array_equal(zz.astype(np.int64), z[g, 16 * s_:16 * s_ + 16].astype(np.int64))


def test_tools_and_bench_parse():
    """Every measurement script under tools/ (and bench.py, __graft_entry__.py) at least parses and only imports what exists: they run on the GPU box where a
    SyntaxError or a renamed helper costs a paid call.  Names imported from this repo's own modules are resolved against those modules' top-level
    definitions (AST only: nothing is executed, no GPU needed)."""
    import ast
    import glob
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "tools", "*.py"))) + [os.path.join(root, "bench.py"), os.path.join(root, "__graft_entry__.py")]
    assert len(files) > 20

    def top_level_names(path):
        tree = ast.parse(open(path).read(), path)
        names = set()
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef, ast.AsyncFunctionDef)):
                names.add(node.name)
            elif isinstance(node, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
                for t in (node.targets if isinstance(node, ast.Assign) else [node.target]):
                    for n in ast.walk(t):
                        if isinstance(n, ast.Name):
                            names.add(n.id)
            elif isinstance(node, (ast.Import, ast.ImportFrom)):
                for a in node.names:
                    names.add((a.asname or a.name).split(".")[0])
            elif isinstance(node, (ast.If, ast.Try, ast.With, ast.For)):
                for n in ast.walk(node):
                    if isinstance(n, (ast.FunctionDef, ast.ClassDef)):
                        names.add(n.name)
                    elif isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store):
                        names.add(n.id)
                    elif isinstance(n, (ast.Import, ast.ImportFrom)):
                        for a in n.names:
                            names.add((a.asname or a.name).split(".")[0])
        return names

    own = {"bench": os.path.join(root, "bench.py")}
    for mod in glob.glob(os.path.join(root, "autogptq_amd", "*.py")):
        own["autogptq_amd." + os.path.basename(mod)[:-3]] = mod
    own["autogptq_amd"] = os.path.join(root, "autogptq_amd", "__init__.py")
    for mod in glob.glob(os.path.join(root, "oracle", "*.py")):
        own["oracle." + os.path.basename(mod)[:-3]] = mod
    defined = {k: top_level_names(v) for k, v in own.items()}
    submodules = {"autogptq_amd": {k.split(".", 1)[1] for k in own if k.startswith("autogptq_amd.")},
                  "oracle": {k.split(".", 1)[1] for k in own if k.startswith("oracle.")}}
    missing = []
    for f in files:
        tree = ast.parse(open(f).read(), f)                      # SyntaxError fails the test here
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level == 0 and node.module in defined:
                for a in node.names:
                    if a.name != "*" and a.name not in defined[node.module] and a.name not in submodules.get(node.module, ()):
                        missing.append((os.path.relpath(f, root), node.module, a.name))
    assert not missing, missing


def test_panel_kernel_is_planned_where_its_tiles_fill_the_chip():
    """gptq_describe_plan (host only), round 6: the whole-K panel kernel (csrc/gemm_panel.hip) on layers that carry their decode copy -- chosen where its 64-row
    tiles fill the 256 CUs (>= ~160 tiles per round) and the measured competitors lose (profiles/r06_panel_sweep_cold.log): 96 ... 767 rows on 4096 -> 4096, up to
    384 rows on 4096 -> 11008 (stream-K from 512), 160 ... 512 rows on 11008 -> 4096; never without a decode copy or for groups that are no power-of-two multiple of 32; 3-, 4- and 8-bit, 32-wide groups included;
    geometry = the time model's choice (tiles 64 x 32 NT); forced geometries through the lab knob; workspace = the permuted x of act-order layers only."""
    lib = _lib.load()

    def plan(K, N, M, copy=True, act=False, tune=None, **kw):
        L = _layer(K=K, N=N, **kw)
        if copy:
            L.qweight_tiled = L.qconst_tiled = 0x2000
            L.tiled_cols = 16
        if act:
            L.g_idx = L.qweight_seq = L.perm = 0x1000
        return _lib.describe_plan(L, M, tune), L

    want = {
        (4096, 4096): {48: "rows", 64: "rows", 65: "panel", 96: "panel", 128: "panel", 256: "panel", 512: "panel", 767: "panel", 768: "wide_sk", 2048: "wide_sk"},      # from 65 rows = two row panels = 256 tiles
        (4096, 11008): {32: "rows", 33: "panel", 48: "panel", 64: "panel", 128: "panel", 384: "panel", 512: "wide_sk", 2048: "wide_sk"},                              # 33 .. 63 rows: one partial panel (172 tiles) against two rounds of row tiles
        (11008, 4096): {64: "rows", 80: "rows", 128: "rows", 160: "panel", 512: "panel", 640: "wide_sk"},
        (5120, 5120): {80: "rows"},                                 # 160 tiles of 256: the rows kernel keeps 65 .. 95 rows (profiles/r06_panel_65_95.log: 0.87x)
        (2048, 4096): {64: "rows", 80: "panel"},
        (8192, 8192): {80: "panel"},
        (8192, 1024): {128: "rows", 256: "rows", 512: "panel", 768: "panel"},
        (28672, 1024): {256: "rows", 512: "tiled", 768: "panel"},
        (8192, 28672): {128: "tiled", 256: "tiled", 512: "wide_sk"},
    }
    for (K, N), by_m in want.items():
        for M, kern in by_m.items():
            p, _ = plan(K, N, M)
            assert p["kernel"] == kern, (K, N, M, p)
    # tile geometry: 64 rows x 32 NT columns, NT from the time model (one round of 256 tiles where it exists)
    assert plan(4096, 4096, 256)[0]["tiles"] == "4x64" and plan(4096, 4096, 512)[0]["tiles"] == "8x32" and plan(4096, 11008, 128)[0]["tiles"] == "2x115"
    p, _ = plan(4096, 4096, 512)
    assert (p["mt"], p["bk"], p["waves"], p["ksplit"], p["perm"]) == (2, 64, 8, 1, 0), p
    # not without the decode copy, not for the other packings / 32-wide groups / a fused epilogue
    assert plan(4096, 4096, 256, copy=False)[0]["kernel"] != "panel"
    for kw in (dict(bits=3, group_size=128), dict(bits=8, group_size=128), dict(group_size=32), dict(bits=3, group_size=32)):      # every packing of the copy, 32-wide groups
        assert plan(4096, 4096, 256, **kw)[0]["kernel"] == "panel", kw
    assert plan(4096, 4096, 256, bits=2, group_size=128, copy=False)[0]["kernel"] != "panel" and plan(4032, 4096, 256, group_size=96)[0]["kernel"] != "panel"
    assert plan(4096, 4096, 256, bits=8, group_size=128)[0]["tiles"] in ("4x64", "4x43", "4x128")      # (8 bits: at most three column blocks per tile)
    p, _ = plan(4096, 4096, 256, epilogue=1)                     # a [gate | up] layer: the kernel runs on the plain layer, SiLU * mul is a separate pass over the staged y
    assert p["kernel"] == "panel" and p["epilogue"] == "separate", p
    # act-order: x permuted in natural order by the pre-pass; the workspace is that and nothing else
    p, L = plan(4096, 4096, 300, act=True)
    assert p["kernel"] == "panel" and p["perm"] == 1, p
    assert int(lib.gptq_workspace_bytes(ctypes.byref(L), 300)) == 65536 + 300 * 4096 * 2
    p, L = plan(4096, 4096, 300)
    assert int(lib.gptq_workspace_bytes(ctypes.byref(L), 300)) == 0
    # the lab knob forces it (and a geometry) wherever it is legal, and switches it off
    t = _lib.GptqTuning()
    t.path, t.reserved[_lib.LAB.GEMM_VARIANT], t.reserved[0] = 3, _lib.LAB.VARIANT_PANEL_ON, 23
    assert plan(1024, 256, 64, tune=t)[0]["kernel"] == "panel" and plan(1024, 256, 64, tune=t)[0]["tiles"] == "1x3"
    t.reserved[_lib.LAB.GEMM_VARIANT], t.reserved[0] = _lib.LAB.VARIANT_PANEL_OFF, 0
    assert plan(4096, 4096, 256, tune=t)[0]["kernel"] != "panel"


def test_planner_rules_beyond_the_7b_shapes():
    """gptq_describe_plan (host only), late round 6: the rules the row-count / geometry sweeps over the 13B / 30B / 70B / 8B layers produced (DESIGN.md 4.1 'the planner beyond
    the Llama-7B shapes', 4.5 (i)-(v); tools/m_sweep.py, strips_geom_sweep.py, mid_band_sweep.py, tp_shard_sweep.py) -- pinned here so that a later threshold edit shows up
    without a GPU."""
    def plan(K, N, M, act=False, **kw):
        L = _layer(K=K, N=N, **kw)
        L.qweight_tiled = L.qconst_tiled = 0x2000
        L.tiled_cols = 16
        if act:
            L.g_idx = L.qweight_seq = L.perm = 0x1000
        return _lib.describe_plan(L, M, None)

    # decode geometry: <= 256 workgroups 16 waves x 2 chunks, 257 .. 512 8 x 2 (two co-resident workgroups per CU), more 4 x 4
    for (K, N), want in (((4096, 4096), (16, 2)), ((11008, 4096), (16, 2)), ((5120, 5120), (8, 2)), ((13824, 5120), (8, 2)), ((6656, 6656), (8, 2)), ((8192, 8192), (8, 2)),
                         ((4096, 11008), (4, 4)), ((4096, 12288), (4, 4))):
        p = plan(K, N, 1)
        assert (p["kernel"], p["waves"], p["u"]) == ("strips",) + want, (K, N, p)
    # two strips per workgroup from 768 strips where K = 5120 / 6656 do not divide into passes of 16 chunks (strips = workgroups: halved), not for K = 4096 below 1024 strips
    assert plan(5120, 13824, 1)["strips"] == 432 and plan(4096, 12288, 1)["strips"] == 768 and plan(4096, 22016, 1)["strips"] == 688
    p = plan(5120, 13824, 4)
    assert (p["strips"], p["waves"], p["u"]) == (432, 8, 2), p
    # BASELINE config 4's shards: no K slices below 5120 k per slice; four on the 28672-deep down shard
    p = plan(8192, 1024, 1)
    assert (p["ksplit"], p["waves"], p["u"]) == (1, 8, 4), p
    assert plan(8192, 128, 1)["ksplit"] == 1 and plan(28672, 1024, 1)["ksplit"] == 4 and plan(4096, 1376, 1)["ksplit"] == 1
    # act-order at 3 - 4 rows from K = 5120 (N >= 4096) leaves the in-kernel gather; 4096-deep layers and narrow shards keep it
    assert plan(5120, 13824, 4, act=True)["kernel"] != "strips" and plan(8192, 8192, 3, act=True)["kernel"] != "strips"
    assert plan(4096, 11008, 4, act=True)["kernel"] == "strips" and plan(8192, 3584, 4, act=True)["kernel"] == "strips" and plan(5120, 13824, 2, act=True)["kernel"] == "strips"
    # the band between decode and prefill on the larger families
    want = {
        (5120, 13824): {16: "stream64", 24: "rows", 48: "panel", 64: "panel", 128: "panel", 384: "wide_sk"},      # wide: one (partial) row panel from 17 rows
        (6656, 17920): {24: "rows", 33: "panel", 64: "panel"},                                                     # 17 .. 32 rows of the wide largest layers: the rows kernel
        (8192, 28672): {24: "rows", 48: "panel", 64: "panel", 96: "tiled", 384: "wide_sk"},
        (13824, 5120): {24: "mid", 48: "rows", 96: "rows", 128: "panel", 192: "panel", 384: "panel"},             # deep: the rows kernel beyond 64 Mi weights at 33 .. 96 rows
        (17920, 6656): {48: "rows", 96: "rows", 128: "tiled", 192: "panel", 320: "wide_sk"},
        (28672, 8192): {48: "rows", 64: "rows", 96: "tiled", 192: "panel", 320: "wide_sk"},
        (14336, 4096): {96: "rows", 128: "rows", 192: "panel"},
        (4096, 14336): {8: "stream64", 24: "panel", 64: "panel", 384: "wide_sk"},                                  # the widest K <= 4096 layers leave the rows kernel at up to 32 rows
        (8192, 8192): {32: "rows", 48: "panel", 80: "panel", 384: "wide_sk"},
        (8192, 3584): {96: "rows"},
        (5120, 5120): {96: "rows", 128: "panel"},
        (8192, 1024): {1024: "panel", 1536: "panel", 2048: "wide_sk"},
    }
    for (K, N), by_m in want.items():
        for M, kern in by_m.items():
            p = plan(K, N, M)
            assert p["kernel"] == kern, (K, N, M, p)
    assert plan(8192, 8192, 8, act=True)["kernel"] == "stream64" and plan(8192, 8192, 17, act=True)["kernel"] == "rows"      # act-order, K >= 8192, up to 16 rows: the 64-column-strip kernel
    assert plan(13824, 5120, 8, bits=3, group_size=32)["kernel"] == "rows"                                                   # 3 bits beyond 64 Mi weights: no 64-column-strip kernel
