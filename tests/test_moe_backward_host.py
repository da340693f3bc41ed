"""CPU: the backward of the mixture-of-experts layers in the C ABI (gptq_moe_backward and its table / workspace / plan entries: exports, argument checks,
workspace formula, plan string), its kernels read off the built code objects (instantiation count, registers, LDS, no scratch; the dequantisation kernel
that paid for them compiled once per dtype), the tests' fp64 oracle of the backward formulas against torch.autograd on a dense fp64 twin, and that a CPU
module under grad keeps the per-expert composition."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402

SYMBOLS = ("gptq_moe_grad_table_bytes", "gptq_moe_build_grad_table", "gptq_moe_backward_workspace_bytes", "gptq_moe_backward",
           "gptq_describe_moe_backward_plan")


def _layer(K, N, bits=4, gs=128, dtype=_lib.GPTQ_F16, act=False):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000          # never dereferenced: validation answers first
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = K, N, bits, min(gs, K) if gs > 0 else K, dtype, 0
    if act:
        L.g_idx, L.qweight_seq, L.perm = 0x2000, 0x3000, 0x4000
    return L


def _moe(E=8, H=256, I=512, **kw):
    layers = [[_layer(H, I, **kw) for _ in range(E)], [_layer(H, I, **kw) for _ in range(E)], [_layer(I, H, **kw) for _ in range(E)]]
    arrs = [(ctypes.POINTER(_lib.GptqLayer) * E)(*[ctypes.pointer(l) for l in ls]) for ls in layers]
    m = _lib.GptqMoe()
    m.E = E
    m.gate, m.up, m.down = (ctypes.addressof(a) for a in arrs)
    m._keep = (layers, arrs)
    return m


def _a256(b):
    return (b + 255) // 256 * 256


def _formula(E, T, topk, H, I, es=2):
    R = T * topk
    tiles = R // 64 + min(E, R)
    return (_lib.WS_HEADER_BYTES + _a256(4 * (E + 1)) + 256 + _a256(16 * tiles) + 2 * _a256(4 * R) + 2 * _a256(R * I * es)
            + _a256(4 * R * ((I + 127) // 128)) + _a256(4 * R * H))


def test_backward_symbols_exported_and_declared_abi_still_8():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert "#define GPTQ_MI355X_ABI_VERSION 8" in header
    assert int(lib.gptq_moe_grad_table_bytes(8)) == 3 * 8 * 32 and int(lib.gptq_moe_grad_table_bytes(0)) == 0


BIG = 1 << 30


@pytest.mark.parametrize("kw,args,code,frag", [
    # (experts, (x, dout, dx, dw, ws, ws_bytes), status, fragment of gptq_last_error)
    (None, (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, BIG), 1, "moe is NULL"),
    (dict(), (0x1000, 0x2000, None, None, 0x5000, BIG), 1, "both NULL"),
    (dict(), (0x1008, 0x2000, 0x3000, 0x4000, 0x5000, BIG), 3, "16-byte aligned"),
    (dict(), (0x1000, 0x2004, 0x3000, 0x4000, 0x5000, BIG), 3, "16-byte aligned"),
    (dict(), (0x1000, 0x2000, 0x3002, 0x4000, 0x5000, BIG), 3, "16-byte aligned"),
    (dict(), (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 4096), 4, "workspace too small"),
    (dict(), (0x1000, 0x2000, 0x3000, 0x4000, None, BIG), 4, "workspace too small"),
    (dict(), (None, 0x2000, 0x3000, 0x4000, 0x5000, BIG), 1, "non-NULL"),
    (dict(), (0x1000, None, 0x3000, 0x4000, 0x5000, BIG), 1, "non-NULL"),
    (dict(bits=3), (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, BIG), 3, "3-bit"),
    (dict(dtype=_lib.GPTQ_F32), (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, BIG), 3, "fp32"),
    (dict(gs=48), (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, BIG), 3, "group_size 48"),
])
def test_backward_argument_checks_answer_before_any_launch(kw, args, code, frag):
    lib = _lib.load()
    m = _moe(**kw) if kw is not None else None
    x, dout, dx, dw, ws, wsb = args
    rc = lib.gptq_moe_backward(ctypes.byref(m) if m is not None else None, 0x6000, 0x7000, x, 0x8000, 0x9000, dout, 9, 2, dx, dw, None, ws, wsb, None)
    assert rc == code, (rc, lib.gptq_last_error())
    assert frag in lib.gptq_last_error().decode()


def test_declined_experts_answer_per_expert_with_the_reason():
    lib = _lib.load()
    for kw, T, topk, frag in ((dict(bits=3), 4, 2, "3-bit"), (dict(dtype=_lib.GPTQ_F32), 4, 2, "fp32"), (dict(), 4, 9, "topk = 9"),
                              (dict(H=2048, I=1344 + 32), 4, 2, "multiples of 64")):
        m = _moe(**kw)
        d = _lib.describe_moe_backward_plan(m, T, topk)
        assert d["path"] == "per_expert" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
        assert int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(m), T, topk)) == 0
    raw = _moe()
    for ls in raw._keep[0]:
        for l in ls:
            l.g_idx = 0x2000                          # raw act-order (no re-sequenced rows): what the forward's grouped path declines, the backward declines
    assert _lib.describe_moe_backward_plan(raw, 4, 2)["path"] == "per_expert"
    assert lib.gptq_moe_build_grad_table(ctypes.byref(_moe(bits=3)), 0x1000, None) == 3
    assert lib.gptq_moe_build_grad_table(ctypes.byref(_moe()), None, None) == 1


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("bits", [4, 8])
def test_workspace_formula_and_plan_string(bits, act):
    lib = _lib.load()
    for E, topk, H, I, dtype in ((8, 2, 256, 512, _lib.GPTQ_F16), (8, 2, 320, 448, _lib.GPTQ_BF16), (60, 4, 2048, 1408, _lib.GPTQ_BF16),
                                 (8, 2, 4096, 14336, _lib.GPTQ_F16), (8, 8, 256, 512, _lib.GPTQ_F16)):
        m = _moe(E, H, I, bits=bits, dtype=dtype, act=act)
        for T in (1, 3, 17, 70, 2048):
            R = T * topk
            assert int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(m), T, topk)) == _formula(E, T, topk, H, I), (E, T, topk, H, I)
            d = _lib.describe_moe_backward_plan(m, T, topk)
            tiles = R // 64 + min(E, R)
            assert d["path"] == "grouped_backward" and d["tiles"] == tiles and d["launches"] == 5, d
            assert d["wg_recompute"] == tiles * (I // 64) and d["wg_down"] == tiles * ((I + 127) // 128) and d["wg_up"] == tiles * ((H + 127) // 128), d
        d0 = _lib.describe_moe_backward_plan(m, 0, topk)
        assert d0["path"] == "grouped_backward" and d0["launches"] == 0 and d0["tiles"] == 0, d0
        # T = 0: nothing is launched, nothing is dereferenced
        assert lib.gptq_moe_backward(ctypes.byref(m), None, None, None, None, None, None, 0, topk, 0x1000, None, None, None, 0, None) == 0
    buf = ctypes.create_string_buffer(512)
    assert lib.gptq_describe_moe_backward_plan(ctypes.byref(_moe()), 17, 2, buf, len(buf)) == 0
    assert re.fullmatch(r"path=grouped_backward tiles=8 launches=5( [a-z_]+=\d+)+", buf.value.decode()), buf.value
    assert lib.gptq_describe_moe_backward_plan(ctypes.byref(_moe()), 17, 2, None, 0) == 1


def test_backward_kernels_in_the_built_code_objects():
    from test_kernel_resources import _kernels
    ks = _kernels()                                     # skips where the LLVM tools or the library are missing
    grad = {n: v for n, v in ks.items() if re.search(r"\d+moe_grad_kernel", n)}
    comb = {n: v for n, v in ks.items() if "moe_grad_combine_kernel" in n}
    assert len(grad) == 2 and len(comb) == 1, (sorted(grad), sorted(comb))       # <f16>, <bf16>: bits, group mode, stage and tile rows are run-time uniform
    for n, v in {**grad, **comb}.items():
        assert (v["spill"] or 0) == 0 and (v["scratch"] or 0) == 0, (n, v)
    for n, v in grad.items():
        assert (v["vgpr"] or 0) + (v["agpr"] or 0) <= 256, (n, v)                # two 4-wave workgroups per CU
        assert (v["lds"] or 0) <= 65536, (n, v)
    assert not any("grad_input_kernel" in n for n in {**grad, **comb})           # test_grad_input_host.py counts the dense kernels by that name
    deq = {n for n in ks if re.search(r"\d+dequant_kernel", n)}
    assert len(deq) == 3, sorted(deq)                   # one per dtype: the packing is a workgroup-uniform switch
    assert len({n for n in ks if "moe_gemm_kernel" in n}) == 2
    assert len(ks) <= 1160, len(ks)


def test_oracle_agrees_with_autograd_on_a_dense_fp64_twin():
    from _moe_backward_oracle import oracle
    E, topk, H, I, T = 4, 2, 64, 128, 9
    gen = torch.Generator().manual_seed(0)
    W1, W3 = (torch.randn((E, H, I), generator=gen, dtype=torch.float64) * 0.2 for _ in range(2))
    W2 = torch.randn((E, I, H), generator=gen, dtype=torch.float64) * 0.2
    x = torch.randn((T, H), generator=gen, dtype=torch.float64)
    dout = torch.randn((T, H), generator=gen, dtype=torch.float64)
    idx = torch.stack([torch.randperm(E, generator=gen)[:topk] for _ in range(T)])
    idx[4, 1] = E                                        # one dropped assignment
    w = torch.rand((T, topk), generator=gen, dtype=torch.float64) + 0.1
    o = oracle(x, idx, w, dout, W1, W3, W2)

    xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = torch.zeros((T, H), dtype=torch.float64)
    gs, us = {}, {}
    for e in range(E):
        tok, j = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        g, u = xa[tok] @ W1[e], xa[tok] @ W3[e]
        g.retain_grad(), u.retain_grad()
        gs[e], us[e] = (g, tok, j), (u, tok, j)
        out = out.index_add(0, tok, ((F.silu(g) * u) @ W2[e]) * wa[tok, j, None])
    out.backward(dout)

    def close(a, b):
        return float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max()))

    assert close(o.dX, xa.grad) and close(o.dw, wa.grad)
    assert float(o.dw[4, 1]) == 0.0 and not bool(o.valid[4, 1]) and int(o.valid.sum()) == T * topk - 1
    for e in gs:
        g, tok, j = gs[e]
        assert close(o.dg[tok, j], g.grad) and close(o.du[tok, j], us[e][0].grad)
    assert not bool(o.dg[4, 1].any()) and not bool(o.du[4, 1].any())


def test_cpu_module_under_grad_keeps_the_per_expert_composition(monkeypatch):
    from autogptq_amd import moe
    q = moe.QuantMoEExperts(4, 64, 128, 4, 32)
    q._switches["backward"] = True                                   # (post_init needs a GPU; the flag alone must not move a CPU call off the composition)
    calls = []
    monkeypatch.setattr(moe, "_per_expert", lambda experts, x, idx, w: (calls.append(x.shape), x * 1.0)[1])
    x = torch.zeros((3, 64), dtype=torch.float16, requires_grad=True)
    idx = torch.zeros((3, 2), dtype=torch.int64)
    w = torch.full((3, 2), 0.5, requires_grad=True)
    out = moe.moe_forward(q, x, idx, w)
    assert calls == [(3, 64)] and out.shape == (3, 64)
    assert q.last_plan["path"] == "per_expert" and "backward" not in q.last_plan
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        q.post_init(backward=True)
