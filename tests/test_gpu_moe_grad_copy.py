"""GPU: the backward of the routed experts on their decode copy (gptq_moe_backward_ex with GPTQ_GRAD_ON_COPY: the grouped mode of grad_copy_kernel,
csrc/moe_grad_copy.cuh; opt-in through the attribute QuantMoEExperts.backward_on_copy = True before post_init(backward=True)).

Reference and bounds: test_gpu_moe_backward.check_backward -- the fp64 oracle with the propagated per-output bounds, unchanged -- run on the copy form's
outputs.  E = 3, topk = 2, H = 384 (three chunks of the gate | up copies), I = 192 (a partial last chunk of the down copies); T = 130 gives every expert a
full 64-row tile and a partial one, T = 1 leaves an expert without rows, T = 65 carries two indices outside [0, E)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_moe_backward as B  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.moe import moe_forward  # noqa: E402
from test_gpu_moe import DEV, _routing, make_experts  # noqa: E402

pytestmark = pytest.mark.gpu
F = _lib.GRAD_ON_COPY
E, TOPK, H, I = 3, 2, 384, 192
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
ACT = pytest.mark.parametrize("act", [False, True], ids=["plain", "act"])


def _experts(gs, act, dtype, bits=4, seed=0, same_order=False):
    q = make_experts(E, H, I, bits, gs, act, dtype, seed=seed, top_k=TOPK)
    if same_order:                                  # gate and up of one g_idx, as a GPTQ checkpoint has them (the order comes from their common input)
        for e in range(E):
            gate, up, _ = q[e].layers()
            up.g_idx = gate.g_idx.clone()
    q.backward_on_copy = True
    q.post_init(backward=True)
    assert q._grad_table is not None and q._decode_table is not None
    return q


def _inputs(T, dtype, invalid=False):
    idx, w = _routing(T, E, TOPK, T + E)
    if invalid:
        idx[3, 0], idx[5, 1] = E, -1
    return B._rand(T, H, dtype, T), idx, w, B._rand(T, H, dtype, 100 + T)


def run_copy(q, x, idx, w, dout, want_dx=True, want_dw=True, want_dgu=True, flags=F):
    """run_backward of test_gpu_moe_backward.py through gptq_moe_backward_ex: the same tuple."""
    lib = _lib.load()
    T, topk = idx.shape
    R, es = T * topk, B._es(x.dtype)
    need = int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(q._moe), T, topk))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    dx = torch.full((T, H), float("nan"), dtype=x.dtype, device=DEV) if want_dx else None
    dw = torch.full((T, topk), float("nan"), dtype=torch.float32, device=DEV) if want_dw else None
    dgu = torch.zeros(2 * R * I * es + 4 * R, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gptq_moe_backward_ex(ctypes.byref(q._moe), q._table.data_ptr(), q._grad_table.data_ptr(), q._decode_table.data_ptr(), x.data_ptr(),
                                        idx.data_ptr(), w.data_ptr(), dout.data_ptr(), T, topk, _lib.ptr(dx), _lib.ptr(dw), dgu.data_ptr(), ws.data_ptr(),
                                        need, flags, B._stream()))
    gb = R * I * es
    return dx, dw, dgu[:gb].view(x.dtype).view(R, I), dgu[gb:2 * gb].view(x.dtype).view(R, I), dgu[2 * gb:].view(torch.int32).view(T, topk)


def _plan(q, T=130):
    return _lib.describe_moe_backward_plan_ex(q._moe, T, TOPK, F)


@pytest.mark.parametrize("gs", [32, 64, 128, -1])
@ACT
@DTYPES
def test_fp64_oracle_with_the_propagated_bounds(monkeypatch, dtype, act, gs):
    q = _experts(gs, act, dtype, seed=gs + 7)
    d = _plan(q)
    assert d["path"] == "grouped_backward_copy" and d["gm"] == {32: 2, 64: 1}.get(gs, 0) and d["act"] == int(act and gs > 0), d
    assert d["launches"] == 4 + d["up_launches"] and d["up_launches"] == 1 + d["act"], d      # (make_experts draws an order per layer: gate and up differ)
    monkeypatch.setattr(B, "run_backward", run_copy)
    for T in (1, 65, 130):
        args = _inputs(T, dtype, invalid=T == 65)
        dx, dw = B.check_backward(q, *args)
        again = run_copy(q, *args)
        assert torch.equal(dx, again[0]) and torch.equal(dw, again[1])


@ACT
def test_same_bits_as_the_rows_backward(monkeypatch, act):
    """dg, du, dX bit for bit: every element sums its reduction axis in the rows form's stage order, and the scalar epilogue is the rows form's."""
    dtype = torch.bfloat16 if act else torch.float16
    q = _experts(128, act, dtype, seed=3)
    args = _inputs(130, dtype)
    rows, copy = B.run_backward(q, *args), run_copy(q, *args)
    for nm, a, b in zip(("dx", "dw", "dg", "du", "pos"), rows, copy):
        if nm != "dw":                              # (dw: the bound of check_backward here, its bits in the test below)
            assert torch.equal(a, b), nm
    monkeypatch.setattr(B, "run_backward", run_copy)
    B.check_backward(q, *args)
    assert all(torch.equal(a, b) for a, b in zip(rows, run_copy(q, *args, flags=0)))      # flags = 0: the rows backward


def test_dw_of_plain_experts_has_the_bits_of_the_rows_backward():
    """fp32 sums of 192 products of either sign, so one product rounded the other way shows: the copy form's down-stage epilogue writes out the fusing
    and the T(a * b) forms of moe_grad_kernel's object code (moe_grad_copy.cuh)."""
    dtype = torch.float16
    q = _experts(128, False, dtype, seed=3)
    args = _inputs(130, dtype)
    rows, copy = B.run_backward(q, *args)[1], run_copy(q, *args)[1]
    print(f"dw: {int((rows != copy).sum())} of {rows.numel()} differ, max |diff| {float((rows - copy).abs().max()):.3e}, max |dw| {float(rows.abs().max()):.3e}")
    assert torch.equal(rows, copy)


def test_split_and_shared_up_stage_perms(monkeypatch):
    dtype = torch.float16
    q = _experts(64, True, dtype, seed=5, same_order=True)          # post_init pointed up's perm at gate's
    assert _plan(q)["up_launches"] == 1 and _plan(q)["launches"] == 5
    args = _inputs(130, dtype)
    monkeypatch.setattr(B, "run_backward", run_copy)
    dx1, dw1 = B.check_backward(q, *args)
    keep = []
    for e in range(E):                              # the same content behind a pointer of its own: W1 and W3 in two launches
        gate, up, _ = q[e].layers()
        keep.append(gate._perm.clone())
        up._layer.perm = keep[-1].data_ptr()
    _lib.check(_lib.load().gptq_moe_build_decode_table(ctypes.byref(q._moe), q._decode_table.data_ptr(), B._stream()))
    assert _plan(q)["up_launches"] == 2 and _plan(q)["launches"] == 6
    dx2, dw2 = B.check_backward(q, *args)
    assert torch.equal(dx1, dx2) and torch.equal(dw1, dw2)


def test_autograd_reaches_it_and_declined_experts_keep_the_rows(caplog):
    dtype, T = torch.float16, 65
    q = _experts(128, True, dtype, seed=9)
    x0, idx, w0, dout = _inputs(T, dtype)
    x, w = x0.clone().requires_grad_(), w0.clone().requires_grad_()
    moe_forward(q, x, idx, w).backward(dout)
    assert q.last_plan["backward"] == "grouped_copy", q.last_plan
    dx, dw = run_copy(q, x0, idx, w0, dout)[:2]
    assert torch.equal(x.grad, dx) and torch.equal(w.grad, dw)
    with caplog.at_level("WARNING"):
        q8 = _experts(128, False, dtype, bits=8, seed=9)
    assert "backward_on_copy = True" in caplog.text and "bits" in caplog.text
    assert _plan(q8)["path"] == "grouped_backward" and _plan(q8)["copy_reason"] == "bits"
    x, w = x0.clone().requires_grad_(), w0.clone().requires_grad_()
    moe_forward(q8, x, idx, w).backward(dout)
    assert q8.last_plan["backward"] == "grouped", q8.last_plan
    dx, dw = B.run_backward(q8, x0, idx, w0, dout)[:2]
    assert torch.equal(x.grad, dx) and torch.equal(w.grad, dw) and torch.equal(dx, run_copy(q8, x0, idx, w0, dout)[0])


def test_guard_band():
    dtype, T, PAD = torch.float16, 65, 4096
    q = _experts(32, True, dtype, seed=13)
    x, idx, w, dout = _inputs(T, dtype, invalid=True)
    ref = run_copy(q, x, idx, w, dout)
    lib = _lib.load()
    need = int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(q._moe), T, TOPK))
    dxb = torch.full((2 * PAD + T * H,), -3.0, dtype=dtype, device=DEV)
    dwb = torch.full((2 * PAD + T * TOPK,), 7.0, dtype=torch.float32, device=DEV)
    wsb = torch.full((2 * PAD + need,), 0x5A, dtype=torch.uint8, device=DEV)
    dx, dw, ws = dxb[PAD:PAD + T * H].view(T, H), dwb[PAD:PAD + T * TOPK].view(T, TOPK), wsb[PAD:PAD + need]
    _lib.check(lib.gptq_moe_backward_ex(ctypes.byref(q._moe), q._table.data_ptr(), None, q._decode_table.data_ptr(), x.data_ptr(), idx.data_ptr(),
                                        w.data_ptr(), dout.data_ptr(), T, TOPK, dx.data_ptr(), dw.data_ptr(), None, ws.data_ptr(), need, F, B._stream()))
    assert torch.equal(dx, ref[0]) and torch.equal(dw, ref[1])      # (no grad_table: the copy form reads no checkpoint row in its two stages)
    for buf, n, v in ((dxb, T * H, -3.0), (dwb, T * TOPK, 7.0), (wsb, need, 0x5A)):
        assert bool((buf[:PAD] == v).all()) and bool((buf[PAD + n:] == v).all())
