"""CPU (-m "not gpu"): the two host-checkable halves of the memory contract.

* tests/_guarded.py, the guard-band buffer of test_gpu_memory_contract.py: a byte poked into either guard, at the first and at the last guard position, is
  reported with the right side and body-relative offset; an untouched buffer passes.
* The alignment contract of the dense entry points (include/gptq_mi355x.h): x, out / outs[i] and workspace at an address = 2 (mod 16) are refused with
  GPTQ_ERR_UNSUPPORTED before anything else happens to them (fake pointers, never dereferenced, as test_host_logic.py does); the aligned call gets past
  that check (it is refused later, for a missing workspace, still before any launch)."""
import ctypes

import pytest
import torch

import _guarded as G
from autogptq_amd import _lib

UNSUPPORTED, WORKSPACE = 3, 4


# ---------------------------------------------------------------------------------------------------------------- the helper
@pytest.mark.parametrize("nbytes", [0, 2, 1000, 4096])
def test_guarded_layout_and_untouched_buffer_passes(nbytes):
    g = G.Guarded(nbytes, 512, 0xFF, G.OUT_GUARD)
    assert g.ptr % 256 == 0 and g.body.numel() == nbytes and (nbytes == 0 or g.body.data_ptr() == g.ptr)
    assert g.high.data_ptr() == g.ptr + nbytes                                  # the high guard begins at byte nbytes exactly
    assert g.low.numel() >= 512 and g.high.numel() >= 512
    assert bool((g.body == 0xFF).all()) and bool((g.low == 0xA5).all()) and bool((g.high == 0xA5).all())
    g.body.fill_(7)                                                             # writing the whole body is not damage
    g.assert_intact("untouched")
    assert g.damage() == []
    if nbytes >= 4:
        v = g.view(torch.float16, (nbytes // 2,))
        assert v.data_ptr() == g.ptr and v.numel() == nbytes // 2


@pytest.mark.parametrize("nbytes", [2, 1000])
def test_guarded_reports_side_and_offsets(nbytes):
    def poked(*at):
        g = G.Guarded(nbytes, 512, 0x00, G.OUT_GUARD)
        flat = g.raw
        for off in at:                                                          # body-relative byte offsets
            flat[g.start + off] = 0x11
        return g
    # first and last position of the high guard
    g = poked(nbytes)
    assert g.damage() == [("high", nbytes, nbytes, 1)]
    with pytest.raises(AssertionError, match=rf"out: high guard damaged: 1 byte\(s\), first at body offset {nbytes}, last at body offset {nbytes} "):
        g.assert_intact("out")
    g = poked()
    g.raw[-1] = 0x11
    last_high = nbytes + g.high.numel() - 1
    assert g.damage() == [("high", last_high, last_high, 1)]
    # first (next to the body) and last (the allocation's first byte) position of the low guard
    assert poked(-1).damage() == [("low", -1, -1, 1)]
    g = poked()
    g.raw[0] = 0x11
    assert g.damage() == [("low", -g.start, -g.start, 1)] and g.start >= 512
    # a 2-byte overrun behind the body plus a stray store far below it: both sides, first / last / count
    g = poked(nbytes, nbytes + 1, -300, -7)
    assert g.damage() == [("low", -300, -7, 2), ("high", nbytes, nbytes + 1, 2)]
    with pytest.raises(G.GuardDamage, match="low guard damaged: 2 byte"):
        g.assert_intact("ws")


def test_guarded_input_fill_is_nan_and_minus_one():
    g = G.Guarded(64, 256, 0x00, G.IN_GUARD)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        assert bool(g.high[:64].view(dt).isnan().all())
    assert bool((g.high[:64].view(torch.int64) == -1).all())
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    gb, v = G.guarded_like(t, 256)
    assert torch.equal(v, t) and gb.nbytes == 48 and v.data_ptr() == gb.ptr
    gb.assert_intact("x")
    assert G.guard_for(2 * 96) == 64 << 10 and G.guard_for(2 * 16384) == 128 * 2 * 16384


# ---------------------------------------------------------------------------------------------------------------- alignment
def _layer(**kw):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000          # never dereferenced: every call below is refused before a launch
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = 4096, 32, 4, 128, 0, 0
    for k, v in kw.items():
        setattr(L, k, v)
    return L


A, ODD, BIG = 0x10000, 0x10002, 1 << 30


def _err():
    return _lib.load().gptq_last_error().decode()


@pytest.mark.parametrize("entry", ["gptq_forward", "gptq_forward_ex", "gptq_gemv", "gptq_gemm"])
@pytest.mark.parametrize("M", [1, 16])
def test_single_layer_entries_refuse_misaligned_pointers(entry, M):
    lib = _lib.load()
    L = _layer()
    assert lib.gptq_workspace_bytes(ctypes.byref(L), M) > 0          # a tiny N forces K slices: the aligned call stops at "workspace too small", no launch
    fn = getattr(lib, entry)
    tail = () if entry == "gptq_forward" else (None,)
    for x, out, ws in ((ODD, A, A), (A, ODD, A), (A, A, ODD)):
        assert fn(ctypes.byref(L), x, out, M, ws, BIG, None, *tail) == UNSUPPORTED
        assert "x / out / workspace must be 16-byte aligned" in _err()
    assert fn(ctypes.byref(L), A, A, M, None, 0, None, *tail) == WORKSPACE and "workspace too small" in _err()
    assert fn(ctypes.byref(L), A, A, M, A, 65536, None, *tail) == WORKSPACE


@pytest.mark.parametrize("ex", [False, True])
def test_forward_multi_refuses_misaligned_pointers(ex):
    lib = _lib.load()
    Ls = [_layer(), _layer(N=64)]
    arr = (ctypes.POINTER(_lib.GptqLayer) * 2)(*[ctypes.pointer(l) for l in Ls])
    M = 1
    assert lib.gptq_workspace_bytes_multi(arr, 2, M) > 0
    fn = lib.gptq_forward_multi_ex if ex else lib.gptq_forward_multi
    tail = (None,) if ex else ()

    def call(x, o0, o1, ws, wsb):
        outs = (ctypes.c_void_p * 2)(o0, o1)
        return fn(arr, 2, x, outs, M, ws, wsb, None, *tail)
    assert call(ODD, A, A, A, BIG) == UNSUPPORTED and "x / out / workspace must be 16-byte aligned" in _err()
    assert call(A, A, A, ODD, BIG) == UNSUPPORTED and "x / out / workspace must be 16-byte aligned" in _err()
    assert call(A, ODD, A, A, BIG) == UNSUPPORTED and "outs[0] must be 16-byte aligned" in _err()
    assert call(A, A, ODD, A, BIG) == UNSUPPORTED and "outs[1] must be 16-byte aligned" in _err()
    assert call(A, A, A, None, 0) == WORKSPACE and "workspace too small" in _err()


@pytest.mark.parametrize("ex", [False, True])
def test_mlp_forward_refuses_misaligned_pointers(ex):
    lib = _lib.load()
    gate, up, down = _layer(K=256, N=512), _layer(K=256, N=512), _layer(K=512, N=256)
    M = 3
    assert lib.gptq_workspace_bytes_mlp(ctypes.byref(gate), ctypes.byref(up), ctypes.byref(down), M) > 0      # (the staging rows: every call needs a workspace)
    fn = lib.gptq_mlp_forward_ex if ex else lib.gptq_mlp_forward
    tail = (None,) if ex else ()
    for x, out, ws in ((ODD, A, A), (A, ODD, A), (A, A, ODD)):
        assert fn(ctypes.byref(gate), ctypes.byref(up), ctypes.byref(down), x, out, M, ws, BIG, None, *tail) == UNSUPPORTED
        assert "x / out / workspace must be 16-byte aligned" in _err()
    assert fn(ctypes.byref(gate), ctypes.byref(up), ctypes.byref(down), A, A, M, None, 0, None, *tail) == WORKSPACE


def test_forward_scatter_and_gather_refuse_misaligned_pointers():
    lib = _lib.load()
    L = _layer(K=256, N=256)
    pg = _lib.GptqPeerGroup()
    pg.world, pg.rank, pg.rows_max, pg.N = 1, 0, 4, 256
    pg.xbuf[0][0] = pg.xbuf[1][0] = pg.flags[0] = pg.state = A
    for x, ws in ((ODD, A), (A, ODD)):
        assert lib.gptq_forward_scatter(ctypes.byref(L), x, 1, ctypes.byref(pg), ws, BIG, None) == UNSUPPORTED
        assert "x / out / workspace must be 16-byte aligned" in _err()
    for x, out, ws in ((ODD, A, A), (A, ODD, A), (A, A, ODD)):
        assert lib.gptq_forward_gather(ctypes.byref(L), x, out, 1, ctypes.byref(pg), 100, ws, BIG, None) == UNSUPPORTED
        assert "x / out / workspace must be 16-byte aligned" in _err()
    # aligned: past the alignment check (this layer carries no decode copy, which is what the entry then says; no launch)
    assert lib.gptq_forward_scatter(ctypes.byref(L), A, 1, ctypes.byref(pg), A, BIG, None) == UNSUPPORTED
    assert "16-byte aligned" not in _err() and "decode-copy kernel" in _err()
    assert lib.gptq_forward_gather(ctypes.byref(L), A, A, 1, ctypes.byref(pg), 100, A, BIG, None) == UNSUPPORTED
    assert "16-byte aligned" not in _err()
