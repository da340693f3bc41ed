"""CPU: GPTQ_MOE_LOW_BIT in gptq_moe_t.flags -- the grouped path (forward and backward plans, workspace) takes 2- and 3-bit experts with the flag and
declines them exactly as before without it; the decode and batch plans decline them whatever the flag says."""
import ctypes
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402
from test_moe_host import _layer, _moe  # noqa: E402

LOW = _lib.MOE_LOW_BIT


def _flagged(flags=LOW, **kw):
    m = _moe(**kw)
    m.flags = flags
    return m


def _mixed(bits_gu, bits_down, E=8, H=256, I=512, flags=LOW):
    layers = [[_layer(H, I, bits=bits_gu) for _ in range(E)], [_layer(H, I, bits=bits_gu) for _ in range(E)], [_layer(I, H, bits=bits_down) for _ in range(E)]]
    arrs = [(ctypes.POINTER(_lib.GptqLayer) * E)(*[ctypes.pointer(l) for l in ls]) for ls in layers]
    m = _lib.GptqMoe()
    m.E, m.flags = E, flags
    m.gate, m.up, m.down = (ctypes.addressof(a) for a in arrs)
    m._keep = (layers, arrs)
    return m


def test_header_and_binding_agree_on_the_flag():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    assert "#define GPTQ_MOE_LOW_BIT 1" in header and LOW == 1
    assert [f[0] for f in _lib.GptqMoe._fields_] == ["E", "flags", "gate", "up", "down"]
    assert _lib.GptqMoe().flags == 0


@pytest.mark.parametrize("gs", [32, 128, 256])
@pytest.mark.parametrize("bits", [2, 3])
def test_forward_plan_and_workspace_with_the_flag(bits, gs):
    lib = _lib.load()
    m = _flagged(bits=bits, gs=gs)          # gs 256 = K of gate / up: one group
    m4 = _moe(bits=4, gs=gs)
    for T in (1, 7, 64, 300):
        d = _lib.describe_moe_plan(m, T, 2)
        assert d["path"] == "grouped" and d["bn"] == 64 and d["launches"] == 4, d
        assert d == _lib.describe_moe_plan(m4, T, 2)
        got = int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), T, 2))
        assert got > 0 and got == int(lib.gptq_moe_workspace_bytes(ctypes.byref(m4), T, 2))
    assert _lib.describe_moe_plan(m, 0, 2)["launches"] == 0


@pytest.mark.parametrize("E,topk,H,I,dtype", [(8, 2, 4096, 14336, _lib.GPTQ_F16), (60, 4, 2048, 1408, _lib.GPTQ_BF16)])
def test_workspace_equals_the_4_bit_value(E, topk, H, I, dtype):
    lib = _lib.load()
    for bits in (2, 3):
        m, m4 = _flagged(E=E, H=H, I=I, bits=bits, dtype=dtype), _moe(E, H, I, bits=4, dtype=dtype)
        for T in (0, 1, 64, 2048):
            assert int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), T, topk)) == int(lib.gptq_moe_workspace_bytes(ctypes.byref(m4), T, topk))
            assert int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(m), T, topk)) == int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(m4), T, topk))


@pytest.mark.parametrize("bits", [2, 3])
def test_backward_plan_with_the_flag(bits):
    lib = _lib.load()
    m = _flagged(bits=bits)
    d = _lib.describe_moe_backward_plan(m, 70, 2)
    assert d["path"] == "grouped_backward" and d["launches"] == 5, d
    assert d == _lib.describe_moe_backward_plan(_moe(bits=4), 70, 2)
    assert int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(m), 70, 2)) > 0


def test_mixed_widths():
    assert _lib.describe_moe_plan(_mixed(3, 4), 1, 2)["path"] == "grouped"
    assert _lib.describe_moe_plan(_mixed(4, 2), 1, 2)["path"] == "grouped"
    assert _lib.describe_moe_backward_plan(_mixed(3, 4), 1, 2)["path"] == "grouped_backward"
    d = _lib.describe_moe_plan(_mixed(3, 4, flags=0), 1, 2)
    assert d["path"] == "per_expert" and "3-bit" in d["reason"], d
    d = _lib.describe_moe_plan(_mixed(4, 2, flags=0), 1, 2)
    assert d["path"] == "per_expert" and "2-bit" in d["reason"], d
    # gate and up still share their width
    m = _mixed(3, 4)
    for l in m._keep[0][1]:
        l.bits = 2
    d = _lib.describe_moe_plan(m, 1, 2)
    assert d["path"] == "per_expert" and "gate and up" in d["reason"].replace("_", " "), d


@pytest.mark.parametrize("bits,frag", [(3, "3-bit"), (2, "2-bit")])
def test_decode_and_batch_plans_decline_whatever_the_flag_says(bits, frag):
    lib = _lib.load()
    for flags in (0, LOW):
        m = _flagged(flags=flags, bits=bits)
        d = _lib.describe_moe_decode_plan(m, 1, 2)
        assert d["path"] == "none" and frag in d["reason"] and "decode_path" in d["reason"], d
        b = _lib.describe_moe_batch_plan(m, 8, 2)
        assert b["path"] == "none" and frag in b["reason"] and "batch_path" in b["reason"], b
        assert int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), 1, 2)) == 0
        assert int(lib.gptq_moe_batch_workspace_bytes(ctypes.byref(m), 8, 2)) == 0


def test_other_widths_and_unknown_flags_decline():
    lib = _lib.load()
    for flags in (0, LOW):
        m = _flagged(flags=flags, bits=5)
        assert _lib.describe_moe_plan(m, 1, 2)["path"] == "per_expert"
        assert _lib.describe_moe_backward_plan(m, 1, 2)["path"] == "per_expert"
        assert int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), 1, 2)) == 0
    for flags in (2, LOW | 4, -1):
        for bits in (3, 4):
            m = _flagged(flags=flags, bits=bits)
            d = _lib.describe_moe_plan(m, 1, 2)
            assert d["path"] == "per_expert" and "flag" in d["reason"], d
            assert _lib.describe_moe_backward_plan(m, 1, 2)["path"] == "per_expert"
            assert int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), 1, 2)) == 0
            rc = lib.gptq_moe_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, 1, 2, 0x1000, None, 0x1000, 1 << 30, None)
            assert rc == 3 and "flag" in lib.gptq_last_error().decode()
            assert lib.gptq_moe_build_table(ctypes.byref(m), 0x1000, None) == 3


@pytest.mark.parametrize("bits", [2, 3])
def test_without_the_flag_the_refusal_is_the_one_it_was(bits):
    lib = _lib.load()
    m = _moe(bits=bits)
    assert m.flags == 0
    want = f"{bits}-bit experts: the grouped path takes 4 or 8 bits"
    d = _lib.describe_moe_plan(m, 1, 2)
    assert d == {"path": "per_expert", "reason": want.replace(" ", "_")}, d
    assert _lib.describe_moe_backward_plan(m, 1, 2) == d
    assert int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), 1, 2)) == 0
    assert int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(m), 1, 2)) == 0
    rc = lib.gptq_moe_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, 1, 2, 0x1000, None, 0x1000, 1 << 30, None)
    assert rc == 3 and lib.gptq_last_error().decode() == want


def test_python_signatures_carry_the_switch():
    from autogptq_amd.model_utils import autogptq_post_init
    from autogptq_amd.moe import QuantMoEExperts
    p = inspect.signature(QuantMoEExperts.post_init).parameters
    assert list(p)[:5] == ["self", "decode_copy", "batch", "backward", "low_bit"] and p["low_bit"].default is False
    p = inspect.signature(autogptq_post_init).parameters
    assert p["expert_low_bit"].default is False
    assert QuantMoEExperts(2, 256, 512, 3, 128)._switches["low_bit"] is False
