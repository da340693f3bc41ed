"""CPU: GPTQ_MOE_LOW_BIT_DECODE in gptq_moe_t.flags -- with the flag the decode plan (1..4 tokens on the decode copy) takes 2- and 3-bit experts and
answers as it does for 4-bit experts of the same shape; without it every entry point answers as before; the grouped and backward plans ignore the bit;
the batch, the prefill and the fused shared-expert plans decline 2 / 3 bits whatever the flags say.  Read off the built library: no kernel was added."""
import ctypes
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402
from test_moe_decode_host import _a256, _layer, _moe  # noqa: E402

LOW = 1
DEC = getattr(_lib, "MOE_LOW_BIT_DECODE", 8)          # (the parent has no such name: the tests below then fail on what the library answers)

SHAPES = [(8, 2, 256, 512, _lib.GPTQ_F16), (4, 2, 320, 448, _lib.GPTQ_BF16), (60, 4, 2048, 1408, _lib.GPTQ_BF16), (8, 2, 4096, 14336, _lib.GPTQ_F16)]


def _flagged(flags, *a, **kw):
    m = _moe(*a, **kw)
    m.flags = flags
    return m


def test_header_and_binding_agree_on_the_flag():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    assert "#define GPTQ_MOE_LOW_BIT_DECODE 8" in header and "#define GPTQ_MOE_LOW_BIT 1" in header
    assert _lib.MOE_LOW_BIT_DECODE == 8 and _lib.MOE_LOW_BIT == 1
    assert _lib.load().gptq_abi_version() == 8          # an additive flag: the ABI number stays, as it did for GPTQ_MOE_LOW_BIT


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [32, 64, 128, -1])
@pytest.mark.parametrize("flags", [DEC, DEC | LOW])
@pytest.mark.parametrize("bits", [2, 3])
def test_decode_plan_and_workspace_with_the_flag(bits, flags, gs, act):
    """The plan string has no key that chunk bytes enter: 2, 3 and 4 bits share 128 k per chunk and 48-byte constant records, so waves and LDS bytes are
    those of the 4-bit plan -- EVERY key is compared (chunk bytes, 64 words-per-lane 4, are a template constant of the kernel)."""
    lib = _lib.load()
    for E, topk, H, I, dtype in SHAPES:
        if gs > 0 and (H % gs or I % gs):          # (320 x 448 with groups of 128: not a shape of this grid)
            continue
        m = _flagged(flags, E, H, I, bits=bits, gs=gs, dtype=dtype, act=act)
        m4 = _moe(E, H, I, bits=4, gs=gs, dtype=dtype, act=act)
        for T in (1, 2, 3, 4):
            d = _lib.describe_moe_decode_plan(m, T, topk)
            assert d["path"] == "decode" and d["launches"] == 2, d
            assert d == _lib.describe_moe_decode_plan(m4, T, topk), d
            assert d["wg_pair"] == T * topk * I // 16 and d["wg_down"] == T * H // 16, d
            got = int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), T, topk))
            assert got > 0 and got == int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m4), T, topk))
            assert got == _lib.WS_HEADER_BYTES + _a256(T * topk * I * 2) + _a256(4 * T * topk)
        d0 = _lib.describe_moe_decode_plan(m, 0, topk)
        assert d0["path"] == "decode" and d0["launches"] == 0, d0
        assert lib.gptq_moe_decode_forward(ctypes.byref(m), None, None, None, None, 0, topk, None, None, None, 0, None) == 0
        d5 = _lib.describe_moe_decode_plan(m, 5, topk)
        assert d5["path"] == "none" and "T___5" in d5["reason"], d5
        assert int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), 5, topk)) == 0
    assert int(lib.gptq_moe_decode_table_bytes(8)) == 3 * 8 * 32


@pytest.mark.parametrize("flags", [DEC, DEC | LOW])
@pytest.mark.parametrize("bits", [2, 3])
def test_batch_and_prefill_plans_decline_whatever_the_flags_say(bits, flags):
    lib = _lib.load()
    m = _flagged(flags, bits=bits)
    b = _lib.describe_moe_batch_plan(m, 8, 2)
    assert b == {"path": "none", "reason": f"{bits}-bit_experts:_the_batch_path_takes_4_or_8_bits"}, b
    p = _lib.describe_moe_prefill_plan(m, 65, 2)
    assert p == {"path": "none", "reason": f"{bits}-bit_experts:_the_prefill_path_takes_4_or_8_bits"}, p
    assert int(lib.gptq_moe_batch_workspace_bytes(ctypes.byref(m), 8, 2)) == 0
    assert int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(m), 65, 2)) == 0


@pytest.mark.parametrize("flags", [0, LOW])
@pytest.mark.parametrize("bits", [2, 3])
def test_without_the_flag_the_decode_refusal_is_the_one_it_was(bits, flags):
    lib = _lib.load()
    m = _flagged(flags, bits=bits)
    want = f"{bits}-bit experts: the decode path takes 4 or 8 bits"
    assert _lib.describe_moe_decode_plan(m, 1, 2) == {"path": "none", "reason": want.replace(" ", "_")}
    assert int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), 1, 2)) == 0
    rc = lib.gptq_moe_decode_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, 1, 2, 0x1000, None, 0x1000, 1 << 30, None)
    assert rc == 3 and lib.gptq_last_error().decode() == want
    assert lib.gptq_moe_build_decode_table(ctypes.byref(m), 0x1000, None) == 3


def test_other_widths_decline_with_the_flag():
    m = _flagged(DEC, bits=5)
    d = _lib.describe_moe_decode_plan(m, 1, 2)
    assert d["path"] == "none" and "got_5" in d["reason"], d          # (the layer check's own refusal, as without the flag)


@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_the_grouped_and_backward_plans_ignore_the_bit(bits):
    """flags 8 answers as flags 0 (2 / 3 bits declined with the message it was), flags 9 as flags 1; bits 2 and 4 stay unknown."""
    lib = _lib.load()
    for flag, same_as in ((DEC, 0), (DEC | LOW, LOW)):
        m, ref = _flagged(flag, bits=bits), _flagged(same_as, bits=bits)
        for T in (1, 70):
            assert _lib.describe_moe_plan(m, T, 2) == _lib.describe_moe_plan(ref, T, 2)
            assert _lib.describe_moe_backward_plan(m, T, 2) == _lib.describe_moe_backward_plan(ref, T, 2)
            assert int(lib.gptq_moe_workspace_bytes(ctypes.byref(m), T, 2)) == int(lib.gptq_moe_workspace_bytes(ctypes.byref(ref), T, 2))
            assert int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(m), T, 2)) == int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(ref), T, 2))
    if bits in (2, 3):
        d = _lib.describe_moe_plan(_flagged(DEC, bits=bits), 1, 2)
        assert d == {"path": "per_expert", "reason": f"{bits}-bit_experts:_the_grouped_path_takes_4_or_8_bits"}, d
        assert _lib.describe_moe_plan(_flagged(DEC | LOW, bits=bits), 1, 2)["path"] == "grouped"
    for flags in (2, 4, DEC | 2, DEC | 4, 16):
        d = _lib.describe_moe_plan(_flagged(flags, bits=bits), 1, 2)
        assert d["path"] == "per_expert" and "unknown_flag" in d["reason"], d


def _mixed(bits_gu, bits_down, flags, E=8, H=256, I=512):
    layers = [[_layer(H, I, bits=bits_gu) for _ in range(E)], [_layer(H, I, bits=bits_gu) for _ in range(E)], [_layer(I, H, bits=bits_down) for _ in range(E)]]
    arrs = [(ctypes.POINTER(_lib.GptqLayer) * E)(*[ctypes.pointer(l) for l in ls]) for ls in layers]
    m = _lib.GptqMoe()
    m.E, m.flags = E, flags
    m.gate, m.up, m.down = (ctypes.addressof(a) for a in arrs)
    m._keep = (layers, arrs)
    return m


@pytest.mark.parametrize("gu,down", [(3, 4), (3, 2), (4, 3), (2, 3)])
def test_mixed_widths_decline_on_the_decode_path(gu, down):
    d = _lib.describe_moe_decode_plan(_mixed(gu, down, DEC | LOW), 1, 2)
    assert d["path"] == "none" and "the_down_layers_of_all_experts_must_share_bits" in d["reason"], d
    m = _mixed(3, 3, DEC)
    for l in m._keep[0][1]:
        l.bits = 2
    d = _lib.describe_moe_decode_plan(m, 1, 2)
    assert d["path"] == "none" and "the_up_layers_of_all_experts_must_share_bits" in d["reason"], d


@pytest.mark.parametrize("bits", [2, 3])
def test_the_other_rules_of_the_decode_plan_stay(bits):
    for kw, T, topk, frag in ((dict(copy=False), 1, 2, "no_decode_copy"), (dict(dtype=_lib.GPTQ_F32), 1, 2, "fp32"), (dict(), 1, 9, "topk___9"),
                              (dict(gs=48), 1, 2, "group_size"), (dict(E=257), 1, 2, "E___257"), (dict(H=288), 1, 2, "multiples_of_64")):
        d = _lib.describe_moe_decode_plan(_flagged(DEC, bits=bits, **kw), T, topk)
        assert d["path"] == "none" and frag in d["reason"], (kw, d)


@pytest.mark.parametrize("flags", [DEC, DEC | LOW])
@pytest.mark.parametrize("bits", [2, 3])
def test_the_shared_decode_plan_declines_low_bit_routed_experts(bits, flags):
    from test_moe_shared_host import _shared
    lib = _lib.load()
    m = _flagged(flags, bits=bits)
    assert _lib.describe_moe_decode_plan(m, 1, 2)["path"] == "decode"
    for sh in (_shared(bits=bits), _shared(bits=4)):
        d = _lib.describe_moe_shared_decode_plan(m, sh, 1, 2)
        assert d["path"] == "none" and f"{bits}-bit_routed_experts" in d["reason"] and "shared_decode_form" in d["reason"], d
        assert int(lib.gptq_moe_shared_decode_workspace_bytes(ctypes.byref(m), ctypes.byref(sh), 1, 2)) == 0
        rc = lib.gptq_moe_shared_decode_forward(ctypes.byref(m), ctypes.byref(sh), 0x1000, 0x1000, 0x1000, 0x1000, 1, 2, 0x1000, None, 0x1000, 1 << 30, None)
        assert rc == 3 and f"{bits}-bit routed experts" in lib.gptq_last_error().decode()


def test_no_kernel_was_added():
    from test_kernel_resources import _kernels
    ks = _kernels()
    assert len(ks) <= 1160, len(ks)
    assert len({n for n in ks if "moe_decode_kernel" in n}) == 8
    mine = {n: v for n, v in ks.items() if "moe_shared" in n}
    assert len(mine) == 1 and "moe_shared_kernel" in next(iter(mine)), sorted(mine)
    for n, v in mine.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0) and (v["vgpr"] or 0) <= 128, (n, v)


def test_python_signatures_carry_the_switch():
    from autogptq_amd.model_utils import autogptq_post_init
    from autogptq_amd.moe import QuantMoEExperts
    p = inspect.signature(QuantMoEExperts.post_init).parameters
    assert list(p) == ["self", "decode_copy", "batch", "backward", "low_bit", "prefill", "low_bit_decode"] and p["low_bit_decode"].default is False
    assert inspect.signature(autogptq_post_init).parameters["expert_low_bit_decode"].default is False
    ex = QuantMoEExperts(2, 256, 512, 3, 128)
    assert ex._switches["low_bit_decode"] is False and ex.low_bit_decode_max_tokens == 4
    assert "3-bit" in ex._declined("decode") and "3-bit" in ex._declined("batch") and "3-bit" in ex._declined("prefill")
    # with low_bit_decode=True the copy's pre-check is asked with low_bit=True; batch= and prefill= are asked as before
    assert ex._declined("decode", low_bit=True) == "" and "3-bit experts: the batch path" in ex._declined("batch") and "3-bit experts: the prefill path" in ex._declined("prefill")
    ex4 = QuantMoEExperts(2, 256, 512, 4, 128)
    assert ex4._declined("decode", low_bit=True) == "" and ex4._declined("batch") == ""
