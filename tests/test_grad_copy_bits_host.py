"""CPU: GPTQ_GRAD_COPY_ANY_BITS (flags 5 = GPTQ_GRAD_ON_COPY | 4) -- 2-, 3- and 8-bit layers and routed experts on the decode-copy backward: the header, the
host plans per width and group mode, what flags 1 keeps answering, the flag's validity, the NULL-qweight check, and the Python values."""
import ctypes
import os

import pytest

from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear
from test_grad_copy_host import _layer
from test_moe_grad_copy_host import _copy_moe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = 5
plan = _lib.describe_grad_input_plan


def test_header_and_python_values():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    assert "#define GPTQ_GRAD_COPY_ANY_BITS 4" in header and "#define GPTQ_GRAD_ON_COPY 1" in header and _lib.load().gptq_abi_version() == 8
    assert [_lib.grad_copy_flags(v) for v in (False, None, True, "any_bits")] == [0, 0, 1, ANY] and QuantLinear.GRAD_ON_COPY is False
    with pytest.raises(ValueError):
        _lib.grad_copy_flags("all")


@pytest.mark.parametrize("bits", [2, 3, 8])
def test_dense_plan_lines(bits):
    for gs, gm in ((32, 2), (64, 1), (128, 0), (1024, 0), (4096, 0)):
        for dtype in (_lib.GPTQ_F16, _lib.GPTQ_BF16):
            assert plan(_layer(bits=bits, group_size=gs, dtype=dtype), 2048, ANY) == f"kernel=grad_copy bm=128 stages=64 gm={gm} act=0 bits={bits}"
        assert plan(_layer(bits=bits, group_size=gs), 2048, 1) == "kernel=grad_rows reason=bits"
    act = dict(qweight=None, g_idx=0x1000, perm=0x1000, qweight_seq=0x1000)
    assert plan(_layer(bits=bits, group_size=32, **act), 64, ANY) == f"kernel=grad_copy bm=64 stages=64 gm=2 act=1 bits={bits}"
    for kw, reason in ((dict(dtype=_lib.GPTQ_F32), "dtype"), (dict(qweight_tiled=None, qconst_tiled=None, tiled_cols=0), "no_copy"), (dict(group_size=96), "group_size"),
                       (dict(group_size=16), "group_size"), (dict(g_idx=0x1000), "no_copy")):
        assert plan(_layer(bits=bits, **kw), 64, ANY) == f"kernel=grad_rows reason={reason}", kw
    # the 4-bit line is the one flags 1 gives; a 2-bit copy qualifies with or without the forward's opt-in bits in tiled_cols
    assert plan(_layer(), 512, ANY) == plan(_layer(), 512, 1) == "kernel=grad_copy bm=64 stages=64 gm=0 act=0"
    for tc in (_lib.COPY_ROWS_INT2, _lib.COPY_ROWS_INT2 | _lib.COPY_ROWS_INT2_WIDE):
        assert plan(_layer(bits=2, tiled_cols=_lib.STRIP_COLS | tc), 64, ANY).endswith("act=0 bits=2")


def test_flag_validity_and_null_qweight():
    lib, buf = _lib.load(), ctypes.create_string_buffer(256)
    for flags in (4, 2, 6, 7, -8):
        assert lib.gptq_grad_input_ex(ctypes.byref(_layer()), 0x2000, 0x3000, 4, 0, flags, None) == 3 and "flags" in lib.gptq_last_error().decode()
        assert lib.gptq_describe_grad_input_plan(ctypes.byref(_layer()), 4, flags, buf, len(buf)) == 3
        assert lib.gptq_describe_moe_backward_plan_ex(ctypes.byref(_copy_moe(H=256, I=512)), 9, 2, flags, buf, len(buf)) == 3
    # 8 bits without rows: flags 5 passes the layer check (the next one answers: dy is NULL), flags 1 needs the rows
    L8 = _layer(qweight=None, bits=8)
    assert lib.gptq_grad_input_ex(ctypes.byref(L8), None, 0x3000, 4, 0, ANY, None) == 1 and "x/out" in lib.gptq_last_error().decode()
    assert lib.gptq_grad_input_ex(ctypes.byref(L8), 0x2000, 0x3000, 4, 0, 1, None) == 1 and "qweight" in lib.gptq_last_error().decode()


@pytest.mark.parametrize("bits", [2, 3, 8])
def test_moe_plan_lines(bits):
    def moe(**kw):
        m = _copy_moe(bits=bits, **kw)
        m.flags = _lib.MOE_LOW_BIT if bits < 4 else 0                   # what the rows backward needs to take 2- / 3-bit experts
        return m
    rows = _lib.describe_moe_backward_plan(moe(), 2048, 2)
    d = _lib.describe_moe_backward_plan_ex(moe(), 2048, 2, 1)
    assert rows["path"] == "grouped_backward" and d.pop("copy_reason") == "bits" and d == rows, d
    d = _lib.describe_moe_backward_plan_ex(moe(), 2048, 2, ANY)
    assert d == dict(path="grouped_backward_copy", tiles=72, launches=5, up_launches=1, gm=0, act=0, gm_down=0, wg_recompute=72 * 224, wg_down=72 * 112,
                     wg_up=72 * 32, bits=bits), d
    d = _lib.describe_moe_backward_plan_ex(moe(gs=32, act=True, up=dict(perm=0x4400)), 17, 2, ANY)
    assert (d["launches"], d["up_launches"], d["gm"], d["gm_down"], d["act"], d["bits"]) == (6, 2, 2, 2, 1, bits), d
    assert _lib.describe_moe_backward_plan_ex(moe(down=dict(bits=4)), 17, 2, ANY)["copy_reason"] == "bits"       # mixed widths: declined as a whole
    assert "bits" not in _lib.describe_moe_backward_plan_ex(_copy_moe(), 17, 2, ANY)                              # 4 bits: the line of flags 1
