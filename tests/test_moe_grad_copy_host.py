"""CPU: the routed experts' backward on the decode copy in the C ABI (gptq_moe_backward_ex / gptq_describe_moe_backward_plan_ex) -- the exports, the host
plan for a qualifying set and for each decline reason, flags = 0 against the entry points it extends, and the grouped mode's budget read off the built
code objects (a mode of grad_copy_kernel: no kernel is added)."""
import ctypes
import os
import re

from autogptq_amd import _lib
from test_moe_backward_host import _moe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = _lib.GRAD_ON_COPY


def _copy_moe(E=8, H=4096, I=14336, **kw):
    """_moe of test_moe_backward_host.py with a 16-column decode copy on every layer; keywords after the layer's own set fields of gate | up | down."""
    fields = {k: kw.pop(k) for k in list(kw) if k in ("gate", "up", "down", "all")}
    m = _moe(E, H, I, **kw)
    for name, ls in zip(("gate", "up", "down"), m._keep[0]):
        for l in ls:
            l.qweight_tiled, l.qconst_tiled, l.tiled_cols = 0x5000, 0x6000, _lib.STRIP_COLS
            for k, v in {**fields.get("all", {}), **fields.get(name, {})}.items():
                setattr(l, k, v)
    return m


def test_exports_and_declarations():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name, decl in (("gptq_moe_backward_ex", "int gptq_moe_backward_ex(const gptq_moe_t *moe, const void *table, const void *grad_table, const void *decode_table, "
                        "const void *x, const int64_t *topk_idx, const float *topk_w, const void *dout, int T, int topk, void *dx, float *dw, void *dgu_out, "
                        "void *workspace, size_t workspace_bytes, int flags, void *stream);"),
                       ("gptq_describe_moe_backward_plan_ex",
                        "int gptq_describe_moe_backward_plan_ex(const gptq_moe_t *moe, int T, int topk, int flags, char *out, size_t out_bytes);")):
        assert name in _lib.EXPORTS and hasattr(lib, name) and decl in flat, name
    assert lib.gptq_abi_version() == 8


def test_plan_strings():
    d = _lib.describe_moe_backward_plan_ex(_copy_moe(), 2048, 2, F)                  # Mixtral-8x7B: 4096 rows, 64 + 8 tiles
    assert d == dict(path="grouped_backward_copy", tiles=72, launches=5, up_launches=1, gm=0, act=0, gm_down=0, wg_recompute=72 * 224, wg_down=72 * 112,
                     wg_up=72 * 32), d
    d = _lib.describe_moe_backward_plan_ex(_copy_moe(E=60, H=2048, I=1408, gs=64, dtype=_lib.GPTQ_BF16, act=True), 17, 4, F)
    assert (d["path"], d["launches"], d["up_launches"], d["gm"], d["gm_down"], d["act"]) == ("grouped_backward_copy", 5, 1, 1, 1, 1), d      # one perm pointer
    d = _lib.describe_moe_backward_plan_ex(_copy_moe(gs=32, act=True, up=dict(perm=0x4400)), 17, 2, F)
    assert (d["launches"], d["up_launches"], d["gm"], d["act"]) == (6, 2, 2, 1), d
    assert _lib.describe_moe_backward_plan_ex(_copy_moe(), 0, 2, F)["launches"] == 0
    for kw, reason in ((dict(bits=8), "bits"), (dict(down=dict(bits=8)), "bits"), (dict(all=dict(qweight_tiled=None, qconst_tiled=None, tiled_cols=0)), "no_copy"),
                       (dict(up=dict(qweight_tiled=0x5008)), "no_copy"), (dict(gs=96), "group_size"), (dict(gs=384), "group_size")):
        m = _copy_moe(**kw)
        d = _lib.describe_moe_backward_plan_ex(m, 17, 2, F)
        rows = _lib.describe_moe_backward_plan(m, 17, 2)
        assert d.pop("copy_reason") == reason and d == rows and rows["path"] == "grouped_backward", (kw, d)
    # what gptq_moe_backward declines stays per expert, with its reason
    d = _lib.describe_moe_backward_plan_ex(_copy_moe(dtype=_lib.GPTQ_F32), 17, 2, F)
    assert d["path"] == "per_expert" and "fp32" in d["reason"], d
    # flags = 0: the line of the entry point it extends, byte for byte
    lib, a, b = _lib.load(), ctypes.create_string_buffer(512), ctypes.create_string_buffer(512)
    for m in (_copy_moe(), _copy_moe(bits=8, act=True), _copy_moe(bits=3), _copy_moe(E=60, H=2048, I=1408)):
        for T in (0, 17, 2048):
            assert lib.gptq_describe_moe_backward_plan(ctypes.byref(m), T, 2, a, len(a)) == lib.gptq_describe_moe_backward_plan_ex(ctypes.byref(m), T, 2, 0, b, len(b)) == 0
            assert a.value == b.value and b"copy" not in b.value, (a.value, b.value)


def test_unknown_flags_and_argument_checks():
    lib = _lib.load()
    m, buf = _copy_moe(H=256, I=512), ctypes.create_string_buffer(512)
    call = lambda flags, grad_table=0x7000, decode_table=0x7800, mm=m: lib.gptq_moe_backward_ex(
        ctypes.byref(mm), 0x6000, grad_table, decode_table, 0x1000, 0x8000, 0x9000, 0x2000, 9, 2, 0x3000, 0x4000, None, 0x5000, 4096, flags, None)
    for flags in (2, 6, -8):
        assert call(flags) == 3 and "flags" in lib.gptq_last_error().decode()
        assert lib.gptq_describe_moe_backward_plan_ex(ctypes.byref(m), 9, 2, flags, buf, len(buf)) == 3
    assert lib.gptq_describe_moe_backward_plan_ex(ctypes.byref(m), 9, 2, F, None, 0) == 1
    # every check answers before a launch: the copy form needs the decode table and no grad table, the rows form the reverse; then the workspace
    assert call(F, decode_table=None) == 1 and "decode_table" in lib.gptq_last_error().decode()
    assert call(F, grad_table=None) == 4 and "workspace too small" in lib.gptq_last_error().decode()
    assert call(0, grad_table=None) == 1 and "grad_table" in lib.gptq_last_error().decode()
    assert call(F, grad_table=None, mm=_copy_moe(H=256, I=512, bits=8)) == 1 and "grad_table" in lib.gptq_last_error().decode()
    assert call(0, decode_table=None) == 4


def test_kernel_budget_of_the_grouped_mode():
    from test_kernel_resources import _kernels
    ks = _kernels()                                     # skips where the LLVM tools or the library are missing
    gk = {n: v for n, v in ks.items() if "grad_copy_kernel" in n}
    assert len(gk) == 2 and all("Grouped" in n for n in gk), sorted(gk)            # <f16>, <bf16>, each with the grouped argument: the mode of one kernel
    for n, v in gk.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0) and (v["vgpr"] or 0) + (v["agpr"] or 0) <= 256 and (v["lds"] or 0) <= 65536, (n, v)
    assert len({n for n in ks if re.search(r"\d+moe_grad_kernel", n)}) == 2 and len(ks) <= 1160, len(ks)
