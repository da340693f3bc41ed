"""CPU: the backward on the decode copy (gptq_grad_input_ex / gptq_describe_grad_input_plan) -- the exports, the host plan for a qualifying and for each
declined layer, and grad_copy_kernel's budget read off the built code objects."""
import ctypes
import os

from autogptq_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(**kw):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = L.qweight_tiled = L.qconst_tiled = 0x1000      # compared with NULL, never dereferenced
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode, L.tiled_cols = 4096, 4096, 4, 128, _lib.GPTQ_F16, 0, _lib.STRIP_COLS
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def test_exports_host_plan_and_kernel_budget():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    for name, decl in (("gptq_grad_input_ex", "int gptq_grad_input_ex(const gptq_layer_t *layer, const void *dy, void *dx, int M, int accumulate, int flags, void *stream);"),
                       ("gptq_describe_grad_input_plan", "int gptq_describe_grad_input_plan(const gptq_layer_t *layer, int M, int flags, char *out, size_t out_bytes);")):
        assert name in _lib.EXPORTS and hasattr(lib, name) and decl in header, name
    assert lib.gptq_abi_version() == 8 and "#define GPTQ_GRAD_ON_COPY 1" in header
    F = _lib.GRAD_ON_COPY
    plan = _lib.describe_grad_input_plan
    assert plan(_layer(), 2048, F) == "kernel=grad_copy bm=128 stages=64 gm=0 act=0"             # 16 x 32 = 512 tiles of 128 rows
    assert plan(_layer(), 512, F) == "kernel=grad_copy bm=64 stages=64 gm=0 act=0"               # 4 x 32 = 128 tiles of 128 rows: 64-row tiles instead
    assert plan(_layer(qweight=None, group_size=32, g_idx=0x1000, perm=0x1000, qweight_seq=0x1000), 64, F) == "kernel=grad_copy bm=64 stages=64 gm=2 act=1"
    assert plan(_layer(group_size=64, dtype=_lib.GPTQ_BF16), 1, F) == "kernel=grad_copy bm=64 stages=64 gm=1 act=0"
    for kw, flags, reason in ((dict(), 0, "flag_off"), (dict(bits=8), F, "bits"), (dict(bits=2), F, "bits"), (dict(bits=3), F, "bits"), (dict(dtype=_lib.GPTQ_F32), F, "dtype"),
                              (dict(qweight_tiled=None, qconst_tiled=None, tiled_cols=0), F, "no_copy"), (dict(group_size=96), F, "group_size"),
                              (dict(group_size=384), F, "group_size")):
        assert plan(_layer(**kw), 64, flags) == f"kernel=grad_rows reason={reason}", kw
    # a declined layer needs its rows; a qualifying one passes the layer check without them (nothing launches: dy is NULL)
    assert lib.gptq_grad_input_ex(ctypes.byref(_layer(qweight=None, bits=8)), 0x2000, 0x3000, 4, 0, F, None) == 1
    assert lib.gptq_grad_input_ex(ctypes.byref(_layer(qweight=None)), None, 0x3000, 4, 0, F, None) == 1 and "x/out" in lib.gptq_last_error().decode()
    assert lib.gptq_grad_input_ex(ctypes.byref(_layer()), 0x2000, 0x3000, 0, 0, F, None) == 2
    assert lib.gptq_grad_input_ex(ctypes.byref(_layer()), 0x2000, 0x3000, 4, 0, 6, None) == 3
    from test_kernel_resources import _kernels
    ks = _kernels()                                     # skips where the LLVM tools or the library are missing
    gk = {n: v for n, v in ks.items() if "grad_copy_kernel" in n}
    assert 1 <= len(gk) <= 2 and not any("grad_input_kernel" in n for n in gk), sorted(gk)
    for n, v in gk.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0) and (v["vgpr"] or 0) + (v["agpr"] or 0) <= 256 and (v["lds"] or 0) <= 65536, (n, v)
    assert len(ks) <= 1160, len(ks)
