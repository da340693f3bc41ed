"""CPU: gptq_grad_input (dX = dY . W^T on the packed weights) -- the built library exports it, its argument checks answer with the documented status
codes before anything reaches a device, and its kernels, read off the built code objects, stay within the instantiation budget with no scratch."""
import ctypes
import importlib.util
import os

import pytest

from autogptq_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(**kw):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000      # never dereferenced: validation fails first
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = 256, 256, 4, 128, 0, 0
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def test_library_exports_grad_input():
    lib = _lib.load()
    assert "gptq_grad_input" in _lib.EXPORTS
    assert hasattr(lib, "gptq_grad_input")
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    assert "int gptq_grad_input(const gptq_layer_t *layer, const void *dy, void *dx, int M, int accumulate, void *stream);" in header


@pytest.mark.parametrize("layer_kw,dy,dx,M,code,frag", [
    (dict(), None, 0x2000, 4, 1, "non-NULL"),
    (dict(), 0x2000, None, 4, 1, "non-NULL"),
    (dict(), 0x2000, 0x3000, 0, 2, "M must be > 0"),
    (dict(), 0x2000, 0x3000, -3, 2, "M must be > 0"),
    (dict(K=100), 0x2000, 0x3000, 4, 2, "multiples of 32"),
    (dict(N=48), 0x2000, 0x3000, 4, 2, "multiples of 32"),
    (dict(group_size=0), 0x2000, 0x3000, 4, 2, "group_size"),
    (dict(bits=5), 0x2000, 0x3000, 4, 3, "Only 2,3,4,8 bits"),
    (dict(dtype=7), 0x2000, 0x3000, 4, 3, "dtype"),
    (dict(qweight=None), 0x2000, 0x3000, 4, 1, "non-NULL"),
    (dict(), 0x2008, 0x3000, 4, 3, "16-byte aligned"),
    (dict(), 0x2000, 0x3002, 4, 3, "16-byte aligned"),
])
def test_grad_input_argument_checks(layer_kw, dy, dx, M, code, frag):
    lib = _lib.load()
    L = _layer(**layer_kw)
    rc = lib.gptq_grad_input(ctypes.byref(L), dy, dx, M, 0, None)
    assert rc == code, (rc, lib.gptq_last_error())
    assert frag in lib.gptq_last_error().decode()


def test_grad_input_null_layer():
    lib = _lib.load()
    assert lib.gptq_grad_input(None, 0x2000, 0x3000, 4, 1, None) == 1


def test_grad_input_kernels_in_the_built_code_objects():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr._kernels()                                  # skips where the LLVM tools or the library are missing
    gk = {n: v for n, v in ks.items() if "grad_input_kernel" in n}
    assert 1 <= len(gk) <= 7, sorted(gk)               # one per dtype: bits, group mode and tile height are runtime arguments
    for n, v in gk.items():
        assert (v["spill"] or 0) == 0 and (v["scratch"] or 0) == 0, (n, v)
        assert (v["vgpr"] or 0) + (v["agpr"] or 0) <= 256, (n, v)      # two 4-wave workgroups per CU
        assert (v["lds"] or 0) <= 65536, (n, v)
