"""CPU: the prefill path of the mixture-of-experts layers in the C ABI (gptq_moe_prefill_*: exports, plan, workspace, declines), its Python switches, and
-- read off the built code objects -- that moe_panel_kernel is compiled four times, scratch-free, inside 256 registers, and passes the in-flight lint."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402

PREFILL_SYMBOLS = ("gptq_moe_prefill_workspace_bytes", "gptq_moe_prefill_forward", "gptq_describe_moe_prefill_plan")
SHAPES = ((8, 2, 256, 512, _lib.GPTQ_F16), (60, 4, 2048, 1408, _lib.GPTQ_BF16), (8, 2, 4096, 14336, _lib.GPTQ_F16))


def _layer(K, N, bits=4, gs=128, dtype=_lib.GPTQ_F16, copy=True, act=False):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000          # never dereferenced by the host-only queries
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = K, N, bits, min(gs, K) if gs > 0 else K, dtype, 0
    if copy:
        L.qweight_tiled, L.qconst_tiled, L.tiled_cols = 0x5000, 0x6000, 16
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


def test_prefill_symbols_exported_and_declared_abi_still_8():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in PREFILL_SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert "#define GPTQ_MI355X_ABI_VERSION 8" in header


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [64, 128, 256, -1])
@pytest.mark.parametrize("bits", [4, 8])
def test_plan_accepts_any_token_count_and_the_workspace_is_its_regions(bits, gs, act):
    lib = _lib.load()
    for E, topk, H, I, dtype in SHAPES:
        m = _moe(E, H, I, bits=bits, gs=gs, dtype=dtype, act=act)
        last = 0
        for T in (1, 7, 64, 65, 100, 300, 2048):
            d = _lib.describe_moe_prefill_plan(m, T, topk)
            R = T * topk
            assert d["path"] == "prefill" and d["bm"] == 64, d
            assert d["tiles"] == R // 64 + min(E, R), d
            assert d["launches"] == (6 if act else 5), d                  # act-order down projections: the gather of H_sorted through perm
            nt = 2 if bits == 8 else 4
            assert d["nt_pair"] == nt // 2 and d["nt_down"] == nt and d["waves"] == 8 and d["waves_pair"] == (4 if act else 8), d
            assert d["spw_pair"] == -(-(H // 64) // d["waves_pair"]) and d["spw_down"] == -(-(I // 64) // 8) and d["lds"] <= 160 * 1024, d
            assert I % (32 * d["nt_pair"]) == 0 and H % (32 * d["nt_down"]) == 0
            regions = (_a256(4 * (E + 1)) + 256 + _a256(16 * d["tiles"]) + 2 * _a256(4 * R) + _a256((2 if act else 1) * R * H * 2) + _a256(R * I * 2)
                       + _a256(4 * R * H) + (_a256(R * I * 2) if act else 0))
            got = int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(m), T, topk))
            assert got >= _lib.WS_HEADER_BYTES + regions, (T, got)
            assert got >= last, (T, got, last)                            # monotone in T
            last = got
        d0 = _lib.describe_moe_prefill_plan(m, 0, topk)
        assert d0["path"] == "prefill" and d0["launches"] == 0, d0
        # T = 0: nothing is launched, nothing is dereferenced
        assert lib.gptq_moe_prefill_forward(ctypes.byref(m), None, None, None, None, 0, topk, None, None, None, 0, None) == 0


@pytest.mark.parametrize("kw,T,topk,frag", [
    (dict(copy=False), 100, 2, "no decode copy"),
    (dict(bits=3), 100, 2, "3-bit"),
    (dict(bits=2), 100, 2, "2-bit"),
    (dict(dtype=_lib.GPTQ_F32), 100, 2, "fp32"),
    (dict(), 100, 9, "topk = 9"),
    (dict(E=257), 100, 2, "E = 257"),
    (dict(gs=32), 100, 2, "group_size 32"),
    (dict(gs=96), 100, 2, "group_size 96"),
    (dict(H=2048, I=1344), 100, 2, "multiples of 128"),
    (dict(H=192, I=512), 100, 2, "multiples of 128"),
    (dict(), 40000, 2, "80000 rows"),
])
def test_plan_declines_with_a_reason(kw, T, topk, frag):
    lib = _lib.load()
    m = _moe(**kw)
    d = _lib.describe_moe_prefill_plan(m, T, topk)
    assert d["path"] == "none" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
    assert int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(m), T, topk)) == 0
    rc = lib.gptq_moe_prefill_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, T, topk, 0x1000, None, 0x1000, 1 << 30, None)
    assert rc == 3 and frag in lib.gptq_last_error().decode()          # GPTQ_ERR_UNSUPPORTED


def test_misaligned_pointers_and_a_short_workspace_are_refused():
    lib = _lib.load()
    m = _moe()
    need = int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(m), 100, 2))
    rc = lib.gptq_moe_prefill_forward(ctypes.byref(m), 0x1000, 0x1002, 0x1000, 0x1000, 100, 2, 0x1000, None, 0x1000, need, None)
    assert rc == 3 and "16-byte aligned" in lib.gptq_last_error().decode()
    rc = lib.gptq_moe_prefill_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, 100, 2, 0x1000, None, 0x1000, need - 1, None)
    assert rc != 0 and "workspace too small" in lib.gptq_last_error().decode()
    m._keep[0][0][3].qweight_tiled = 0x5008
    d = _lib.describe_moe_prefill_plan(m, 100, 2)
    assert d["path"] == "none" and "expert_3_gate" in d["reason"] and "aligned" in d["reason"], d


def test_one_expert_without_a_copy_declines_by_name():
    m = _moe()
    m._keep[0][2][5].qweight_tiled = m._keep[0][2][5].qconst_tiled = None
    m._keep[0][2][5].tiled_cols = 0
    d = _lib.describe_moe_prefill_plan(m, 100, 2)
    assert d["path"] == "none" and "expert_5_down" in d["reason"], d


def test_the_batch_answer_is_unchanged():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    assert lib.gptq_describe_moe_batch_plan(ctypes.byref(_moe()), 16, 2, buf, len(buf)) == 0
    assert buf.value.decode().startswith("path=batch bm=16 s=4 tiles=10 launches=4 ")
    assert lib.gptq_describe_moe_batch_plan(ctypes.byref(_moe()), 65, 2, buf, len(buf)) == 0
    assert buf.value.decode().startswith("path=none ")


def test_python_switches_accept_the_flag():
    from autogptq_amd.model_utils import autogptq_post_init
    from autogptq_amd.moe import QuantMoEExperts
    assert inspect.signature(QuantMoEExperts.post_init).parameters["prefill"].default is False
    assert inspect.signature(autogptq_post_init).parameters["expert_prefill"].default is False
    import torch
    q = QuantMoEExperts(4, 256, 512, 4, 128)
    assert q._switches["prefill"] is False and q._declined("prefill") == ""
    assert "group_size 32" in QuantMoEExperts(4, 256, 512, 4, 32)._declined("prefill")
    assert "multiples of 128" in QuantMoEExperts(4, 256, 192, 4, 64)._declined("prefill")
    assert "3-bit" in QuantMoEExperts(4, 256, 512, 3, 128)._declined("prefill")
    assert "fp32" in QuantMoEExperts(4, 256, 512, 4, 128, weight_dtype=torch.float32)._declined("prefill")
    assert q.plan(300)["path"] == "per_expert"                            # cpu tensors: nothing to plan
    with pytest.raises(RuntimeError):
        q.post_init(prefill=True)                                         # no CPU path


def test_panel_kernel_is_compiled_four_times_inside_256_registers_without_scratch():
    from test_kernel_resources import _kernels
    ks = _kernels()
    panel = {n: v for n, v in ks.items() if "moe_panel_kernel" in n}
    assert 1 <= len(panel) <= 4, sorted(panel)                        # <T, BITS>: fp16 / bf16 x 4 / 8 bits; pair / down, the group shift and the planes are run-time uniform
    for n, v in panel.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0), (n, v)
        assert (v["vgpr"] or 0) + (v["agpr"] or 0) <= 256, (n, v)     # 8 waves per workgroup: two per SIMD
        for fam in ("gemm_panel_kernel", "gemm_rows_kernel", "gemv_tiled_kernel"):
            assert fam not in n
    for fam in ("gemv_reduce_kernel", "silu_mul2_kernel", "permute_columns_kernel"):      # the utility kernels that paid for the four: one code object each
        assert sum(1 for n in ks if re.search(r"\d" + fam + "E", n)) == 1, fam
    assert len(ks) <= 1160, len(ks)


def test_no_instruction_touches_an_in_flight_register_in_the_panel_kernel():
    """moe_panel_kernel's weight / constant loads are inline asm behind hand-counted s_waitcnt: tools/isa_inflight_lint.py on its disassembly."""
    from test_kernel_resources import LLVM, MAGIC, SO
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not os.path.exists(SO) or not all(os.path.exists(t) for t in tools):
        pytest.skip("built library or ROCm LLVM tools not present")
    spec = importlib.util.spec_from_file_location("isa_inflight_lint", os.path.join(ROOT, "tools", "isa_inflight_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    seen = 0
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([tools[0], f"--dump-section=.hip_fatbin={fat}", SO, os.path.join(d, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, a in enumerate(starts):
            chunk = blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"moe_panel_kernel" not in chunk:
                continue
            part, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"co{i}.o")
            open(part, "wb").write(chunk)
            r = subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            asm = subprocess.run([tools[2], "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            seen += len(re.findall(r"moe_panel_kernel\w*>?:", asm))
            bad = lint.lint(asm, "moe_panel_kernel")
            assert not bad, bad[:5]
    assert seen == 4, seen
