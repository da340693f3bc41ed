"""CPU: the batch path of the mixture-of-experts layers in the C ABI (gptq_moe_batch_*: exports, plan, workspace formula, declines), that the grouped and the
decode entry points answer as before, and -- read off the built code objects -- that the new kernels are scratch-free, pass the in-flight lint, and that the
load-time kernels that paid for their instantiations are compiled once."""
import ctypes
import importlib.util
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

BATCH_SYMBOLS = ("gptq_moe_batch_workspace_bytes", "gptq_moe_batch_forward", "gptq_describe_moe_batch_plan")
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


def test_batch_symbols_exported_and_declared_abi_still_8():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in BATCH_SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and hasattr(lib, s), s
    assert lib.gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert "#define GPTQ_MI355X_ABI_VERSION 8" in header


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [32, 64, 128, -1])
@pytest.mark.parametrize("bits", [4, 8])
def test_plan_accepts_1_to_64_tokens(bits, gs, act):
    lib = _lib.load()
    for E, topk, H, I, dtype in SHAPES:
        m = _moe(E, H, I, bits=bits, gs=gs, dtype=dtype, act=act)
        for T in (1, 5, 16, 64):
            d = _lib.describe_moe_batch_plan(m, T, topk)
            R = T * topk
            assert d["path"] == "batch" and d["bm"] == 16 and d["s"] == 4, d
            assert d["tiles"] == R // 16 + min(E, R), d
            assert d["launches"] == (6 if act else 4), d              # act-order: the row gather through perm in front of either GEMM
            assert d["lds_pair"] <= 160 * 1024 and d["lds_down"] <= 160 * 1024 and 1 <= d["waves_pair"] <= 8 and 1 <= d["waves_down"] <= 8, d
            want = (_lib.WS_HEADER_BYTES + _a256(4 * (E + 1)) + 256 + _a256(16 * d["tiles"]) + 2 * _a256(4 * R) + _a256(R * I * 2) + _a256(4 * R * H)
                    + _a256(2 * R * H * 2) + _a256(R * I * 2))
            assert int(lib.gptq_moe_batch_workspace_bytes(ctypes.byref(m), T, topk)) == want, (T, want)
        d0 = _lib.describe_moe_batch_plan(m, 0, topk)
        assert d0["path"] == "batch" and d0["launches"] == 0, d0
        # T = 0: nothing is launched, nothing is dereferenced
        assert lib.gptq_moe_batch_forward(ctypes.byref(m), None, None, None, None, 0, topk, None, None, None, 0, None) == 0


@pytest.mark.parametrize("kw,T,topk,frag", [
    (dict(), 65, 2, "T = 65"),
    (dict(copy=False), 8, 2, "no decode copy"),
    (dict(bits=3), 8, 2, "3-bit"),
    (dict(bits=2), 8, 2, "2-bit"),
    (dict(dtype=_lib.GPTQ_F32), 8, 2, "fp32"),
    (dict(), 8, 9, "topk = 9"),
    (dict(gs=48), 8, 2, "group_size 48"),
    (dict(H=2048, I=1344), 8, 2, "multiples of 128"),
])
def test_plan_declines_with_a_reason(kw, T, topk, frag):
    lib = _lib.load()
    m = _moe(**kw)
    d = _lib.describe_moe_batch_plan(m, T, topk)
    assert d["path"] == "none" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
    assert int(lib.gptq_moe_batch_workspace_bytes(ctypes.byref(m), T, topk)) == 0
    rc = lib.gptq_moe_batch_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, T, topk, 0x1000, None, 0x1000, 1 << 30, None)
    assert rc == 3 and frag in lib.gptq_last_error().decode()          # GPTQ_ERR_UNSUPPORTED


def test_one_expert_without_a_copy_declines_by_name():
    m = _moe()
    m._keep[0][2][5].qweight_tiled = m._keep[0][2][5].qconst_tiled = None
    m._keep[0][2][5].tiled_cols = 0
    d = _lib.describe_moe_batch_plan(m, 8, 2)
    assert d["path"] == "none" and "expert_5_down" in d["reason"], d


# what the two existing describe entry points answered before the batch path existed (recorded from the parent revision)
GROUPED = {
    (8, 2, 256, 512, 1): "path=grouped bm=16 bn=64 tiles=2 ksplit=1 launches=4",
    (8, 2, 256, 512, 5): "path=grouped bm=16 bn=64 tiles=8 ksplit=1 launches=4",
    (8, 2, 256, 512, 64): "path=grouped bm=16 bn=64 tiles=16 ksplit=1 launches=4",
    (8, 2, 4096, 14336, 16): "path=grouped bm=16 bn=64 tiles=10 ksplit=1 launches=4",
    (8, 2, 4096, 14336, 64): "path=grouped bm=16 bn=64 tiles=16 ksplit=1 launches=4",
    (60, 4, 2048, 1408, 16): "path=grouped bm=16 bn=64 tiles=64 ksplit=1 launches=4",
}
DECODE = {
    (8, 2, 256, 512, 1): "path=decode launches=2 wg_pair=64 wg_down=16 waves_pair=2 waves_down=1 lds_pair=880 lds_down=1312",
    (8, 2, 4096, 14336, 4): "path=decode launches=2 wg_pair=7168 wg_down=1024 waves_pair=8 waves_down=16 lds_pair=11920 lds_down=35344",
    (8, 2, 256, 512, 5): "path=none reason=T___5_tokens:_the_decode_path_takes_1..4_(the_grouped_path_serves_more)",
}


def test_grouped_and_decode_answers_are_unchanged():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    for (E, topk, H, I, T), want in GROUPED.items():
        assert lib.gptq_describe_moe_plan(ctypes.byref(_moe(E, H, I)), T, topk, buf, len(buf)) == 0
        assert buf.value.decode() == want, (E, topk, H, I, T)
    for (E, topk, H, I, T), want in DECODE.items():
        assert lib.gptq_describe_moe_decode_plan(ctypes.byref(_moe(E, H, I)), T, topk, buf, len(buf)) == 0
        assert buf.value.decode() == want, (E, topk, H, I, T)
    m = _moe()
    assert int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), 5, 2)) == 0
    assert int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), 4, 2)) == _lib.WS_HEADER_BYTES + _a256(8 * 512 * 2) + _a256(32)


def test_batch_kernels_are_scratch_free_and_the_load_time_kernels_are_compiled_once():
    from test_kernel_resources import _kernels
    ks = _kernels()
    rows = {n: v for n, v in ks.items() if "moe_rows_kernel" in n}
    assert len(rows) == 4, sorted(rows)                              # <T, BITS>: fp16 / bf16 x 4 / 8 bits; pair / down, the group mode and the planes are run-time uniform
    for n, v in rows.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0), (n, v)
        assert (v["vgpr"] or 0) <= (256 if "Li8E" in n else 128), (n, v)      # 4 bits: two 8-wave workgroups per CU
    gather = {n: v for n, v in ks.items() if "moe_gather_rows_kernel" in n}
    assert len(gather) == 1 and not any((v["spill"] or 0) or (v["scratch"] or 0) for v in gather.values()), gather
    for fam in ("unpack_weights_kernel", "pack_zeros_kernel", "resequence_kernel", "prepack_decode_weights_kernel", "unprepack_decode_weights_kernel"):
        assert sum(1 for n in ks if re.search(r"\d" + fam, n)) == 1, fam          # (mangled: <length><name>)
    assert len({n for n in ks if "moe_decode_kernel" in n}) == 8
    assert len(ks) <= 1160, len(ks)


def test_no_instruction_touches_an_in_flight_register_in_the_batch_kernel():
    """moe_rows_kernel's weight / constant loads are inline asm behind hand-counted s_waitcnt: tools/isa_inflight_lint.py on its disassembly."""
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
            if b"moe_rows_kernel" not in chunk:
                continue
            part, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"co{i}.o")
            open(part, "wb").write(chunk)
            r = subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            asm = subprocess.run([tools[2], "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            seen += len(re.findall(r"moe_rows_kernel\w*>?:", asm))
            bad = lint.lint(asm, "moe_rows_kernel")
            assert not bad, bad[:5]
    assert seen == 4, seen
