"""CPU: GPTQ_MOE_LOW_BIT_PREFILL in gptq_moe_t.flags -- with the flag the prefill plan (any T on the decode copy; Python: 65 tokens and more) takes 2- and
3-bit experts with the plan keys and the workspace of the 4-bit set of the same shape; without it every entry point answers as before; the decode, shared
and batch entry points ignore the bit, the grouped and backward ones keep refusing it.  A numpy restatement of the address map of moe_panel_lowbit_kernel
(STRIP_CH / STEP_B / SLOT_B / COL_B per width) against the layout formula of prepack_decode_weights_kernel: every lane's bytes lie in its strip, the lanes
and steps tile each strip exactly once, and the words a lane fetches are the k = 64 kt + 32 half + 0..31 of its column.  Read off the built library: the
four new kernels exist next to the four 4- / 8-bit ones, inside 256 registers, scratch-free, lint-clean, fed by dwordx3 / dwordx2, inside the count cap."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402
from test_moe_prefill_host import SHAPES, _a256, _moe  # noqa: E402

LOW, DEC, BAT = 1, 8, 0x10
PRE = getattr(_lib, "MOE_LOW_BIT_PREFILL", 0x20)        # (a library without the flag: the tests below then fail on what it answers)


def _flagged(flags, *a, **kw):
    m = _moe(*a, **kw)
    m.flags = flags
    return m


def test_flag_values():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    assert "#define GPTQ_MOE_LOW_BIT_PREFILL 0x20" in header and "#define GPTQ_MOE_LOW_BIT_BATCH 0x10" in header
    assert _lib.MOE_LOW_BIT_PREFILL == 0x20 and _lib.MOE_LOW_BIT_BATCH == 0x10 and _lib.MOE_LOW_BIT_DECODE == 8 and _lib.MOE_LOW_BIT == 1
    assert _lib.load().gptq_abi_version() == 8 and _lib.ABI_VERSION == 8          # an additive flag: the ABI number stays


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [64, 128, 256, -1])
@pytest.mark.parametrize("flags", [PRE, PRE | BAT, PRE | DEC | LOW])
@pytest.mark.parametrize("bits", [2, 3])
def test_prefill_plan_and_workspace_with_the_flag(bits, flags, gs, act):
    """2, 3 and 4 bits share 128 k per chunk, NT = 4 and the 48-byte constant record: every key of the plan and the workspace are the 4-bit set's."""
    lib = _lib.load()
    for E, topk, H, I, dtype in SHAPES:
        m = _flagged(flags, E, H, I, bits=bits, gs=gs, dtype=dtype, act=act)
        m4 = _moe(E, H, I, bits=4, gs=gs, dtype=dtype, act=act)
        for T in (1, 64, 65, 300, 2048):
            d = _lib.describe_moe_prefill_plan(m, T, topk)
            assert d["path"] == "prefill" and d.pop("bits") == bits, d
            assert d == _lib.describe_moe_prefill_plan(m4, T, topk), d
            got = int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(m), T, topk))
            assert got > 0 and got == int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(m4), T, topk))
        assert lib.gptq_moe_prefill_forward(ctypes.byref(m), None, None, None, None, 0, topk, None, None, None, 0, None) == 0      # T = 0: nothing is read
    raw = ctypes.create_string_buffer(512)
    assert lib.gptq_describe_moe_prefill_plan(ctypes.byref(_flagged(flags, bits=bits, gs=gs, act=act)), 65, 2, raw, len(raw)) == 0
    assert raw.value.decode().startswith("path=prefill bm=64 launches=") and raw.value.decode().endswith(f" bits={bits}"), raw.value
    assert lib.gptq_describe_moe_prefill_plan(ctypes.byref(_flagged(flags, bits=4, gs=gs, act=act)), 65, 2, raw, len(raw)) == 0 and "bits=" not in raw.value.decode()


@pytest.mark.parametrize("bits", [2, 3])
def test_forward_gets_past_the_width_check_with_the_flag(bits):
    lib = _lib.load()
    m = _flagged(PRE, bits=bits)
    need = int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(m), 65, 2))
    assert need > 0
    assert lib.gptq_moe_prefill_forward(ctypes.byref(m), None, 0x1000, 0x1000, 0x1000, 65, 2, 0x1000, None, 0x1000, need, None) == 1      # GPTQ_ERR_NULL
    assert "must be non-NULL" in lib.gptq_last_error().decode()
    rc = lib.gptq_moe_prefill_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, 65, 2, 0x1000, None, 0x1000, need - 1, None)
    assert rc != 0 and "workspace too small" in lib.gptq_last_error().decode()


@pytest.mark.parametrize("flags", [0, LOW, DEC, BAT, BAT | DEC | LOW])
@pytest.mark.parametrize("T", [1, 65, 300])
@pytest.mark.parametrize("bits", [2, 3])
def test_without_the_flag_the_prefill_refusal_is_the_one_it_was(bits, T, flags):
    lib = _lib.load()
    m = _flagged(flags, bits=bits)
    want = f"{bits}-bit experts: the prefill path takes 4 or 8 bits"
    assert _lib.describe_moe_prefill_plan(m, T, 2) == {"path": "none", "reason": want.replace(" ", "_").replace("=", "_")}
    assert int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(m), T, 2)) == 0
    rc = lib.gptq_moe_prefill_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, T, 2, 0x1000, None, 0x1000, 1 << 30, None)
    assert rc == 3 and lib.gptq_last_error().decode() == want


@pytest.mark.parametrize("bits", [2, 3])
def test_the_other_rules_of_the_prefill_plan_stay(bits):
    for kw, T, topk, frag in ((dict(copy=False), 100, 2, "no_decode_copy"), (dict(dtype=_lib.GPTQ_F32), 100, 2, "fp32"), (dict(), 100, 9, "topk___9"),
                              (dict(gs=48), 100, 2, "group_size_48"), (dict(gs=32), 100, 2, "group_size_32"), (dict(E=257), 100, 2, "E___257"),
                              (dict(H=2048, I=1344), 100, 2, "multiples_of_128"), (dict(H=192, I=512), 100, 2, "multiples_of_128"),
                              (dict(), 40000, 2, "80000_rows")):
        d = _lib.describe_moe_prefill_plan(_flagged(PRE, bits=bits, **kw), T, topk)
        assert d["path"] == "none" and frag in d["reason"], (kw, d)
    d = _lib.describe_moe_prefill_plan(_flagged(PRE, bits=5), 100, 2)
    assert d["path"] == "none" and "got_5" in d["reason"], d
    m = _flagged(PRE, bits=bits)
    m._keep[0][0][3].qweight_tiled = 0x5008                     # (3 bits: a lane's 12 bytes are 4-byte aligned in an aligned copy; the copy itself keeps the rule)
    d = _lib.describe_moe_prefill_plan(m, 100, 2)
    assert d["path"] == "none" and "expert_3_gate" in d["reason"] and "aligned" in d["reason"], d


@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_the_other_paths_with_the_bit(bits):
    """decode, batch and the fused shared form ignore the bit (they answer as without it); the grouped and the backward entry points refuse 0x20 as an
    unknown bit with the message they have; 4- and 8-bit experts answer the prefill plan as without it."""
    from test_moe_shared_host import _shared
    lib = _lib.load()
    for base in (0, DEC, BAT, DEC | BAT):
        m, ref = _flagged(base | PRE, bits=bits), _flagged(base, bits=bits)
        for T in (1, 4):
            assert _lib.describe_moe_decode_plan(m, T, 2) == _lib.describe_moe_decode_plan(ref, T, 2)
            assert int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), T, 2)) == int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(ref), T, 2))
            sh = _shared(bits=4)
            assert _lib.describe_moe_shared_decode_plan(m, sh, T, 2) == _lib.describe_moe_shared_decode_plan(ref, sh, T, 2)
            assert (int(lib.gptq_moe_shared_decode_workspace_bytes(ctypes.byref(m), ctypes.byref(sh), T, 2))
                    == int(lib.gptq_moe_shared_decode_workspace_bytes(ctypes.byref(ref), ctypes.byref(sh), T, 2)))
        for T in (5, 64, 65):
            assert _lib.describe_moe_batch_plan(m, T, 2) == _lib.describe_moe_batch_plan(ref, T, 2)
            assert int(lib.gptq_moe_batch_workspace_bytes(ctypes.byref(m), T, 2)) == int(lib.gptq_moe_batch_workspace_bytes(ctypes.byref(ref), T, 2))
        if bits in (4, 8):
            for T in (1, 65, 300):
                assert _lib.describe_moe_prefill_plan(m, T, 2) == _lib.describe_moe_prefill_plan(ref, T, 2)
                assert int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(m), T, 2)) == int(lib.gptq_moe_prefill_workspace_bytes(ctypes.byref(ref), T, 2)) > 0
    for flags in (PRE, PRE | LOW, PRE | DEC, PRE | BAT):
        for d in (_lib.describe_moe_plan(_flagged(flags, bits=bits), 65, 2), _lib.describe_moe_backward_plan(_flagged(flags, bits=bits), 65, 2)):
            assert d["path"] == "per_expert" and d["reason"] == (f"moe->flags___0x{flags:x}:_unknown_flag_bits_(GPTQ_MOE_LOW_BIT_and_GPTQ_MOE_LOW_BIT_DECODE_are_"
                                                                 "the_only_ones)"), d
        assert int(lib.gptq_moe_workspace_bytes(ctypes.byref(_flagged(flags, bits=bits)), 65, 2)) == 0
    assert "unknown_flag" in _lib.describe_moe_plan(_flagged(0x40, bits=bits), 5, 2)["reason"]


@pytest.mark.parametrize("bits", [2, 3])
def test_the_decode_table_is_built_for_the_prefill_path_alone(bits):
    """With the prefill bit alone the table build passes the prefill path's check (and declines what that declines); the batch bit goes first, the decode
    bit in front of both; with neither the answer is the one it was."""
    lib = _lib.load()
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(PRE, bits=bits)), None, None) == 1 and "table is NULL" in lib.gptq_last_error().decode()
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(PRE, bits=bits, H=320, I=448)), None, None) == 3
    assert "multiples of 128" in lib.gptq_last_error().decode()
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(PRE, bits=bits, gs=32)), None, None) == 3      # the prefill path's group rule, not the batch path's
    assert "the prefill path takes 64 times a power of two" in lib.gptq_last_error().decode()
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(PRE | BAT, bits=bits, gs=32)), None, None) == 1       # batch first: it takes 32-wide groups
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(PRE | DEC, bits=bits, H=320, I=448)), None, None) == 1      # 0x20 | 8 behaves as 8
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(DEC, bits=bits, H=320, I=448)), None, None) == 1
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(0, bits=bits)), 0x1000, None) == 3
    assert lib.gptq_last_error().decode() == f"{bits}-bit experts: the decode path takes 4 or 8 bits"
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(PRE, bits=4, H=320, I=448)), None, None) == 1             # 4 bits: the bit changes nothing


# ---- the address map, restated ----------------------------------------------------------------------------------------------------------------------
WIDTHS = {4: dict(STRIP_CH=1024, STEP_B=512, SLOT_B=256, COL_B=16, WPL=4), 3: dict(STRIP_CH=768, STEP_B=384, SLOT_B=192, COL_B=12, WPL=3),
          2: dict(STRIP_CH=512, STEP_B=256, SLOT_B=128, COL_B=8, WPL=2)}


def _copy_word_owner(K, N, WPL):
    """prepack_decode_weights_kernel's store, restated: word ((s chunks + c) 64 WPL + (kb 16 + col) WPL + w) of the copy holds word w of the lane that owns
    k = 128 c + 32 kb + 0..31 of column 16 s + col.  Returns [words] -> (first k, column, w)."""
    chunks, strips = K // 128, N // 16
    s, c, kb, col, w = np.meshgrid(np.arange(strips), np.arange(chunks), np.arange(4), np.arange(16), np.arange(WPL), indexing="ij")
    idx = (s * chunks + c) * (64 * WPL) + (kb * 16 + col) * WPL + w
    owner = np.full((strips * chunks * 64 * WPL, 3), -1, dtype=np.int64)
    owner[idx.ravel()] = np.stack([(128 * c + 32 * kb).ravel(), (16 * s + col).ravel(), w.ravel()], axis=1)
    assert (owner >= 0).all()
    return owner


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_the_address_map_tiles_every_strip_once_and_fetches_the_lanes_own_k(bits):
    """moe_panel_body.inc: column block nb (32 columns = strips nb / 16, + 1), lane (l31, half), 64-deep step kt reads COL_B bytes at
    (nb / 16 + l31 / 16) chunks STRIP_CH + kt STEP_B + half SLOT_B + (l31 % 16) COL_B of the expert's copy."""
    c = WIDTHS[bits]
    assert c["STEP_B"] == 2 * c["SLOT_B"] and c["SLOT_B"] == 16 * c["COL_B"] and c["STRIP_CH"] == 2 * c["STEP_B"] and c["COL_B"] == 4 * c["WPL"]
    rng = np.random.default_rng(bits)
    for K in sorted({128, 256, *(128 * int(v) for v in rng.integers(1, 40, size=4))}):
        N = 64
        chunks, steps = K // 128, K // 64
        owner = _copy_word_owner(K, N, c["WPL"])
        strip_bytes = chunks * c["STRIP_CH"]
        hits = np.zeros(N // 16 * strip_bytes, dtype=np.int32)
        l31, half, kt = np.meshgrid(np.arange(32), np.arange(2), np.arange(steps), indexing="ij")
        for nb in range(0, N, 32):
            strip = nb // 16 + l31 // 16
            off = strip * strip_bytes + kt * c["STEP_B"] + half * c["SLOT_B"] + (l31 % 16) * c["COL_B"]
            assert (off >= strip * strip_bytes).all() and (off + c["COL_B"] <= (strip + 1) * strip_bytes).all()      # inside the lane's own strip
            assert (off % 4 == 0).all()
            for b in range(c["COL_B"]):
                np.add.at(hits, (off + b).ravel(), 1)
            for w in range(c["WPL"]):                                  # the words fetched: k = 64 kt + 32 half + 0..31 of column nb + l31, word w of that lane
                got = owner[(off // 4 + w).ravel()]
                want = np.stack([(64 * kt + 32 * half).ravel(), (nb + l31).ravel(), np.full(l31.size, w)], axis=1)
                assert np.array_equal(got, want), (K, nb, w)
        assert (hits == 1).all(), (K, int(hits.min()), int(hits.max()))          # the union over lanes and steps: every byte of every strip exactly once


# ---- the built library --------------------------------------------------------------------------------------------------------------------------------
def test_the_four_new_kernels_exist_inside_256_registers_and_the_count_stays_inside_its_cap():
    from test_kernel_resources import _kernels
    ks = _kernels()
    new = {n: v for n, v in ks.items() if "moe_panel_lowbit_kernel" in n}
    assert len(new) == 4, sorted(new)                               # <T, BITS>: fp16 / bf16 x 2 / 3 bits
    assert sorted(re.search(r"I(DF16_|DF16b)Li(\d)E", n).groups() for n in new) == [("DF16_", "2"), ("DF16_", "3"), ("DF16b", "2"), ("DF16b", "3")]
    old = {n: v for n, v in ks.items() if "moe_panel_kernel" in n}
    assert len(old) == 4 and not set(old) & set(new), sorted(old)   # the 4- / 8-bit forms keep their name and number
    for n, v in {**new, **old}.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0), (n, v)
        assert (v["vgpr"] or 0) + (v["agpr"] or 0) <= 256, (n, v)   # 8 waves per workgroup: two per SIMD
    # what paid: BITS of the fp32 matrix-core GEMM (4 -> 1) and the dtype of the K-split reduction (2 -> 1) became launch-uniform arguments
    assert sum(1 for n in ks if re.search(r"\d+gemm_f32_kernel", n)) == 1 and sum(1 for n in ks if re.search(r"\d+gemm_reduce_kernel", n)) == 1
    assert len(ks) <= 1160, len(ks)


def test_no_instruction_touches_an_in_flight_register_in_the_new_kernels():
    from test_kernel_resources import LLVM, MAGIC, SO
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not os.path.exists(SO) or not all(os.path.exists(t) for t in tools):
        pytest.skip("built library or ROCm LLVM tools not present")
    spec = importlib.util.spec_from_file_location("isa_inflight_lint", os.path.join(ROOT, "tools", "isa_inflight_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    seen = fed = 0
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([tools[0], f"--dump-section=.hip_fatbin={fat}", SO, os.path.join(d, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, a in enumerate(starts):
            chunk = blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"moe_panel_lowbit_kernel" not in chunk:
                continue
            part, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"co{i}.o")
            open(part, "wb").write(chunk)
            r = subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            asm = subprocess.run([tools[2], "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            seen += len(re.findall(r"moe_panel_lowbit_kernel\w*>?:", asm))
            for fam in ("moe_panel_lowbit_kernel", "moe_panel_kernel"):
                bad = lint.lint(asm, fam)
                assert not bad, bad[:5]
            # the ring element is one load's destination: the copy's words come by dwordx3 (3 bits) / dwordx2 (2 bits) and never by dwordx4 here
            for name, body in re.findall(r"<(_Z\w*moe_panel_lowbit_kernel\w*)>:\n(.*?)(?=\n[0-9a-f]+ <_Z|\Z)", asm, flags=re.S):
                want = "global_load_dwordx3" if "Li3E" in name else "global_load_dwordx2"
                assert want in body and "global_load_dwordx4 v" not in body.replace("global_load_lds_dwordx4", ""), name
                # the hand counts: a step's weight loads stay in flight with (12) or without (4) the 8 constant loads of a group's first step
                assert "s_waitcnt vmcnt(4)" in body and "s_waitcnt vmcnt(12)" in body, name
                fed += 1
    assert seen == 4 and fed == 4, (seen, fed)


def test_python_carries_the_switch():
    from autogptq_amd.model_utils import autogptq_post_init
    from autogptq_amd.moe import _PATHS, QuantMoEExperts
    import torch
    assert inspect.signature(autogptq_post_init).parameters["expert_low_bit_prefill"].default is False
    assert list(inspect.signature(QuantMoEExperts.post_init).parameters) == ["self", "decode_copy", "batch", "backward", "low_bit", "prefill", "low_bit_decode"]
    ex = QuantMoEExperts(2, 256, 512, 3, 128)
    assert ex.low_bit_prefill is False and "prefill" not in ex._live and ex.low_bit_prefill_min_tokens == 65
    assert "3-bit" in ex._declined("decode") and "3-bit experts: the prefill path" in ex._declined("prefill")
    assert (_PATHS["prefill"].multiple, _PATHS["prefill"].groups[:2]) == (128, (64, ()))
    # what post_init makes of the attribute for 2- / 3-bit experts: the copy's and the path's pre-check with low_bit=True
    assert ex._declined("decode", low_bit=True) == "" and "3-bit experts: the prefill path" in ex._declined("prefill")      # prefill=True alone stays without effect
    assert ex._declined("prefill", low_bit=True) == ""
    for args, kw, frag in (((2, 256, 192, 3, 64), {}, "multiples of 128"), ((2, 256, 512, 2, 32), {}, "group_size 32: the prefill path takes 64 times a power of two"),
                           ((2, 256, 512, 2, 96), {}, "group_size 96"), ((2, 256, 512, 3, 128), dict(weight_dtype=torch.float32), "fp32")):
        odd = QuantMoEExperts(*args, **kw)
        assert frag in odd._declined("prefill", low_bit=True), frag
    assert ex.plan(300)["path"] == "per_expert"                     # cpu tensors: nothing to plan
