"""CPU: GPTQ_MOE_LOW_BIT_BATCH in gptq_moe_t.flags -- with the flag the batch plan (5..64 tokens on the decode copy) takes 2- and 3-bit experts with the
plan keys and the workspace of the 4-bit set of the same shape; without it every entry point answers as before; the grouped and backward entry points
keep refusing the bit (the Python layer keeps a struct of its own for the batch path).  A numpy restatement of how moe_rows_lowbit_kernel reads the 2- and
3-bit decode copy (rowsk::Deq1_2 on a shifted word, rowsk::Deq1_3::frag cases 0..3) on words made by the oracle's restatement of the copy: every k of a
lane's 32 lands where the A operand of the MFMA step has it, and every fp16 intermediate is exact.  Read off the built library: the four new kernels
exist, are scratch- and spill-free inside 128 registers, pass the in-flight lint, and the kernel count stays inside its cap."""
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
from oracle.gptq_oracle import _decode_copy_lane_words  # noqa: E402
from test_moe_decode_host import _a256, _moe  # noqa: E402

LOW, DEC = 1, 8
BAT = getattr(_lib, "MOE_LOW_BIT_BATCH", 0x10)          # (the parent has no such name: the tests below then fail on what the library answers)

SHAPES = [(8, 2, 256, 512, _lib.GPTQ_F16), (4, 2, 640, 384, _lib.GPTQ_BF16), (60, 4, 2048, 1408, _lib.GPTQ_BF16), (8, 2, 4096, 14336, _lib.GPTQ_F16)]


def _flagged(flags, *a, **kw):
    m = _moe(*a, **kw)
    m.flags = flags
    return m


def test_flag_values():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    assert "#define GPTQ_MOE_LOW_BIT_BATCH 0x10" in header and "#define GPTQ_MOE_LOW_BIT_DECODE 8" in header and "#define GPTQ_MOE_LOW_BIT 1" in header
    assert _lib.MOE_LOW_BIT_BATCH == 0x10 and _lib.MOE_LOW_BIT_DECODE == 8 and _lib.MOE_LOW_BIT == 1
    assert _lib.load().gptq_abi_version() == 8 and _lib.ABI_VERSION == 8          # an additive flag: the ABI number stays


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("gs", [32, 64, 128, -1])
@pytest.mark.parametrize("flags", [BAT, BAT | DEC, BAT | DEC | LOW])
@pytest.mark.parametrize("bits", [2, 3])
def test_batch_plan_and_workspace_with_the_flag(bits, flags, gs, act):
    """2, 3 and 4 bits share 128 k per chunk and the 48-byte constant record: every key of the plan and the workspace are the 4-bit set's; the width is named."""
    lib = _lib.load()
    for E, topk, H, I, dtype in SHAPES:
        m = _flagged(flags, E, H, I, bits=bits, gs=gs, dtype=dtype, act=act)
        m4 = _moe(E, H, I, bits=4, gs=gs, dtype=dtype, act=act)
        for T in (5, 16, 64):
            d = _lib.describe_moe_batch_plan(m, T, topk)
            assert d["path"] == "batch" and d.pop("bits") == bits, d
            assert d == _lib.describe_moe_batch_plan(m4, T, topk), d
            got = int(lib.gptq_moe_batch_workspace_bytes(ctypes.byref(m), T, topk))
            assert got > 0 and got == int(lib.gptq_moe_batch_workspace_bytes(ctypes.byref(m4), T, topk))
            R = T * topk
            assert got == (_lib.WS_HEADER_BYTES + _a256(4 * (E + 1)) + 256 + _a256(16 * d["tiles"]) + 2 * _a256(4 * R) + _a256(R * I * 2) + _a256(4 * R * H)
                           + _a256(2 * R * H * 2) + _a256(R * I * 2))
        d65 = _lib.describe_moe_batch_plan(m, 65, topk)
        assert d65["path"] == "none" and "T___65" in d65["reason"], d65
        assert int(lib.gptq_moe_batch_workspace_bytes(ctypes.byref(m), 65, topk)) == 0
        assert lib.gptq_moe_batch_forward(ctypes.byref(m), None, None, None, None, 0, topk, None, None, None, 0, None) == 0      # T = 0: nothing is read
    raw = ctypes.create_string_buffer(512)
    assert lib.gptq_describe_moe_batch_plan(ctypes.byref(_flagged(flags, bits=bits, gs=gs, act=act)), 5, 2, raw, len(raw)) == 0
    assert raw.value.decode().startswith("path=batch bm=16 s=4 tiles=8 launches=") and raw.value.decode().endswith(f" bits={bits}")
    assert lib.gptq_describe_moe_batch_plan(ctypes.byref(_moe(gs=gs, act=act)), 5, 2, raw, len(raw)) == 0 and "bits=" not in raw.value.decode()


@pytest.mark.parametrize("flags", [0, LOW, DEC, DEC | LOW])
@pytest.mark.parametrize("T", [5, 64, 65])
@pytest.mark.parametrize("bits", [2, 3])
def test_without_the_flag_the_batch_refusal_is_the_one_it_was(bits, T, flags):
    lib = _lib.load()
    m = _flagged(flags, bits=bits)
    want = f"T = {T} tokens: the batch path takes 1..64 (the grouped path serves more)" if T > 64 else f"{bits}-bit experts: the batch path takes 4 or 8 bits"
    assert _lib.describe_moe_batch_plan(m, T, 2) == {"path": "none", "reason": want.replace(" ", "_").replace("=", "_")}
    assert int(lib.gptq_moe_batch_workspace_bytes(ctypes.byref(m), T, 2)) == 0
    rc = lib.gptq_moe_batch_forward(ctypes.byref(m), 0x1000, 0x1000, 0x1000, 0x1000, T, 2, 0x1000, None, 0x1000, 1 << 30, None)
    assert rc == 3 and lib.gptq_last_error().decode() == want
    if not flags & DEC:
        assert lib.gptq_moe_build_decode_table(ctypes.byref(m), 0x1000, None) == 3
        assert lib.gptq_last_error().decode() == f"{bits}-bit experts: the decode path takes 4 or 8 bits"


@pytest.mark.parametrize("bits", [2, 3])
def test_the_other_rules_of_the_batch_plan_stay(bits):
    for kw, T, topk, frag in ((dict(copy=False), 8, 2, "no_decode_copy"), (dict(dtype=_lib.GPTQ_F32), 8, 2, "fp32"), (dict(), 8, 9, "topk___9"),
                              (dict(gs=48), 8, 2, "group_size_48"), (dict(E=257), 8, 2, "E___257"), (dict(H=2048, I=1344), 8, 2, "multiples_of_128"),
                              (dict(), 65, 2, "T___65")):
        d = _lib.describe_moe_batch_plan(_flagged(BAT, bits=bits, **kw), T, topk)
        assert d["path"] == "none" and frag in d["reason"], (kw, d)
    d = _lib.describe_moe_batch_plan(_flagged(BAT, bits=5), 8, 2)
    assert d["path"] == "none" and "got_5" in d["reason"], d


@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_the_other_paths_with_the_bit(bits):
    """decode, prefill and the fused shared form ignore the bit (they answer as without it); the grouped and the backward entry points keep refusing 0x10
    with the message they had for it; 4- and 8-bit experts answer the batch plan as without it."""
    from test_moe_shared_host import _shared
    lib = _lib.load()
    for base in (0, DEC):
        m, ref = _flagged(base | BAT, bits=bits), _flagged(base, bits=bits)
        for T in (1, 4):
            assert _lib.describe_moe_decode_plan(m, T, 2) == _lib.describe_moe_decode_plan(ref, T, 2)
            assert int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(m), T, 2)) == int(lib.gptq_moe_decode_workspace_bytes(ctypes.byref(ref), T, 2))
            sh = _shared(bits=4)
            assert _lib.describe_moe_shared_decode_plan(m, sh, T, 2) == _lib.describe_moe_shared_decode_plan(ref, sh, T, 2)
        assert _lib.describe_moe_prefill_plan(m, 65, 2) == _lib.describe_moe_prefill_plan(ref, 65, 2)
        if bits in (4, 8):
            assert _lib.describe_moe_batch_plan(m, 16, 2) == _lib.describe_moe_batch_plan(ref, 16, 2)
    for flags in (BAT, BAT | LOW, BAT | DEC):
        for d in (_lib.describe_moe_plan(_flagged(flags, bits=bits), 5, 2), _lib.describe_moe_backward_plan(_flagged(flags, bits=bits), 5, 2)):
            assert d["path"] == "per_expert" and d["reason"] == (f"moe->flags___0x{flags:x}:_unknown_flag_bits_(GPTQ_MOE_LOW_BIT_and_GPTQ_MOE_LOW_BIT_DECODE_are_"
                                                                 "the_only_ones)"), d
    assert "unknown_flag" in _lib.describe_moe_plan(_flagged(0x40, bits=bits), 5, 2)["reason"]


@pytest.mark.parametrize("bits", [2, 3])
def test_the_decode_table_is_built_for_the_batch_path_alone(bits):
    """With the batch bit alone the table build passes the batch path's check (and declines what that declines); T = 0 reaches the NULL-table check."""
    lib = _lib.load()
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(BAT, bits=bits)), None, None) == 1 and "table is NULL" in lib.gptq_last_error().decode()
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(BAT, bits=bits, H=320, I=448)), None, None) == 3
    assert "multiples of 128" in lib.gptq_last_error().decode()
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(BAT | DEC, bits=bits, H=320, I=448)), None, None) == 1      # both bits: the decode path's check, as before
    assert lib.gptq_moe_build_decode_table(ctypes.byref(_flagged(BAT, bits=4, H=320, I=448)), None, None) == 1             # 4 bits: the bit changes nothing


# ---- the readers, restated ----------------------------------------------------------------------------------------------------------------------------
def _h(bits16):
    """fp16 values of uint16 bit patterns, as float64 (exact)."""
    return np.asarray(bits16, dtype=np.uint16).view(np.float16).astype(np.float64)


class _Exact:
    """fp16 arithmetic that asserts every result is representable: a + b and a * b are computed in float64 and must survive the rounding to fp16."""

    def __init__(self):
        self.ops = 0

    def _chk(self, v):
        r = v.astype(np.float16).astype(np.float64)
        assert np.array_equal(r, v), "an fp16 intermediate is not exact"
        self.ops += v.size
        return v

    def add(self, a, b):
        return self._chk(a + b)

    def mul(self, a, b):
        return self._chk(a * b)


def _halves(word):
    """The two 16-bit halves of uint32 words as a trailing axis (low = the even k of a pair)."""
    return np.stack([word & np.uint32(0xffff), word >> np.uint32(16)], axis=-1)


def _field(ex, word, mask16, rr, cbits):
    """rowsk::Deq1_x::p<i>: OR the exponent of 1024 over the masked field of both halves, times rr, plus the constant whose fp16 bits are cbits."""
    v = _h((_halves(word) & np.uint32(mask16)) | np.uint32(0x6400))
    if rr != 1.0:
        v = ex.mul(v, rr)
    return ex.add(v, float(_h(cbits)))


def _frag2(ex, words, ks, z):
    """Deq1_2::frag(words[ks >> 1] >> 8 (ks & 1)) before the scale: [..., 8] = the lane's k 8 ks .. 8 ks + 7 minus z."""
    q = words[..., ks >> 1] >> np.uint32(8 * (ks & 1))
    c = [(z * 1 + 0xE400) & 0xffff, (z * 4 + 0xDC00) & 0xffff, (z * 16 + 0xD400) & 0xffff, (z * 64 + 0xCC00) & 0xffff]
    ps = [_field(ex, q, 0x0003, 1.0, c[0]), _field(ex, q, 0x000c, 0.25, c[1]), _field(ex, q, 0x0030, 0.0625, c[2]), _field(ex, q, 0x00c0, 0.015625, c[3])]
    return np.concatenate(ps, axis=-1)


def _frag3(ex, w, ks, z):
    """Deq1_3::frag(words, ks) before the scale."""
    c0, c1, c2 = (z + 0xE400) & 0xffff, (z * 8 + 0xD800) & 0xffff, (z * 64 + 0xCC00) & 0xffff

    def p0(q): return _field(ex, q, 0x0007, 1.0, c0)
    def p1(q): return _field(ex, q, 0x0038, 0.125, c1)
    def p2(q): return _field(ex, q, 0x01c0, 0.015625, c2)
    w0, w1, w2 = w[..., 0], w[..., 1], w[..., 2]
    s6 = np.uint32(6)
    if ks == 0:
        h = [p0(w0), p1(w0), p2(w0), p1(w0 >> s6)]
    elif ks == 1:
        h = [p2(w0 >> s6), p0(w1), p1(w1), p2(w1)]
    elif ks == 2:
        h = [p1(w1 >> s6), p2(w1 >> s6), p0(w2), p1(w2)]
    else:
        t = (w0 >> np.uint32(15)) & np.uint32(0x00010001)
        t = ((w1 >> np.uint32(14)) & np.uint32(0x00020002)) | t
        t = ((w2 >> np.uint32(13)) & np.uint32(0x00040004)) | t
        h = [p2(w2), p1(w2 >> s6), p2(w2 >> s6), p0(t)]
    return np.concatenate(h, axis=-1)


@pytest.mark.parametrize("bits", [2, 3])
def test_readers_put_every_k_where_the_a_operand_has_it_and_stay_exact(bits):
    """MFMA step ks of lane (column r, k-slot g) multiplies the 16-byte piece 4 g + ks of the staged row -- x[32 g + 8 ks + 0..7] in memory order -- with the
    B fragment the reader makes of the lane's words: element j of it must be (value of k 8 ks + j) - z.  Both zero conventions: z = (f + 1) & maxq (wrap:
    0..maxq) and z = f + 1 (nowrap: 1..maxq + 1); every field value at every position (a de Bruijn-free brute force: random lanes plus the constant ones)."""
    maxq = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    v = rng.integers(0, maxq + 1, size=(256, 32), dtype=np.uint32)
    v = np.concatenate([v, np.full((1, 32), maxq, dtype=np.uint32), np.zeros((1, 32), dtype=np.uint32), (np.arange(32, dtype=np.uint32) % (maxq + 1))[None]])
    for f in range(maxq + 1):                                    # one-hot lanes: value f at one k, the complement everywhere else
        one = np.full((32, 32), maxq - f, dtype=np.uint32)
        one[np.arange(32), np.arange(32)] = f
        v = np.concatenate([v, one])
    words = _decode_copy_lane_words(v, bits)
    assert words.shape[-1] == (2 if bits == 2 else 3)
    ex = _Exact()
    for mode, zs in (("wrap", range(0, maxq + 1)), ("nowrap", range(1, maxq + 2))):
        for z in zs:
            for ks in range(4):
                got = (_frag2 if bits == 2 else _frag3)(ex, words, ks, z)
                want = v[:, 8 * ks:8 * ks + 8].astype(np.float64) - z
                assert np.array_equal(got, want), (mode, z, ks)
    assert ex.ops > 0


# ---- the built library --------------------------------------------------------------------------------------------------------------------------------
def test_the_four_new_kernels_exist_scratch_free_and_the_count_stays_inside_its_cap():
    from test_kernel_resources import _kernels
    ks = _kernels()
    new = {n: v for n, v in ks.items() if "moe_rows_lowbit_kernel" in n}
    assert len(new) == 4, sorted(new)                               # <T, BITS>: fp16 / bf16 x 2 / 3 bits
    assert sorted(re.search(r"I(DF16_|DF16b)Li(\d)E", n).groups() for n in new) == [("DF16_", "2"), ("DF16_", "3"), ("DF16b", "2"), ("DF16b", "3")]
    for n, v in new.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0), (n, v)
        assert (v["vgpr"] or 0) <= 128, (n, v)                      # the 4-bit form's budget: two 8-wave workgroups per CU
    assert len({n for n in ks if "moe_rows_kernel" in n}) == 4      # the 4- / 8-bit forms keep their name and number
    # what paid: SLOT of the act-order row permutes became a launch-uniform argument (6 + 2 instantiations -> 3 + 1)
    assert sum(1 for n in ks if re.search(r"\d+permute_rows_kernel", n)) == 3 and sum(1 for n in ks if re.search(r"\d+permute_rows4_kernel", n)) == 1
    assert len(ks) <= 1160, len(ks)


def test_no_instruction_touches_an_in_flight_register_in_the_new_kernels():
    from test_kernel_resources import LLVM, MAGIC, SO
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not os.path.exists(SO) or not all(os.path.exists(t) for t in tools):
        pytest.skip("built library or ROCm LLVM tools not present")
    spec = importlib.util.spec_from_file_location("isa_inflight_lint", os.path.join(ROOT, "tools", "isa_inflight_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    seen = wide = 0
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([tools[0], f"--dump-section=.hip_fatbin={fat}", SO, os.path.join(d, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, a in enumerate(starts):
            chunk = blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"moe_rows_lowbit_kernel" not in chunk:
                continue
            part, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"co{i}.o")
            open(part, "wb").write(chunk)
            r = subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            asm = subprocess.run([tools[2], "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            seen += len(re.findall(r"moe_rows_lowbit_kernel\w*>?:", asm))
            bad = lint.lint(asm, "moe_rows_lowbit_kernel")
            assert not bad, bad[:5]
            # the ring element is one load's destination: the copy's words come by dwordx3 (3 bits) / dwordx2 (2 bits) and never by dwordx4 here
            for name, body in re.findall(r"<(_Z\w*moe_rows_lowbit_kernel\w*)>:\n(.*?)(?=\n[0-9a-f]+ <_Z|\Z)", asm, flags=re.S):
                want = "global_load_dwordx3" if "Li3E" in name else "global_load_dwordx2"
                assert want in body and "global_load_dwordx4 v" not in body.replace("global_load_lds_dwordx4", ""), name
                wide += 1
    assert seen == 4 and wide == 4, (seen, wide)


def test_python_carries_the_switch():
    from autogptq_amd.model_utils import autogptq_post_init
    from autogptq_amd.moe import _PATHS, QuantMoEExperts
    assert inspect.signature(autogptq_post_init).parameters["expert_low_bit_batch"].default is False
    ex = QuantMoEExperts(2, 256, 512, 3, 128)
    assert ex.low_bit_batch is False and "batch" not in ex._live and ex.low_bit_batch_max_tokens == 64
    assert "3-bit" in ex._declined("decode") and "3-bit experts: the batch path" in ex._declined("batch")
    assert (_PATHS["batch"].multiple, _PATHS["batch"].groups[:2]) == (128, (128, (32, 64)))
    # what post_init makes of the attribute for 2- / 3-bit experts: the copy's and the path's pre-check with low_bit=True
    assert ex._declined("decode", low_bit=True) == "" and "3-bit experts: the batch path" in ex._declined("batch")      # batch=True alone stays without effect
    assert ex._declined("batch", low_bit=True) == ""
    odd = QuantMoEExperts(2, 256, 192, 3, 64)
    assert "multiples of 128" in odd._declined("batch", low_bit=True)
