"""CPU: the head of the decode-copy kernel, read from the BUILT library (no GPU).  The three instantiations of the Llama-7B decode step -- q|k|v
(<4, 1, 4, f16, 8, 0, 0>), o / down (<4, 1, 2, f16, 16, 0, 0>) and the two-strip gate|up launch (<4, 1, 4, f16, 8, 6, 0>) -- are disassembled as
test_tiled_tail_isa.py does (its own copy of the extraction), and the HEAD is taken to be the instructions, in static order, in front of the first
global_load_dwordx4 that is not an LDS DMA: the first weight load.

What is asserted, and what the parent commit had:
  (a) every s_load_* of the head precedes its first s_waitcnt that names lgkmcnt: ONE scalar-load round trip in front of the first weight load
      -- parent: five s_load, a wait, then s_load_dwordx8 / s_load_dwordx2 of the layer record (instructions 64 / 65 of o / down, 65 / 66 of the others) and a
         second wait; now two s_load_dwordx16 and one wait;
  (b) no v_readfirstlane_b32 of the head is fed by a v_cndmask_b32 (directly or through vector arithmetic): the layer is selected on the scalar unit
      -- parent: the three compares of the selector went through v_cndmask_b32 + v_readfirstlane_b32 (2 / 2 / 3 v_cndmask_b32 in the head); now none;
  (c) the head is short.  Static instruction counts, q|k|v / o, down / gate|up:
         parent  186 / 180 / 198
         now     139 / 134 / 144      bound = now + 10 %: 152 / 147 / 158
      Two thirds of the parent (124 / 120 / 132) is NOT reached in static count.  What remains: the entry batch and the cold-branch defaults (~17), the selector
      (19 static; a first-layer workgroup leaves it after 5), two straight-line rounds each for x and for the constants (13 + 14 static instructions per
      block, a wave with no piece skips a block on one compare) and the weight address (~24).  The rounds are static instructions few waves execute: at
      K = 4096 a wave of the 16-wave launches runs 60 (no piece), 76 (an x piece) or 93 (x and constants) instructions in front of its first weight load,
      where the parent ran about 135 and waited for two scalar-load round trips.
Only the opcodes named here are looked at.  Skipped where the LLVM tools or the library are missing (the product needs neither)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.environ.get("GPTQ_MI355X_LIB", os.path.join(ROOT, "autogptq_amd", "libgptq_mi355x.so"))
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
HEADLINE = {"qkv": "<4, 1, 4, _Float16, 8, 0, 0>", "o_down": "<4, 1, 2, _Float16, 16, 0, 0>", "gate_up": "<4, 1, 4, _Float16, 8, 6, 0>"}
BOUND = {"qkv": 152, "o_down": 147, "gate_up": 158}


def _bodies():
    """{template arguments: [instruction, ...]} of the three kernels."""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not os.path.exists(SO) or not all(os.path.exists(t) for t in tools):
        pytest.skip("built library or ROCm LLVM tools not present")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([tools[0], f"--dump-section=.hip_fatbin={fat}", SO, os.path.join(d, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, a in enumerate(starts):
            chunk = blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"gemv_tiled_kernel" not in chunk:
                continue
            part, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"co{i}.o")
            open(part, "wb").write(chunk)
            r = subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            asm = subprocess.run([tools[2], "-d", "-C", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            for key, targs in HEADLINE.items():
                m = re.search(r"^[0-9a-f]+ <void gptq::gemv_tiled_kernel" + re.escape(targs) + r"\(gptq::TiledParams\)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", asm, re.S | re.M)
                if m:
                    out[key] = [ln.split("//")[0].strip() for ln in m.group(1).splitlines() if ln.strip()]
    return out


def _head(ins):
    first = next(i for i, s in enumerate(ins) if s.split()[0] == "global_load_dwordx4")          # (the DMAs are global_load_lds_dwordx4)
    return ins[:first]


def _vregs(operand):
    """The vector registers an operand names: v7 -> {7}, v[2:3] -> {2, 3}; anything else -> {}."""
    m = re.fullmatch(r"v(\d+)", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def _readfirstlane_fed_by_cndmask(head):
    """Indices of v_readfirstlane_b32 whose source derives from a v_cndmask_b32 through vector instructions of the head."""
    tainted, hits = set(), []
    for i, s in enumerate(head):
        op, _, rest = s.partition(" ")
        if not op.startswith("v_"):
            continue
        ops = [o.strip() for o in rest.split(",")]
        srcs = set().union(*[_vregs(o) for o in ops[1:]]) if len(ops) > 1 else set()
        if op == "v_readfirstlane_b32":
            if srcs & tainted:
                hits.append(i)
            continue
        dst = _vregs(ops[0])
        if op.startswith("v_cndmask_b32") or (srcs & tainted):
            tainted |= dst
        else:
            tainted -= dst
    return hits


def test_headline_kernels_reach_their_first_weight_load_after_one_scalar_round_trip():
    bodies = _bodies()
    assert set(bodies) == set(HEADLINE), sorted(bodies)
    for key, ins in bodies.items():
        head = _head(ins)
        wait = next((i for i, s in enumerate(head) if s.startswith("s_waitcnt") and "lgkmcnt" in s), len(head))
        late = [(i, s) for i, s in enumerate(head) if s.startswith("s_load_") and i > wait]
        assert any(s.startswith("s_load_") for s in head[:wait]), (key, "no kernel-argument load in front of the first wait?")
        assert not late, (key, "a scalar load behind the first lgkmcnt wait, in front of the first weight load", late[:4])
        fed = _readfirstlane_fed_by_cndmask(head)
        assert not fed, (key, "a v_readfirstlane_b32 fed by a v_cndmask_b32: the selector is on the vector unit", [(i, head[i]) for i in fed])
        assert len(head) <= BOUND[key], (key, len(head), BOUND[key])
