"""CPU: the K loop of the decode-copy kernel, read from the BUILT library (no GPU).  The three instantiations of the Llama-7B decode step -- q|k|v
(<4, 1, 4, f16, 8, 0, 0>, U = 4 chunks per wave and pass), o / down (<4, 1, 2, f16, 16, 0, 0>, U = 2) and the two-strip gate|up launch (<4, 1, 4, f16, 8, 6, 0>,
U = 4) -- are disassembled as test_tiled_tail_isa.py does (its own copy of the extraction, which here keeps each instruction's address and branch target), and
the LOOP BLOCK is taken to be the span from the target of a backward branch to that branch which holds matrix-core steps: the steady state of the K loop
(the wave's last pass is peeled behind it and requests nothing).

What is asserted, and what the parent commit had:
  (a) there is such a block, and it holds the matrix-core steps of U chunks (8 v_mfma per 4-bit chunk at one row);
  (b) the first s_waitcnt naming vmcnt in front of the block's first v_mfma leaves at least U - 1 loads outstanding, and so does every later one of the block:
      the weight stream does not drain inside the steady state
      -- parent: vmcnt(U - 1) in front of the first chunk, then U - 2 .. 0: nothing in flight under the last chunk of every pass;
  (c) at least U global_load_dwordx4 of the block lie BEHIND its first v_mfma: the refill of a chunk's registers is issued when the chunk has been decoded,
      between the matrix-core steps of this chunk and of the next one (for the last chunk of the block: of the next trip), not as one burst above the first
      -- parent: all U loads of the block in front of its first v_mfma.
Only these opcodes are looked at.  Skipped where the LLVM tools or the library are missing (the product needs neither)."""
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
DEPTH = {"qkv": 4, "o_down": 2, "gate_up": 4}          # U: chunks a wave has in flight
MFMA_PER_CHUNK = 8                                      # 4-bit, one row: 32 k per lane = 8 steps of 4 k


def _bodies():
    """{kernel: [(address, instruction, branch target address or None), ...]} of the three kernels."""
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
                m = re.search(r"^([0-9a-f]+) <void gptq::gemv_tiled_kernel" + re.escape(targs) + r"\(gptq::TiledParams\)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", asm, re.S | re.M)
                if not m:
                    continue
                base, ins = int(m.group(1), 16), []
                for ln in m.group(2).splitlines():
                    if not ln.strip():
                        continue
                    text, _, note = ln.partition("//")
                    am = re.match(r"\s*([0-9A-Fa-f]+):", note)
                    tm = re.search(r"\+0x([0-9A-Fa-f]+)>\s*$", note)
                    ins.append((int(am.group(1), 16) if am else None, text.strip(), base + int(tm.group(1), 16) if tm and text.strip().startswith(("s_cbranch", "s_branch")) else None))
                out[key] = ins
    return out


def _loop_blocks(ins):
    """[(first, last)] instruction index spans of the innermost backward branches whose span holds a v_mfma."""
    at = {a: i for i, (a, _, _) in enumerate(ins) if a is not None}
    spans = []
    for i, (a, s, t) in enumerate(ins):
        if t is not None and a is not None and t <= a and t in at and any(x[1].startswith("v_mfma") for x in ins[at[t]:i + 1]):
            spans.append((at[t], i))
    return [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]      # innermost: a later backward jump may span the loop and the peeled pass


def _vmcnt(s):
    m = re.search(r"vmcnt\((\d+)\)", s)
    return int(m.group(1)) if s.startswith("s_waitcnt") and m else None


def test_headline_kernels_keep_the_weight_stream_in_flight_inside_the_k_loop():
    bodies = _bodies()
    assert set(bodies) == set(HEADLINE), sorted(bodies)
    for key, ins in bodies.items():
        U = DEPTH[key]
        spans = _loop_blocks(ins)
        assert spans, (key, "no loop block with matrix-core steps: is the K loop gone?")
        for a, z in spans:
            ops = [s for _, s, _ in ins[a:z + 1]]
            mf = [i for i, s in enumerate(ops) if s.startswith("v_mfma")]
            assert len(mf) == U * MFMA_PER_CHUNK, (key, "matrix-core steps in the loop block", len(mf), U * MFMA_PER_CHUNK)
            waits = [(i, _vmcnt(s)) for i, s in enumerate(ops) if _vmcnt(s) is not None]
            first = [n for i, n in waits if i < mf[0]]
            assert first, (key, "no vmcnt wait in front of the block's first matrix-core step")
            assert first[0] >= U - 1, (key, "the first wait of the loop block drains the weight stream", first[0], U - 1)
            assert all(n >= U - 1 for _, n in waits), (key, "a wait inside the loop block leaves fewer than U - 1 loads in flight", waits)
            loads = [i for i, s in enumerate(ops) if s.split()[0] == "global_load_dwordx4"]
            behind = [i for i in loads if i > mf[0]]
            assert len(behind) >= U, (key, "weight loads of the loop block behind its first matrix-core step", len(behind), "of", len(loads), "need", U)
