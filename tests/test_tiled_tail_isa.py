"""CPU: the tail of the decode-copy kernel, read from the BUILT library (no GPU).  The three instantiations of the Llama-7B decode step -- q|k|v
(<4, 1, 4, f16, 8, 0, 0>), o / down (<4, 1, 2, f16, 16, 0, 0>) and the two-strip gate|up launch (<4, 1, 4, f16, 8, 6, 0>) -- are disassembled as
test_kernel_resources.py does, and the HOT TAIL is taken to be what lies between the last matrix-core instruction (the end of the K loop) and the first
s_endpgm behind it: the path of a launch without K slices at the planner's wave counts.

What is asserted, and on which library each assertion holds:
  * no ds_bpermute_b32 in the hot tail           -- parent: 3 / 3 / 2 (the two k-slot shuffles, the cross-wave xor loop); now 0: v_permlane16_swap / v_permlane32_swap
  * no s_load in the hot tail                    -- parent: 13 in the two single-strip kernels (ksplit, blockDim, M, nsum, the granule pointers .. re-read from the
                                                    kernel-argument segment behind the K loop); now 0.  (The two-strip kernel had none: it passes on both.)
  * at most two s_barrier in it                  -- parent: 3 in the single-strip kernels (the K-slice owner's barrier sat on the path); now 2, one of them skipped
                                                    (the staging barrier of a workgroup with no chunk)
  * the hot tail is short                        -- parent: 792 / 789 / 160 instructions up to the first s_endpgm; now 138 / 74 / 90 (bound: 150)
  * the K-slice code lies BEHIND the hot s_endpgm -- its polling loop's s_sleep: parent in front of the first s_endpgm, now behind it (single-strip kernels)
Skipped where the LLVM tools or the library are missing (the product needs neither)."""
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


def _hot_tail(ins):
    last = max(i for i, s in enumerate(ins) if s.startswith("v_mfma"))
    end = next(i for i in range(last, len(ins)) if ins[i].startswith("s_endpgm"))
    return ins[last + 1:end + 1], ins[end + 1:]


def test_headline_kernels_end_in_a_straight_line_tail():
    bodies = _bodies()
    assert set(bodies) == set(HEADLINE), sorted(bodies)
    for key, ins in bodies.items():
        hot, rest = _hot_tail(ins)
        count = lambda prefix, span=hot: sum(1 for s in span if s.startswith(prefix))
        assert count("ds_bpermute_b32") == 0, (key, "a shuffle through the LDS in the hot tail")
        assert count("v_permlane16_swap") >= 1 and count("v_permlane32_swap") >= 1, (key, "the k-slot sum is not the two register swaps")
        assert count("s_load_") == 0, (key, "a kernel-argument load behind the K loop", [s for s in hot if s.startswith("s_load_")][:4])
        assert count("s_barrier") <= 2, (key, count("s_barrier"))
        assert count("ds_write") + count("ds_read") >= 2, (key, "the cross-wave sum left the hot tail?")
        assert count("global_store_short") == 1 and count("flat_store") == 0, (key, "the output store")
        assert len(hot) <= 150, (key, len(hot))
        if key != "gate_up":                                         # the multi-strip form has no K slices
            assert count("s_sleep") == 0 and count("s_sleep", rest) >= 1, (key, "the K-slice polling loop is not behind the hot s_endpgm")
