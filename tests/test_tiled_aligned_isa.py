"""CPU: the ALIGNED form of the decode-copy kernel's K loop, read from the BUILT library (no GPU).  The aligned twins of the three instantiations of
the Llama-7B decode step -- q|k|v (<4, 1, 4, f16, 8, 0, 2>), o / down (<4, 1, 2, f16, 16, 0, 2>) and the two-strip gate|up launch (<4, 1, 4, f16, 8, 6, 2>); the last
template argument is the flag word, bit 1 = aligned -- are disassembled next to their general forms with the extraction of test_tiled_loop_isa.py (imported, not
copied: the same loop block, the steady state of the K loop).

What is asserted of every aligned twin:
  (a) its loop block holds no v_mad_u64_u32 (LDS addresses are 32-bit), no v_cmp (no compare with K: liveness in the steady loop is the loop's own condition) and
      no v_min_i32 (no clamp of the group index);
  (b) its vector-ALU instructions per chunk (every v_* of the block but the matrix-core steps, over U) are at least 8 fewer than those of the matching GENERAL
      instantiation in the same library -- nothing hard-coded;
  (c) as in the general form: every vmcnt wait of the block leaves >= U - 1 loads in flight, and U weight loads lie behind its first matrix-core step;
  (d) no scratch, no spill, at most 128 VGPRs (kernel metadata, as test_kernel_resources.py reads it).
Skipped where the LLVM tools or the library are missing (the product needs neither)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_kernel_resources as KR          # noqa: E402
import test_tiled_loop_isa as TL            # noqa: E402

GENERAL = dict(TL.HEADLINE)
ALIGNED = {k: v[:-len("0>")] + "2>" for k, v in GENERAL.items()}
MANGLED = {"qkv": "ILi4ELi1ELi4EDF16_Li8ELi0ELi2EE", "o_down": "ILi4ELi1ELi2EDF16_Li16ELi0ELi2EE", "gate_up": "ILi4ELi1ELi4EDF16_Li8ELi6ELi2EE"}


def _bodies_of(names):
    saved = TL.HEADLINE
    TL.HEADLINE = names                     # _bodies() looks its kernels up in this table
    try:
        return TL._bodies()
    finally:
        TL.HEADLINE = saved


def _valu(ops):
    return [s for s in ops if s.startswith("v_") and not s.startswith("v_mfma")]


def _block(key, ins):
    spans = TL._loop_blocks(ins)
    assert len(spans) == 1, (key, "one steady loop block with matrix-core steps expected", spans)
    a, z = spans[0]
    return [s for _, s, _ in ins[a:z + 1]]


def test_aligned_twins_of_the_headline_kernels_drop_the_index_arithmetic():
    gen, al = _bodies_of(GENERAL), _bodies_of(ALIGNED)
    assert set(gen) == set(GENERAL) and set(al) == set(ALIGNED), (sorted(gen), sorted(al))
    for key in GENERAL:
        U = TL.DEPTH[key]
        g_ops, a_ops = _block(key, gen[key]), _block(key + " (aligned)", al[key])
        mf = [i for i, s in enumerate(a_ops) if s.startswith("v_mfma")]
        assert len(mf) == U * TL.MFMA_PER_CHUNK, (key, len(mf))
        for bad in ("v_mad_u64_u32", "v_cmp", "v_min_i32"):
            hit = [s for s in a_ops if s.startswith(bad)]
            assert not hit, (key, "index arithmetic left in the aligned loop block", hit)
        per_g, per_a = len(_valu(g_ops)) / U, len(_valu(a_ops)) / U
        print(f"{key}: vector-ALU instructions per chunk, general {per_g:.2f}, aligned {per_a:.2f}")
        assert per_g - per_a >= 8, (key, "VALU per chunk, general / aligned", per_g, per_a)
        waits = [(i, TL._vmcnt(s)) for i, s in enumerate(a_ops) if TL._vmcnt(s) is not None]
        assert [n for i, n in waits if i < mf[0]], (key, "no vmcnt wait in front of the block's first matrix-core step")
        assert all(n >= U - 1 for _, n in waits), (key, "a wait inside the loop block leaves fewer than U - 1 loads in flight", waits)
        loads = [i for i, s in enumerate(a_ops) if s.split()[0] == "global_load_dwordx4"]
        assert len([i for i in loads if i > mf[0]]) >= U, (key, "weight loads behind the first matrix-core step", loads, mf[0])


def test_aligned_twins_fit_the_register_budget_without_scratch():
    ks = KR._kernels()
    for key, tag in MANGLED.items():
        hit = {n: v for n, v in ks.items() if "gemv_tiled_kernel" + tag in n}
        assert len(hit) == 1, (key, sorted(hit))
        v = next(iter(hit.values()))
        assert not (v["spill"] or 0) and not (v["scratch"] or 0) and (v["vgpr"] or 0) <= 128, (key, v)
