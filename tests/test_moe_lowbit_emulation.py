"""CPU (-m "not gpu"): the 2- and 3-bit forms of moe_gemm_kernel (csrc/moe.hip Proj<T>::load / frag / group, rowsk::Deq1_3 / Deq1_2 in
csrc/gemm_rows_kernel.cuh) restated in numpy, instruction for instruction (row choice, v_alignbit_b32, shifts, masks, and-or with the exponent of 1024,
packed fp16 fma), on random CHECKPOINT words and checked against ``oracle.unpack_rows`` / ``unpack_zeros``.  It pins

  * which checkpoint rows a lane (k-slot ks = lane >> 4) reads for its 8 consecutive k of a 32-deep step, and that none lies outside the step,
  * which field lands in which half of which register: pairs (0,4) (1,5) (2,6) (3,7), the order ``order_a`` applies to the A fragment for 4 bits,
  * that every fp16 intermediate is exact (the decode is exact, not merely close) for both zero-point conventions (wrap: 0..maxq, no-wrap: 1..maxq + 1),
  * the zero points of a lane's column quad, the straddling quads of the 3-bit rows (n % 32 in {8, 20}) included, without a read past the row."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gptq_oracle as O  # noqa: E402

MAGIC = 0x64006400
STEPS, N = 4, 64                     # K = 128: four 32-deep steps; one 64-column block


def alignbit(hi, lo, sh):
    """v_alignbit_b32: low 32 bits of {hi, lo} >> (sh & 31)."""
    return (((int(hi) << 32) | int(lo)) >> (sh & 31)) & 0xffffffff


def halves(u):
    return np.array([u & 0xffff, (u >> 16) & 0xffff], dtype=np.uint16).view(np.float16)


def pk_fma(t, mask, scale, c):
    """as_f16x2((t & mask) | magic) * scale + c (packed fp16); asserts the product and the sum are exact in fp16, so fusing them or not is the same."""
    v = halves((t & mask) | MAGIC).astype(np.float64)
    m = v * scale
    assert np.all(m.astype(np.float16).astype(np.float64) == m), "product not exact in fp16"
    r = m + c
    r16 = r.astype(np.float16)
    assert np.all(r16.astype(np.float64) == r), "intermediate not exact in fp16"
    return r16


def const16(z, step, base):
    """setup(): an integer add on the fp16 bit pattern of -(2^m): z * step + base, one half."""
    return float(np.array([(z * step + base) & 0xffff], dtype=np.uint16).view(np.float16)[0])


def consts3(z):
    return const16(z, 0x0001, 0xE400), const16(z, 0x0008, 0xD800), const16(z, 0x0040, 0xCC00)


def consts2(z):
    return const16(z, 0x0001, 0xE400), const16(z, 0x0004, 0xDC00), const16(z, 0x0010, 0xD400), const16(z, 0x0040, 0xCC00)


def frag3(q0, q1, ks, z):
    """Proj::frag at 3 bits: the 24-bit window of the lane, its halves moved to bits 0 / 16, Deq1_3's readers p0, p1, p2, p1(w >> 6)."""
    c0, c1, c2 = consts3(z)
    v = alignbit(q1, q0, (24 * ks) & 31) & 0xffffff
    w = (v & 0xfff) | ((v >> 12) << 16)
    return [pk_fma(w, 0x00070007, 1.0, c0), pk_fma(w, 0x00380038, 0.125, c1), pk_fma(w, 0x01c001c0, 1 / 64, c2), pk_fma(w >> 6, 0x00380038, 0.125, c1)]


def frag2(q0, ks, z):
    """Proj::frag at 2 bits: half ks & 1 of the word, its bytes moved to the halves, Deq1_2's readers p0 .. p3."""
    c0, c1, c2, c3 = consts2(z)
    v = int(q0) >> (16 * (ks & 1))
    w = (v & 0xff) | ((v & 0xff00) << 8)
    return [pk_fma(w, 0x00030003, 1.0, c0), pk_fma(w, 0x000c000c, 0.25, c1), pk_fma(w, 0x00300030, 1 / 16, c2), pk_fma(w, 0x00c000c0, 1 / 64, c3)]


def rows3(st, ks):
    """Proj::load at 3 bits: the two checkpoint rows of the lane's window."""
    lo = (24 * ks) >> 5
    hi = min(lo + 1, 2)
    return 3 * st + lo, 3 * st + hi


def zrange(bits, zero_mode):
    maxq = (1 << bits) - 1
    return range(0, maxq + 1) if zero_mode == "wrap" else range(1, maxq + 2)


def test_constants_are_exact_fp16_bit_patterns():
    for z in range(0, 9):
        assert consts3(z) == (-(1024 + z), -(128 + z), -(16 + z))
    for z in range(0, 5):
        assert consts2(z) == (-(1024 + z), -(256 + z), -(64 + z), -(16 + z))


@pytest.mark.parametrize("zero_mode", ["wrap", "nowrap"])
def test_3bit_window_of_every_step_and_k_slot(zero_mode):
    rng = np.random.default_rng(3)
    q = rng.integers(0, 1 << 32, (STEPS * 3, N), dtype=np.uint64).astype(np.uint32)
    f = O.unpack_rows(q.view(np.int32), 3).astype(np.int64)                   # [K, N]
    for st in range(STEPS):
        for ks in range(4):
            r0, r1 = rows3(st, ks)
            assert 3 * st <= r0 <= r1 <= 3 * st + 2                          # k-slot 3 of the last step stays inside the tensor
            for n in range(N):
                for z in zrange(3, zero_mode):
                    h = frag3(q[r0, n], q[r1, n], ks, z)
                    for i in range(4):
                        k = 32 * st + 8 * ks + i
                        assert (float(h[i][0]), float(h[i][1])) == (f[k, n] - z, f[k + 4, n] - z), (st, ks, n, i, z)
                    if n >= 4:                                                # (every column of a few, every z; then one z per column)
                        break


@pytest.mark.parametrize("zero_mode", ["wrap", "nowrap"])
def test_2bit_half_word_of_every_step_and_k_slot(zero_mode):
    rng = np.random.default_rng(2)
    q = rng.integers(0, 1 << 32, (STEPS * 2, N), dtype=np.uint64).astype(np.uint32)
    f = O.unpack_rows(q.view(np.int32), 2).astype(np.int64)
    for st in range(STEPS):
        for ks in range(4):
            r = 2 * st + (ks >> 1)
            for n in range(N):
                for z in zrange(2, zero_mode):
                    h = frag2(q[r, n], ks, z)
                    for i in range(4):
                        k = 32 * st + 8 * ks + i
                        assert (float(h[i][0]), float(h[i][1])) == (f[k, n] - z, f[k + 4, n] - z), (st, ks, n, i, z)


def test_pair_order_is_the_4bit_one():
    """order_a(bits != 8): A registers (k0,k4) (k1,k5) (k2,k6) (k3,k7) -- the halves of the weight registers above hold the same k."""
    x = np.arange(8) + 100
    v = [int(x[2 * r]) | (int(x[2 * r + 1]) << 16) for r in range(4)]            # 8 consecutive k, two per register

    def perm(s0, s1, sel):
        b = [(s1 >> (8 * i)) & 0xff for i in range(4)] + [(s0 >> (8 * i)) & 0xff for i in range(4)]
        return sum(b[(sel >> (8 * i)) & 0xff] << (8 * i) for i in range(4))

    a = [perm(v[2], v[0], 0x05040100), perm(v[2], v[0], 0x07060302), perm(v[3], v[1], 0x05040100), perm(v[3], v[1], 0x07060302)]
    assert [(r & 0xffff, r >> 16) for r in a] == [(100 + i, 104 + i) for i in range(4)]


@pytest.mark.parametrize("zero_mode", ["wrap", "nowrap"])
@pytest.mark.parametrize("bits", [2, 3])
def test_zero_points_of_every_column_quad(bits, zero_mode):
    """Proj::group: 4 fields at bit bits * n of the qzeros row; the second word is read only when the quad straddles, and then it exists."""
    rng = np.random.default_rng(bits)
    Nz = 192                                                                  # three 64-column blocks: the last one starts on an odd multiple of 64
    words = Nz // 32 * bits
    qz = rng.integers(0, 1 << 32, (2, words), dtype=np.uint64).astype(np.uint32)
    want = O.unpack_zeros(qz.view(np.int32), bits, zero_mode)                 # [G, N] as used
    maxq = (1 << bits) - 1
    straddlers = set()
    for g in range(2):
        for n in range(0, Nz, 4):
            bit = bits * n
            wi, sh = bit >> 5, bit & 31
            zw = int(qz[g, wi]) >> sh
            if sh + 4 * bits > 32:
                assert wi + 1 < words, "a straddling quad at the end of the row"
                zw |= (int(qz[g, wi + 1]) << (32 - sh)) & 0xffffffff
                straddlers.add(n % 32)
            for c in range(4):
                z = ((zw >> (bits * c)) & maxq) + 1
                if zero_mode == "wrap":
                    z &= maxq
                assert z == want[g, n + c], (g, n, c)
    assert straddlers == ({8, 20} if bits == 3 else set())
