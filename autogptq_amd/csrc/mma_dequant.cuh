// mma_dequant.cuh -- the device primitives every matrix-core kernel family shares, one definition each: the bit casts around the MFMA builtins, the
// 32x32x16 and 16x16x32 matrix-core steps (Mma32, Mma16), the packed-register helpers (and_or, bf16_scaled_pair, pack4, unpack8, swz) and the one-column
// magic-number dequantisation of the decode copy (Deq1, Deq1_3, Deq1_8, Deq1_2).  The 0x6400 arithmetic below is what makes the outputs bit-exact against
// the reference: a fix to it belongs here and nowhere else.  The STATEMENT LAYOUT of a dequant body is part of the kernels that inline it -- it reaches
// the instruction scheduler -- so a change to one is checked with tools/isa_same.py on every translation unit that includes this header.
#pragma once
#include "common.cuh"

namespace gptq {

typedef unsigned u32x3 __attribute__((ext_vector_type(3)));

// ---- bit casts (by value: see common.cuh, as_f16x2) ----------------------------------------------------------------------------------------------
__device__ __forceinline__ f16x8 as_f16x8(u32x4 v) { return __builtin_bit_cast(f16x8, v); }
__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ unsigned f16x2_bits(f16x2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ unsigned short t_bits(f16 v) { return __builtin_bit_cast(unsigned short, v); }
__device__ __forceinline__ unsigned short t_bits(bf16 v) { return __builtin_bit_cast(unsigned short, v); }

// (a & mask) | orv in one VALU op (hipcc emits v_and + v_or for the C expression: VOP3 takes no literals on gfx9).  Safe in the 128 x 128-per-wave
// kernels too, where all 256 accumulator registers are live.
__device__ __forceinline__ unsigned and_or(unsigned a, unsigned mask, unsigned orv) {
    unsigned r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(mask), "v"(orv));
    return r;
}
// the same in plain C, scheduled and register-allocated by hipcc: what gemm_mid.hip uses
__device__ __forceinline__ unsigned and_or_c(unsigned q, unsigned mask, unsigned magic) { return (q & mask) | magic; }

// ---- matrix-core steps: operands as four packed words per lane, fp32 accumulators ----------------------------------------------------------------------
template <typename T> struct Mma32;            // v_mfma_f32_32x32x16
template <> struct Mma32<f16> {
    static __device__ __forceinline__ f32x16 run(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(as_f16x8(a), as_f16x8(b), c, 0, 0, 0);
    }
};
template <> struct Mma32<bf16> {
    static __device__ __forceinline__ f32x16 run(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a), as_bf16x8(b), c, 0, 0, 0);
    }
};
template <typename T> struct Mma16;            // v_mfma_f32_16x16x32; fp32 operands: four v_mfma_f32_16x16x4, one per word
template <> struct Mma16<f16> {
    static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(as_f16x8(a), as_f16x8(b), c, 0, 0, 0);
    }
};
template <> struct Mma16<bf16> {
    static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a), as_bf16x8(b), c, 0, 0, 0);
    }
};
template <> struct Mma16<float> {
    static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(as_f32(a.x), as_f32(b.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(as_f32(a.y), as_f32(b.y), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(as_f32(a.z), as_f32(b.z), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(as_f32(a.w), as_f32(b.w), c, 0, 0, 0);
        return c;
    }
};

// ---- packing ------------------------------------------------------------------------------------------------------------------------------------------
// four fp32 accumulators -> four T (RNE) in two words
template <typename T> __device__ __forceinline__ u32x2 pack4(f32x4 v) {
    struct { T a, b, c, d; } o{DType<T>::from_f32(v[0]), DType<T>::from_f32(v[1]), DType<T>::from_f32(v[2]), DType<T>::from_f32(v[3])};
    return __builtin_bit_cast(u32x2, o);
}
// eight T of a 16-byte load -> fp32
template <typename T>
__device__ __forceinline__ void unpack8(u32x4 v, float (&f)[8]) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(w[c >> 1] >> (16 * (c & 1)))));
}
// byte offset of 16-byte slot s of row r in an LDS image of 128-byte rows (8 slots), XOR-swizzled so that a 16-lane ds_read_b128 group is conflict free
__device__ __forceinline__ int swz(int r, int s) { return r * 128 + ((s ^ ((r >> 1) & 7)) << 4); }

// ---- bf16: (w - z) exact in packed fp16, times the scale in fp32 (exact product), ONE rounding to bf16 -- the reference's scales * (weight - zeros) ------
__device__ __forceinline__ unsigned bf16_scaled_pair(f16x2 h, float sc) {
    // v_fma_mix_f32 reads either half of the packed fp16 register directly (fp32 result): no separate v_cvt_f32_f16
    const unsigned hb = __builtin_bit_cast(unsigned, h);
    float lo, hi;
    asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(lo) : "v"(hb), "v"(sc));
    asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(hi) : "v"(hb), "v"(sc));
    const bf16x2 v = {(bf16)lo, (bf16)hi};
    return __builtin_bit_cast(unsigned, v);
}
template <typename T> struct Scale4;           // the 4 columns' scales and the last step of every pair: (w - z) * scale, rounded once to T
template <> struct Scale4<f16> {
    f16x2 s2[4];
    __device__ __forceinline__ void setup(u32x2 s) {
#pragma unroll
        for (int col = 0; col < 4; ++col) {
            const unsigned sw = s[col >> 1];
            s2[col] = as_f16x2(((col & 1) ? (sw >> 16) : (sw & 0xffffu)) * 0x00010001u);
        }
    }
    __device__ __forceinline__ unsigned mul(f16x2 h, int col) const { return f16x2_bits(h * s2[col]); }
};
template <> struct Scale4<bf16> {
    float s[4];
    __device__ __forceinline__ void setup(u32x2 sv) {
#pragma unroll
        for (int col = 0; col < 4; ++col) {
            const unsigned sw = sv[col >> 1];
            s[col] = (float)__builtin_bit_cast(bf16, (unsigned short)((col & 1) ? (sw >> 16) : (sw & 0xffffu)));
        }
    }
    __device__ __forceinline__ unsigned mul(f16x2 h, int col) const { return bf16_scaled_pair(h, s[col]); }
};

// ---- one-column dequantisation ------------------------------------------------------------------------------------------------------------------------
// 4 bits: one column's constants (scale bits, zero-point as used), one word = 8 consecutive k in the slot order k0,k4,k1,k5,k2,k6,k3,k7 at a time:
// (q & 0x000f000f) | 0x64006400 is the half2 (1024 + w_k, 1024 + w_k+4); adding c1 = -(1024 + z) leaves w - z exactly (the high nibbles: times 1/16, plus
// c2 = c1 + 960 = -(64 + z)), then x scale with ONE rounding to T: the reference's scales * (w - z), bit for bit.
template <typename T> struct Deq1;
template <> struct Deq1<f16> {
    f16x2 s2, c1, c2;
    __device__ __forceinline__ void setup(unsigned sraw, unsigned z) {
        const f16x2 k960 = {(f16)960.f, (f16)960.f};
        s2 = as_f16x2(sraw * 0x00010001u);
        c1 = as_f16x2(z * 0x00010001u + 0xE400E400u);                // -(1024 + z)
        c2 = c1 + k960;                                               // -(64 + z)
    }
    __device__ __forceinline__ u32x4 frag(unsigned q) const {
        const unsigned q8 = q >> 8;
        const f16x2 r16 = {(f16)0.0625f, (f16)0.0625f};
        const f16x2 h0 = as_f16x2(and_or(q, 0x000f000fu, 0x64006400u)) + c1;
        const f16x2 h1 = as_f16x2(and_or(q, 0x00f000f0u, 0x64006400u)) * r16 + c2;
        const f16x2 h2 = as_f16x2(and_or(q8, 0x000f000fu, 0x64006400u)) + c1;
        const f16x2 h3 = as_f16x2(and_or(q8, 0x00f000f0u, 0x64006400u)) * r16 + c2;
        return u32x4{f16x2_bits(h0 * s2), f16x2_bits(h1 * s2), f16x2_bits(h2 * s2), f16x2_bits(h3 * s2)};
    }
};
template <> struct Deq1<bf16> {
    float s;
    f16x2 c1, c2;
    __device__ __forceinline__ void setup(unsigned sraw, unsigned z) {
        const f16x2 k960 = {(f16)960.f, (f16)960.f};
        s = (float)__builtin_bit_cast(bf16, (unsigned short)sraw);
        c1 = as_f16x2(z * 0x00010001u + 0xE400E400u);
        c2 = c1 + k960;
    }
    __device__ __forceinline__ u32x4 frag(unsigned q) const {
        const unsigned q8 = q >> 8;
        const f16x2 r16 = {(f16)0.0625f, (f16)0.0625f};
        const f16x2 h0 = as_f16x2(and_or(q, 0x000f000fu, 0x64006400u)) + c1;
        const f16x2 h1 = as_f16x2(and_or(q, 0x00f000f0u, 0x64006400u)) * r16 + c2;
        const f16x2 h2 = as_f16x2(and_or(q8, 0x000f000fu, 0x64006400u)) + c1;
        const f16x2 h3 = as_f16x2(and_or(q8, 0x00f000f0u, 0x64006400u)) * r16 + c2;
        return u32x4{bf16_scaled_pair(h0, s), bf16_scaled_pair(h1, s), bf16_scaled_pair(h2, s), bf16_scaled_pair(h3, s)};
    }
};

// 3 bits (utils.hip prepack_decode_weights_kernel<3>): word j of the lane's three holds pairs 5 j + i at bit 3 i of its halves, bit 15 / 31 = bit j of k30 / k31;
// fields inside the fp16 mantissa are read in place (gemm_wide_common.cuh: wide::Deq3 is the four-column form of the same arithmetic)
template <typename T> struct Deq1_3 {
    Scale4<T> sc;                                                  // (column 0 of it)
    f16x2 c0, c1, c2;
    __device__ __forceinline__ void setup(unsigned sraw, unsigned z) {
        sc.setup(u32x2{sraw & 0xffffu, 0u});
        c0 = as_f16x2(z * 0x00010001u + 0xE400E400u);                 // -(1024 + z)
        c1 = as_f16x2(z * 0x00080008u + 0xD800D800u);                 // -(128 + z)
        c2 = as_f16x2(z * 0x00400040u + 0xCC00CC00u);                 // -(16 + z)
    }
    __device__ __forceinline__ f16x2 p0(unsigned q) const { return as_f16x2(and_or(q, 0x00070007u, 0x64006400u)) + c0; }
    __device__ __forceinline__ f16x2 p1(unsigned q) const {
        const f16x2 rr = {(f16)0.125f, (f16)0.125f};
        return as_f16x2(and_or(q, 0x00380038u, 0x64006400u)) * rr + c1;
    }
    __device__ __forceinline__ f16x2 p2(unsigned q) const {
        const f16x2 rr = {(f16)0.015625f, (f16)0.015625f};
        return as_f16x2(and_or(q, 0x01c001c0u, 0x64006400u)) * rr + c2;
    }
    __device__ __forceinline__ u32x4 frag(const u32x3& w, int ks) const {      // k = 8 ks .. 8 ks + 7 of the lane's 32
        f16x2 h[4];
        if (ks == 0) {
            h[0] = p0(w[0]); h[1] = p1(w[0]); h[2] = p2(w[0]); h[3] = p1(w[0] >> 6);
        } else if (ks == 1) {
            h[0] = p2(w[0] >> 6); h[1] = p0(w[1]); h[2] = p1(w[1]); h[3] = p2(w[1]);
        } else if (ks == 2) {
            const unsigned q6 = w[1] >> 6;
            h[0] = p1(q6); h[1] = p2(q6); h[2] = p0(w[2]); h[3] = p1(w[2]);
        } else {
            const unsigned q6 = w[2] >> 6;
            unsigned t = (w[0] >> 15) & 0x00010001u;
            t = and_or(w[1] >> 14, 0x00020002u, t);
            t = and_or(w[2] >> 13, 0x00040004u, t);
            h[0] = p2(w[2]); h[1] = p1(q6); h[2] = p2(q6); h[3] = p0(t);
        }
        return u32x4{sc.mul(h[0], 0), sc.mul(h[1], 0), sc.mul(h[2], 0), sc.mul(h[3], 0)};
    }
};
// 8 bits: stored byte p of word w = k 4 w + {0, 2, 1, 3}[p]
template <typename T> struct Deq1_8 {
    Scale4<T> sc;
    f16x2 c1;
    __device__ __forceinline__ void setup(unsigned sraw, unsigned z) {
        sc.setup(u32x2{sraw & 0xffffu, 0u});
        c1 = as_f16x2(z * 0x00010001u + 0xE400E400u);
    }
    __device__ __forceinline__ u32x4 frag(unsigned q0, unsigned q1) const {
        const f16x2 h0 = as_f16x2(and_or(q0, 0x00ff00ffu, 0x64006400u)) + c1;
        const f16x2 h1 = as_f16x2(and_or(q0 >> 8, 0x00ff00ffu, 0x64006400u)) + c1;
        const f16x2 h2 = as_f16x2(and_or(q1, 0x00ff00ffu, 0x64006400u)) + c1;
        const f16x2 h3 = as_f16x2(and_or(q1 >> 8, 0x00ff00ffu, 0x64006400u)) + c1;
        return u32x4{sc.mul(h0, 0), sc.mul(h1, 0), sc.mul(h2, 0), sc.mul(h3, 0)};
    }
};
// 2 bits: fields i = 0..3 at bit 2 i of both halves of w (pairs (i, 4 + i)), read in place like the 3-bit ones: OR-ing the exponent of 1024 over field i
// gives 1024 + 4^i f, and one fma with 4^-i and -(1024 / 4^i + z) leaves f - z exactly
template <typename T> struct Deq1_2 {
    Scale4<T> sc;                                                  // (column 0 of it)
    f16x2 c0, c1, c2, c3;
    __device__ __forceinline__ void setup(unsigned sraw, unsigned z) {
        sc.setup(u32x2{sraw & 0xffffu, 0u});
        c0 = as_f16x2(z * 0x00010001u + 0xE400E400u);                 // -(1024 + z)
        c1 = as_f16x2(z * 0x00040004u + 0xDC00DC00u);                 // -(256 + z)
        c2 = as_f16x2(z * 0x00100010u + 0xD400D400u);                 // -(64 + z)
        c3 = as_f16x2(z * 0x00400040u + 0xCC00CC00u);                 // -(16 + z)
    }
    __device__ __forceinline__ f16x2 p0(unsigned q) const { return as_f16x2(and_or(q, 0x00030003u, 0x64006400u)) + c0; }
    __device__ __forceinline__ f16x2 p1(unsigned q) const {
        const f16x2 rr = {(f16)0.25f, (f16)0.25f};
        return as_f16x2(and_or(q, 0x000c000cu, 0x64006400u)) * rr + c1;
    }
    __device__ __forceinline__ f16x2 p2(unsigned q) const {
        const f16x2 rr = {(f16)0.0625f, (f16)0.0625f};
        return as_f16x2(and_or(q, 0x00300030u, 0x64006400u)) * rr + c2;
    }
    __device__ __forceinline__ f16x2 p3(unsigned q) const {
        const f16x2 rr = {(f16)0.015625f, (f16)0.015625f};
        return as_f16x2(and_or(q, 0x00c000c0u, 0x64006400u)) * rr + c3;
    }
    __device__ __forceinline__ u32x4 frag(unsigned w) const {         // k order (0,4,1,5,2,6,3,7)
        return u32x4{sc.mul(p0(w), 0), sc.mul(p1(w), 0), sc.mul(p2(w), 0), sc.mul(p3(w), 0)};
    }
};
template <typename T, int BITS> struct DeqSel { typedef Deq1<T> type; };
template <typename T> struct DeqSel<T, 3> { typedef Deq1_3<T> type; };
template <typename T> struct DeqSel<T, 8> { typedef Deq1_8<T> type; };

}  // namespace gptq
