// act_int8.hip -- W4A8 (opt-in): int8 activations, 4-bit weights, the i8 matrix core (v_mfma_i32_32x32x32_i8).  Two launches:
//
//   act_quant_kernel        x [M][K] (fp16 / bf16) -> sx[m] = amax_m / 127 (IEEE fp32, true division) and xq[m][.] = (int8) rintf(x / sx[m]), one workgroup per
//                           row at a time: the row is read ONCE (16-byte vectors) into LDS while its |max| is reduced, the second pass runs from LDS.  Act-order
//                           layers: stored position i holds x[m][perm[i]] -- the order of qweight_seq and of the decode copy -- so the GEMM needs no pre-pass.
//   gemm_a8_kernel          out[m][n] = T( sx[m] * sum_g s[g][n] * I[m][g][n] + bias[n] ),  I = sum_{k in g} xq[m][k] * (q[k][n] - z[g][n])  (exact int32)
//                           on the layer's DECODE COPY (qweight_tiled / qconst_tiled, untouched).
//
// The k order.  A lane (kb, col) of the copy owns one 16-byte load = the 32 consecutive k of k-slot kb of its column; word w, nibble p = k 8 w + {0, 2, 4, 6, 1, 3,
// 5, 7}[p].  `w & 0x0F0F0F0F` is therefore four operand BYTES, k 8 w + {0, 4, 1, 5}, and `(w >> 4) & 0x0F0F0F0F` the other four, k 8 w + {2, 6, 3, 7}: a lane's load
// is two 16-byte B operands of the 32-deep i8 step, no decode.  Inside one quant group the order of k does not change an integer sum, so act_quant_kernel writes xq
// in THAT order (a8_k_of_pos) and the A fragment of a step is one 16-byte LDS read.  The halves (lane >> 5) of a step:
//   groups of 64 and more (GM 0 / 1)   half h loads k-slot 2 u + h; step 2 u takes the low nibbles of both halves, step 2 u + 1 the high ones (64 k per load pair)
//   groups of 32          (GM 2)       both halves load k-slot t; half 0 takes its low nibbles, half 1 its high ones -- step t stays inside group 4 c + t
// Which byte of a half the hardware calls which k does not matter: A and B use the same (half, byte) -> k map and the step sums over all of it.
//
// Zero-point, form (b) of the two (counted in the ISA): ((nibbles | 0x80808080) - z * 0x01010101) ^ 0x80808080 = q - z in every byte (0x80 | q >= 128 > z:
// no byte borrows), three VALU per word and nothing at the group boundary; the row-sum form would pay 64 multiply-subtracts per wave at every boundary.
//
// Workgroup = 128 rows x 128 columns x the whole K, four waves as 2 x 2, a wave = 64 x 64 = 2 x 2 tiles of 32 x 32: 64 int32 accumulators of the running group and
// 64 fp32 masters; at a group boundary master += float(I) * s (one FMA each), nothing is converted in between.  xq tiles (128 rows x 128 k = 16 KiB) come by
// global_load_lds_dwordx4 into two LDS buffers -- the lane of a DMA fetches 16-byte piece slot ^ ((row >> 1) & 7) of its row, so the 16 rows of a fragment read fall
// on all 64 banks (the swizzle of gemm_rows64_kernel) -- one barrier per chunk.  Weights and constants go from global memory to registers one chunk ahead.  No
// atomics, no exchange between waves or workgroups: bit-reproducible, capturable, and a row's bits depend on that row alone.  Rows past M repeat the last row,
// column tiles past N the last strip; neither is stored.
#include "common.cuh"
#include "launch.h"

namespace gptq {

// Both kernels are compiled WITHOUT the packed-fp32 instructions (per function here; the Makefile passes the same switch for the file).  It is a register
// matter, not a style one: with them hipcc's SLP pass turns the group fold into v_pk_fma_f32 on VGPR pairs (about 890 v_pk_* in gemm_a8_kernel), the masters
// can no longer live next to accumulators in the AGPR half, and the kernel ends at 512 registers with 164 spilled (268 bytes of scratch per lane); without them:
// 484 registers, no spill, no scratch.  Read off the code object both ways.
#if defined(__HIP_DEVICE_COMPILE__)
#define A8_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define A8_NO_PACKED_F32
#endif

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// stored position p (0 .. 127) of a chunk of xq -> the k (0 .. 127) of the chunk it holds: step t = p >> 5, half h = (p >> 4) & 1, word w and byte b of the operand
__host__ __device__ constexpr int a8_k_of_pos(int p, bool g32) {
    const int t = p >> 5, h = (p >> 4) & 1, w = (p >> 2) & 3, b = p & 3;
    const int kb = g32 ? t : 2 * (t >> 1) + h, hi = g32 ? h : (t & 1);
    return 32 * kb + 8 * w + 4 * (b & 1) + (b >> 1) + 2 * hi;
}

// ---- activation quantise ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void act_quant_body(const T* __restrict__ x, const int* __restrict__ perm, int M, int K, int Kp, int g32, float* __restrict__ sx,
                                               signed char* __restrict__ xq, char* smem, float* red) {
    T* const row = (T*)smem;
    const int tid = threadIdx.x;
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        const T* xr = x + (size_t)m * K;
        float amax = 0.f;
        for (int i = tid * 8; i < K; i += 256 * 8) {                 // K % 32 == 0, x 16-byte aligned
            const u32x4 v = *(const u32x4*)(xr + i);
            *(u32x4*)(row + i) = v;
        }
        __syncthreads();
        for (int i = tid; i < K; i += 256) amax = fmaxf(amax, fabsf(DType<T>::to_f32(row[i])));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
        if ((tid & 63) == 0) red[tid >> 6] = amax;
        __syncthreads();
        amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        const float s = amax / 127.0f;                               // true division; an all-zero row: s = 0, xq = 0
        if (tid == 0) sx[m] = s;
        for (int u = tid; u < Kp / 16; u += 256) {                   // one thread = 16 stored bytes = one operand of one MFMA step
            unsigned wds[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                unsigned v = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int p = u * 16 + w * 4 + b;
                    const int i = (p & ~127) + a8_k_of_pos(p & 127, g32 != 0);
                    int q = 0;
                    if (i < K && s != 0.f) q = (int)rintf(DType<T>::to_f32(row[perm ? perm[i] : i]) / s);
                    v |= ((unsigned)q & 255u) << (8 * b);
                }
                wds[w] = v;
            }
            *(u32x4*)(xq + (size_t)m * Kp + (size_t)u * 16) = u32x4{wds[0], wds[1], wds[2], wds[3]};
        }
        __syncthreads();                                             // the next row overwrites the staging and red[]
    }
}

// one code object for the two dtypes (a launch-uniform branch, as silu_mul_kernel: the library keeps to its kernel count)
A8_NO_PACKED_F32 __global__ void __launch_bounds__(256) act_quant_kernel(const void* __restrict__ x, const int* __restrict__ perm, int M, int K, int Kp, int g32, int dtype,
                                                        float* __restrict__ sx, signed char* __restrict__ xq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // the row, K elements of T
    __shared__ float red[4];
    if (dtype == GPTQ_F16) act_quant_body<f16>((const f16*)x, perm, M, K, Kp, g32, sx, xq, smem, red);
    else act_quant_body<bf16>((const bf16*)x, perm, M, K, Kp, g32, sx, xq, smem, red);
}

// ---- the GEMM ----------------------------------------------------------------------------------------------------------------------------------------
struct A8Params {
    const char* qw;               // decode copy: [strip][chunk][1024 bytes]
    const char* qc;               // constant records: [strip][group][48 bytes]
    const void* bias;
    void* out;
    const signed char* xq;        // [M][Kp] in a8_k_of_pos order
    const float* sx;              // [M]
    int M, N, Kp, chunks, groups, gshift, strips, npm;
    int dtype, gm;                // launch-uniform: which body of gemm_a8_kernel runs
};

// GM: 0 = group_size a multiple of 128 (group of chunk c = c >> gshift; 31: one group), 1 = 64 (k-slots 0, 1 | 2, 3), 2 = 32 (one group per k-slot)
template <typename T, int GM>
__device__ __forceinline__ void gemm_a8_body(const A8Params& p, char* xs) {
    constexpr int NL = GM == 2 ? 4 : 2;                       // 16-byte weight loads per chunk and column block
    constexpr int NG = GM == 0 ? 1 : (GM == 1 ? 2 : 4);       // groups per chunk
    constexpr int XB = 128 * 128;                             // bytes of one xq tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave >> 1, wc = wave & 1;
    const int Lb = xcd_remap(blockIdx.x, gridDim.x);
    const int pm = Lb % p.npm, pn = Lb / p.npm;               // consecutive workgroups (one XCD): the same columns, the next rows
    const int m0 = pm * 128, n0 = pn * 128 + wc * 64;
    const int c31 = lane & 31, h = lane >> 5, col = lane & 15;
    const unsigned xs_lds = lds_addr_of(xs);

    // xq DMA j of this wave (8 rows x 128 bytes, instruction 4 wave + j of the tile's 16): lane (row 8 i + (lane >> 3), slot lane & 7) fetches piece
    // slot ^ ((row >> 1) & 7), so LDS slot s of row R holds piece s ^ ((R >> 1) & 7)
    const signed char* xsrc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 8 * (4 * wave + j) + (lane >> 3);
        const int m = min(m0 + row, p.M - 1);
        xsrc[j] = p.xq + (size_t)m * p.Kp + (((lane & 7) ^ ((row >> 1) & 7)) * 16);
    }
    auto issue_x = [&](int c, int b) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_dma16(xsrc[j] + (size_t)c * 128, xs_lds + (unsigned)(b * XB + (4 * wave + j) * 1024));
    };
    // A fragment of row block rb, step t: piece 2 t + h of row 64 wr + 32 rb + c31, at slot piece ^ ((row >> 1) & 7)
    unsigned aoff[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) aoff[t] = (unsigned)((64 * wr + c31) * 128 + (((2 * t + h) ^ ((c31 >> 1) & 7)) * 16));

    // weights: column block cb = columns n0 + 32 cb + c31 -> strip (clamped: a column tile past N repeats the last strip), lane (kb, col) of the strip-chunk
    const char* wptr[2];
    const char* cptr[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int strip = min((n0 + 32 * cb + c31) >> 4, p.strips - 1);
        wptr[cb] = p.qw + (size_t)strip * p.chunks * 1024 + col * 16;
        cptr[cb] = p.qc + (size_t)strip * p.groups * 48;
    }
    struct WBuf { u32x4 w[2][NL]; unsigned cs[2][NG], cz[2][NG]; };
    auto load_w = [&](int c, WBuf& B) __attribute__((always_inline)) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int kb = GM == 2 ? i : 2 * i + h;
                B.w[cb][i] = *(const u32x4*)(wptr[cb] + (size_t)c * 1024 + kb * 256);
            }
#pragma unroll
            for (int gi = 0; gi < NG; ++gi) {
                const int grp = min(GM == 0 ? (c >> p.gshift) : NG * c + gi, p.groups - 1);
                const char* rec = cptr[cb] + (size_t)grp * 48;
                B.cs[cb][gi] = *(const unsigned short*)(rec + 2 * col);
                B.cz[cb][gi] = *(const unsigned char*)(rec + 32 + col);
            }
        }
    };

    i32x16 acc[2][2];
    f32x16 master[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[rb][cb][r] = 0;
                master[rb][cb][r] = 0.f;
            }
    // the group boundary: the exact int32 sums of the finished group go to the fp32 masters with the column's scale
    auto fold = [&](const WBuf& B, int gi) __attribute__((always_inline)) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const float s = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)B.cs[cb][gi]));
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    master[rb][cb][r] = fmaf((float)acc[rb][cb][r], s, master[rb][cb][r]);
                    acc[rb][cb][r] = 0;
                }
        }
    };
    auto compute = [&](int c, const WBuf& B, int b) __attribute__((always_inline)) {
        const char* xb = xs + b * XB;
        i32x4 a[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) a[t][rb] = *(const i32x4*)(xb + rb * 4096 + aoff[t]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int gi = GM == 0 ? 0 : (GM == 1 ? t >> 1 : t);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const unsigned zz = B.cz[cb][gi] * 0x01010101u;
                const u32x4 w = B.w[cb][GM == 2 ? t : t >> 1];
                const unsigned sh = GM == 2 ? 4u * (unsigned)h : 4u * (unsigned)(t & 1);
                i32x4 bq;
#pragma unroll
                for (int j = 0; j < 4; ++j) bq[j] = (int)(((((w[j] >> sh) & 0x0F0F0F0Fu) | 0x80808080u) - zz) ^ 0x80808080u);      // q - z, byte by byte
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) acc[rb][cb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[t][rb], bq, acc[rb][cb], 0, 0, 0);
            }
            if (GM == 2 || (GM == 1 && (t & 1))) fold(B, gi);
        }
        if (GM == 0 && (c + 1 == p.chunks || ((c + 1) >> p.gshift) != (c >> p.gshift))) fold(B, 0);
    };

    // chunk c: its xq tile and weights were issued one chunk earlier; the barrier also says every wave is done with the buffer the next tile lands in
    WBuf q[2];
    load_w(0, q[0]);
    issue_x(0, 0);
    for (int c = 0; c < p.chunks; c += 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cc = c + j;
            if (cc >= p.chunks) break;
            wait_vmcnt<0>();
            __syncthreads();
            if (cc + 1 < p.chunks) {
                issue_x(cc + 1, j ^ 1);
                load_w(cc + 1, q[j ^ 1]);
            }
            compute(cc, q[j], j);
        }
    }

    // ---- sx, bias, store: C/D layout of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) ----------------------------------
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int n = n0 + 32 * cb + c31;
        if (n >= p.N) continue;
        const float bv = p.bias ? DType<T>::to_f32(((const T*)p.bias)[n]) : 0.f;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + 64 * wr + 32 * rb + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < p.M) ((T*)p.out)[(size_t)m * p.N + n] = DType<T>::from_f32(fmaf(p.sx[m], master[rb][cb][r], bv));
            }
    }
}

// <T, GM> behind one launch-uniform switch: ONE code object (the library is at its kernel budget); every body is its own straight-line loop
A8_NO_PACKED_F32 __global__ void __launch_bounds__(256) gemm_a8_kernel(A8Params p) {
    __shared__ __attribute__((aligned(16))) char xs[2 * 128 * 128];
    if (p.dtype == GPTQ_F16) {
        if (p.gm == 0) gemm_a8_body<f16, 0>(p, xs);
        else if (p.gm == 1) gemm_a8_body<f16, 1>(p, xs);
        else gemm_a8_body<f16, 2>(p, xs);
    } else {
        if (p.gm == 0) gemm_a8_body<bf16, 0>(p, xs);
        else if (p.gm == 1) gemm_a8_body<bf16, 1>(p, xs);
        else gemm_a8_body<bf16, 2>(p, xs);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------
A8Plan plan_a8(const gptq_layer_t& L, int M) {
    A8Plan pl{};
    auto no = [&](const char* why) { pl.why = why; return pl; };
    if (L.bits != 4) return no("the int8-activation path takes 4-bit layers");
    if (L.dtype != GPTQ_F16 && L.dtype != GPTQ_BF16) return no("the int8-activation path takes fp16 / bf16 layers");
    if (!L.qweight_tiled || !L.qconst_tiled || GPTQ_COPY_COLS(L.tiled_cols) != GPTQ_STRIP_COLS) return no("the int8-activation path reads the decode copy (qweight_tiled / qconst_tiled), this layer has none");
    if (L.g_idx && !L.perm) return no("an act-order layer needs perm (and a decode copy of its re-sequenced rows) on the int8-activation path");
    if (L.epilogue != GPTQ_EPI_NONE) return no("the int8-activation path has no fused epilogue");
    if (M <= 0 || L.K <= 0 || L.K % 32 || L.K > 32736 || L.N <= 0 || L.N % GPTQ_STRIP_COLS)      // (a row of x is staged in the default 64 KiB of LDS)
        return no("the int8-activation path needs M > 0, K a multiple of 32 up to 32736 and N a multiple of 16");
    const int gs = L.group_size;
    if (gs == 32) pl.gm = 2;
    else if (gs == 64) pl.gm = 1;
    else if (gs >= L.K) pl.gshift = 31;
    else if (gs > 0 && gs % 128 == 0 && ((gs / 128) & (gs / 128 - 1)) == 0) {
        while ((128 << pl.gshift) < gs) ++pl.gshift;
    } else return no("the int8-activation path takes group sizes 32, 64, 128 times a power of two, or one group");
    pl.groups = gs >= L.K ? 1 : (L.K + gs - 1) / gs;
    pl.chunks = (L.K + 127) / 128;
    pl.Kp = pl.chunks * 128;
    pl.off_xq = ((size_t)M * 4 + 255) / 256 * 256;
    pl.bytes = pl.off_xq + ((size_t)M * pl.Kp + 255) / 256 * 256;
    pl.npm = (M + 127) / 128;
    pl.npn = (L.N + 127) / 128;
    pl.ok = true;
    return pl;
}

hipError_t launch_act_quant(const gptq_layer_t& L, const A8Plan& pl, const void* x, int M, void* ws, hipStream_t st) {
    float* sx = (float*)ws;
    signed char* xq = (signed char*)ws + pl.off_xq;
    const dim3 grid(M < 4096 ? M : 4096), block(256);
    hipLaunchKernelGGL(act_quant_kernel, grid, block, (size_t)L.K * 2, st, x, L.perm, M, L.K, pl.Kp, pl.gm == 2 ? 1 : 0, (int)L.dtype, sx, xq);
    return hipGetLastError();
}

hipError_t launch_gemm_a8(const gptq_layer_t& L, const A8Plan& pl, const void* ws, void* out, int M, hipStream_t st) {
    A8Params p;
    p.qw = (const char*)L.qweight_tiled;
    p.qc = (const char*)L.qconst_tiled;
    p.bias = L.bias;
    p.out = out;
    p.xq = (const signed char*)ws + pl.off_xq;
    p.sx = (const float*)ws;
    p.M = M, p.N = L.N, p.Kp = pl.Kp, p.chunks = pl.chunks, p.groups = pl.groups, p.gshift = pl.gshift, p.strips = L.N / GPTQ_STRIP_COLS, p.npm = pl.npm;
    p.dtype = L.dtype, p.gm = pl.gm;
    hipLaunchKernelGGL(gemm_a8_kernel, dim3(pl.npm * pl.npn), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace gptq
