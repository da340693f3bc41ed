// gemv_shared.cuh -- device helpers shared by the decode kernels of gemv.hip and gemv_tiled.hip (moved here verbatim from gemv.hip).
#pragma once
#include <type_traits>

#include "common.cuh"
#include "launch.h"

namespace gptq {

// kernel arguments of the checkpoint-layout GEMVs (gemv.hip, gemv_generic.hip)
struct GemvParams {
    const unsigned* qweight;
    const unsigned* qzeros;
    const void* scales;
    const int* g_idx;   // per-k groups (PERK mode) or nullptr
    const int* perm;    // x gather for re-sequenced act-order layers, or nullptr
    const void* bias;
    const void* x;
    void* out;
    float* partial;     // [ksplit][M][N] when ksplit > 1
    int M, K, N, group_size, zero_mode;
    int units_total, units_per_split, chunk_units, ksplit;
    int gu_shift;       // log2(group_size / 8) or -1 (matrix-core 4-bit kernel)
    int pair_off;       // gated epilogue: column distance between the gate and the up half (N / 2), else 0
    int act;            // ... and its gptq_epilogue_t (gated_act)
};
// gemv_generic.hip: fp32-math GEMV for any bits / dtype / group structure (fp32 layers, raw act-order g_idx, odd group sizes)
hipError_t launch_gemv_generic(const gptq_layer_t& L, const GemvPlan& pl, const GemvParams& p, hipStream_t st);

// Sum over the 64/LN row slots of a wave (lanes l, l+LN, l+2LN, ...): DPP rotates inside a 16-lane row,
// ds_bpermute across rows.  Every lane ends up with the total.
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
    const int r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false);
    return v + __builtin_bit_cast(float, r);
}
template <int LN> __device__ __forceinline__ float row_slot_sum(float v) {
    if constexpr (LN <= 4) v = dpp_add<0x124>(v);     // row_ror:4
    if constexpr (LN <= 8) v = dpp_add<0x128>(v);     // row_ror:8
    if constexpr (LN <= 16) v += __shfl_xor(v, 16, 64);
    if constexpr (LN <= 32) v += __shfl_xor(v, 32, 64);
    return v;
}

// The same two last steps for the tail of a kernel whose lanes 0..15 alone go on (gemv_tiled_kernel): (v + v[l ^ 16]) + (the same of l ^ 32), the association of
// the two shuffles, through the gfx950 row / half swaps -- register to register, where __shfl_xor is a ds_bpermute_b32: an LDS round trip behind index arithmetic.
__device__ __forceinline__ float kslot_sum_swap(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);         // [0]: rows 0 0 2 2 of v, [1]: rows 1 1 3 3
    const unsigned a0 = a[0], a1 = a[1];                                          // (scalars first: __builtin_bit_cast applied to a[1] itself reads element 0 -- hipcc of ROCm 7.2)
    const unsigned s = as_u32(as_f32(a0) + as_f32(a1));
    const auto b = __builtin_amdgcn_permlane32_swap(s, s, false, false);         // [0]: the low half of s twice, [1]: the high half twice
    const unsigned b0 = b[0], b1 = b[1];
    return as_f32(b0) + as_f32(b1);
}
// Cross-wave sums of one entry of the LDS slabs (r[w * STRIDE] = the partial of wave w), the wave count known where the code is generated: every read is issued
// before the first add -- ONE LDS round trip, no run-time loop.  tree_sum: the xor tree of stream_finish -- (0,1) (2,3) .., then pairs of pairs; seq_sum: waves in
// ascending order from 0.f (the multi-strip and pair forms).  Same pairs in the same order as the run-time loops they replace: the same bits.
template <int WN, int STRIDE> __device__ __forceinline__ float tree_sum(const float* r) {
    float a[WN];
#pragma unroll
    for (int w = 0; w < WN; ++w) a[w] = r[w * STRIDE];
#pragma unroll
    for (int off = 1; off < WN; off <<= 1)
#pragma unroll
        for (int i = 0; i < WN; i += 2 * off) a[i] += a[i + off];
    return a[0];
}
template <int WN, int STRIDE> __device__ __forceinline__ float seq_sum(const float* r) {
    float a[WN];
#pragma unroll
    for (int w = 0; w < WN; ++w) a[w] = r[w * STRIDE];
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < WN; ++w) t += a[w];
    return t;
}

// 4x4x4 matrix-core step on packed 2-byte operands (u32x2 = 4 values) for both fp16 and bf16
template <typename T> struct Mma4;
template <> struct Mma4<f16> {
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ f32x4 run(u32x2 a, u32x2 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_4x4x4f16(__builtin_bit_cast(v4, a), __builtin_bit_cast(v4, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ unsigned short bits_of_int(int d) { return as_u16((f16)(short)d); }
};
template <> struct Mma4<bf16> {
    typedef short v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ f32x4 run(u32x2 a, u32x2 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(__builtin_bit_cast(v4, a), __builtin_bit_cast(v4, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ unsigned short bits_of_int(int d) { return (unsigned short)(as_u32((float)d) >> 16); }  // exact
};

// The 16-byte LDS DMA of common.cuh (lds_dma16 / lds_dma16_nt: why it is issued from asm) from a 64-bit SCALAR base plus a 32-bit lane offset
// (global_load_lds with saddr), for a burst whose lanes keep one offset register.  Unlike those two, and unlike gemm_mid's dma16_sv_keep_m0, M0 is set
// per DMA and NOT saved -- nothing else in these kernels reads it (gfx9 LDS instructions do not; the compiler emits no other M0 user here), and the save /
// restore pair was two of five instructions.  sbase must come from scalar arithmetic on kernel arguments (no VALU-written SGPR: the VMEM read of it would
// need wait states the compiler cannot see inside the string); s_nop 0: the M0 write -> LDS-DMA hazard.
template <bool NT> __device__ __forceinline__ void dma16_sv_drop_m0(__attribute__((address_space(1))) const char* sbase, unsigned voff, unsigned lds_dst) {
    if constexpr (NT) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 nt" : : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
    else asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
// Stage ROWS rows of `pieces` 16-byte pieces, global -> LDS, by all waves of a workgroup: piece i of row r goes from base[r] + 16 i to LDS byte lds[r] + 16 i.
// Round t moves pieces [t step, (t + 1) step) (step = threads of the workgroup), thread tid its piece tid + t step: the lane offset 16 (tid + t step) is the
// DMAs' only vector operand, the row's base stays scalar.  Straight-line for what the planner's geometries produce -- a wave with no piece skips everything
// on ONE scalar compare (w64 = 64 * wave), one round, two rounds -- and a loop from the third round on (long K).  Only a ragged last wave runs with lanes
// masked off.
template <int ROWS, bool NT>
__device__ __forceinline__ void stage_rows(__attribute__((address_space(1))) const char* const (&base)[ROWS], const unsigned (&lds)[ROWS], int tid, int w64, int step, int pieces) {
    if (w64 >= pieces) return;
    if (tid < pieces) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) dma16_sv_drop_m0<NT>(base[r], (unsigned)tid * 16u, lds[r] + (unsigned)w64 * 16u);
    }
    if (w64 + step >= pieces) return;
    if (tid + step < pieces) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) dma16_sv_drop_m0<NT>(base[r], (unsigned)(tid + step) * 16u, lds[r] + (unsigned)(w64 + step) * 16u);
    }
    if (__builtin_expect(w64 + 2 * step >= pieces, 1)) return;
    for (int a = 2 * step; w64 + a < pieces; a += step) {                         // wave-uniform trip count
        if (tid + a < pieces) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) dma16_sv_drop_m0<NT>(base[r], (unsigned)(tid + a) * 16u, lds[r] + (unsigned)(w64 + a) * 16u);
        }
    }
}
// (a >= b) as 1 / 0 on the scalar unit: written in C++, a wave-uniform compare with several users becomes a lane mask and a v_cndmask_b32
__device__ __forceinline__ int scalar_ge(int a, int b) {
    int r;
    asm("s_cmp_ge_i32 %1, %2\n\ts_cselect_b32 %0, 1, 0" : "=s"(r) : "s"(a), "s"(b) : "scc");
    return r;
}

// (c != 0 ? a : b) on the scalar unit, for the reason scalar_ge gives
__device__ __forceinline__ int scalar_sel_nz(unsigned c, int a, int b) {
    int r;
    asm("s_cmp_lg_u32 %1, 0\n\ts_cselect_b32 %0, %2, %3" : "=s"(r) : "s"(c), "s"(a), "s"(b) : "scc");
    return r;
}

struct GemvSeg {
    const unsigned* qweight;
    const unsigned* qzeros;
    const void* scales;
    const void* bias;
    void* out;
    int N;         // columns of this layer
    int blk_end;   // cumulative strip count up to and including this layer
    int col0;      // first column of this layer in the concatenated partial slab
    int pad_;
};
struct GemvStreamParams {
    GemvSeg seg[4];
    const void* x;
    unsigned long long* gran;   // [ksplit - 1][M][nsum] exchange granules {fp32 partial sum, tag} of K slices 1 .. ksplit - 1
    unsigned* epochs;           // [strips_total] per-strip launch epoch (header bytes 32768 ..): bumped by the strip's owner slice, never reset
    unsigned* err;              // sticky error word (header tail): a bounded wait gave up
    int nseg, M, K, zero_mode, units_total, units_per_split, ksplit, gu_shift, nsum;
    unsigned max_spins;
};

// Shared tail of the streamed GEMV kernels: row slots (DPP / bpermute), waves (LDS, the kernel's only barrier), then write -- or, with a K split,
// publish / combine through {fp32, tag} granules.
// (stage: optional LDS copy of the finished [MT][CT] outputs of the strip; sg.out may then be null.)
// Second half of the streamed kernels' tail: the per-wave partial sums of the workgroup's CT columns x MT rows are in LDS (red[wave * (MT * CT + 4) + m * CT + c],
// behind a barrier); cross-wave sum, then write -- or, with a K split, publish / combine through {fp32, tag} granules.
template <int CT, int MT, typename T, typename PP = GemvStreamParams, typename SG = GemvSeg>
__device__ __forceinline__ void stream_finish(const PP& p, const SG& sg, int strip, int sidx, int ks, int N, const float* red, T* stage = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = blockDim.x >> 6;
    constexpr int E = MT * CT, ES = E + 4;                                    // slab stride padded by 16 B: the W partials of an entry spread over banks
    // K split: slice ks >= 1 PUBLISHES its partial sums as 8-byte {fp32, tag} granules (one write-through store each) and is done; slice 0,
    // the strip's OWNER, polls the granules of the other slices for its entries, takes each the moment its tag is this launch's, adds them in
    // slice order (fixed order: bit-reproducible) and writes the result -- ONE memory hop after the last slice has published, where the
    // ticket scheme this replaces (publish, drain, draw a ticket, last arriver reads everything back) was three (~3 us).
    // tag = the strip's epoch word + 1 in a NaN pattern; the owner bumps the word when all its waves are through (by then every producer
    // wave has read it), so the next launch on this workspace -- any layer -- uses a tag that no stale granule carries.
    unsigned tag = 0;
    if (p.ksplit > 1) {
        unsigned ep;
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ep) : "s"(p.epochs + sidx) : "memory");
        tag = 0x7FE00000u | ((ep + 1u) & 0x1FFFFFu);
    }
    const size_t slab = (size_t)p.M * p.nsum;
    bool gave_up = false;
    auto emit = [&](int e, float t) {
        const int m = e / CT, c = e % CT;
        const int n = strip * CT + c;
        if (n >= N || m >= p.M) return;
        if (p.ksplit > 1) {
            const size_t at = (size_t)m * p.nsum + sg.col0 + n;
            if (ks != 0) {
                const unsigned long long g8 = (unsigned long long)as_u32(t) | ((unsigned long long)tag << 32);
                __hip_atomic_store(p.gran + (size_t)(ks - 1) * slab + at, g8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            constexpr int KMAX = 8;                                           // planner: ksplit <= 8
            unsigned long long v[KMAX - 1];
            unsigned pending = (1u << (p.ksplit - 1)) - 1u;
            for (unsigned spins = 0; pending; ++spins) {
#pragma unroll
                for (int k = 0; k < KMAX - 1; ++k)
                    if (pending & (1u << k)) v[k] = __hip_atomic_load(p.gran + (size_t)k * slab + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int k = 0; k < KMAX - 1; ++k)
                    if ((pending & (1u << k)) && (unsigned)(v[k] >> 32) == tag) pending &= ~(1u << k);
                if (pending && spins > p.max_spins) { gave_up = true; break; }
                if (pending) __builtin_amdgcn_s_sleep(2);
            }
#pragma unroll
            for (int k = 0; k < KMAX - 1; ++k)
                if (k < p.ksplit - 1) t += as_f32((unsigned)(v[k] & 0xffffffffu));
            // consumed granules are cleared: between launches the exchange area holds NO valid tag, so a tag that is valid now was written by
            // this launch -- per-strip epochs alone would let a strip whose epoch lags (it is used by fewer layers of the model) accept what
            // another layer published at the same address under the same number
#pragma unroll
            for (int k = 0; k < KMAX - 1; ++k)
                if (k < p.ksplit - 1) __hip_atomic_store(p.gran + (size_t)k * slab + at, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (sg.bias) t += DType<T>::to_f32(((const T*)sg.bias)[n]);
        const T o = DType<T>::from_f32(t);
        if (sg.out) ((T*)sg.out)[(size_t)m * N + n] = o;
        if (stage) stage[m * CT + c] = o;                                      // tensor-parallel epilogue (gemv_tiled.hip): the strip's rows, for the peer stores
    };
    if ((W & (W - 1)) == 0) {
        // every wave takes 64 / W entries per round; its lanes are (entry, partial w) pairs: one LDS read each, then a fixed
        // xor tree over the W lanes of an entry (deterministic order) -- instead of one thread walking W slabs per entry
        const int lw = __builtin_ctz((unsigned)W);
        const int w_of_lane = lane & (W - 1), e_of_lane = lane >> lw;
        for (int e0 = 0; e0 < E; e0 += 64) {
            const int e = e0 + wave * (64 >> lw) + e_of_lane;
            float t = (e < E) ? red[w_of_lane * ES + e] : 0.f;
            for (int off = 1; off < W; off <<= 1) t += __shfl_xor(t, off, 64);
            if (w_of_lane == 0 && e < E) emit(e, t);
        }
    } else {
        for (int e = tid; e < E; e += blockDim.x) {
            float t = 0.f;
            for (int w = 0; w < W; ++w) t += red[w * ES + e];
            emit(e, t);
        }
    }
    if (p.ksplit > 1 && ks == 0) {
        if (gave_up) __hip_atomic_store(p.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();                                                      // every wave of the owner has its granules: every producer wave has read the epoch
        if (tid == 0) __hip_atomic_store(p.epochs + sidx, (tag & 0x1FFFFFu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int LN, int MT, typename T>
__device__ __forceinline__ void stream_epilogue(f32x4 (&acc)[MT], const GemvStreamParams& p, const GemvSeg& sg, int strip, int sidx, int ks, int N,
                                                float* red) {
    constexpr int CT = LN * 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = blockDim.x >> 6;
    // ---- row slots (DPP / bpermute), waves (LDS, the only barrier), then write or publish ------------------------------
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[m][c] = row_slot_sum<LN>(acc[m][c]);
    constexpr int E = MT * CT, ES = E + 4;                                    // slab stride padded by 16 B: the W partials of an entry spread over banks
    if (lane < LN) {
#pragma unroll
        for (int m = 0; m < MT; ++m) *(f32x4*)(red + wave * ES + m * CT + lane * 4) = acc[m];
    }
    __syncthreads();
    stream_finish<CT, MT, T>(p, sg, strip, sidx, ks, N, red);
}


}  // namespace gptq
