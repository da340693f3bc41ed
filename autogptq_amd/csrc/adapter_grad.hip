// adapter_grad.hip -- the LoRA adapters' weight gradients (steps 2 and 3 of gptq_lora_backward):
//   dA[j, k] = s * sum_m du[m, j] * x[m, k]     fp32 [r, K]
//   dB[n, j] = s * sum_m dY[m, n] * u[m, j]     fp32 [N, r]
// Both are one transposed tall-skinny product out = s * big^T . small (or its transpose) with big [M][L] (L = K or N) and small [M][r]: the summed
// index is the ROW index of both operands -- the opposite of lora.hip, whose operands lie in memory as the matrix core wants them.  Here they do not:
// 32-row tiles of both operands are staged row-major in LDS (16-byte coalesced loads, rows past M zero-filled) and both MFMA operands are fetched with
// ds_read_b64_tr_b16, the transposing LDS read: a 16-lane group reads a block of 4 rows x 16 columns and each lane receives one column.
//   unit:   one 64-wide block of L  x  all of r (padded to 64 in LDS, zero-filled)  x  one slice of M.  256 threads; wave w owns columns 16 w .. 16 w + 15
//           of the block and four 16-wide blocks of r: 4 accumulators, 2 + 8 transposed reads and 4 v_mfma_f32_16x16x32 per 32-row step.  The waves
//           share nothing but the staged tile, so there is no meeting: an output element is ONE accumulator chain over the slice's steps.
//   k map:  slot 8 g + e of the matrix core's 32-long k (g = lane / 16) is tile row 4 g + e (e < 4) or 16 + 4 g + e - 4: the same for both operands, so
//           the sum runs over all 32 rows; a 32-lane half then reads 8 consecutive rows, which an LDS row of 160 bytes spreads over all 64 banks.
//   EXEC:   every lane of every wave issues every transposed read with an in-bounds address (the tile is padded, not masked); no early return.
//   slices: S = wgrad_slices(M, P, Q), a function of the shapes alone.  S = 1: out = s * acc.  S > 1: fp32 partials [S][P][Q] in the workspace, then
//           wgrad_sum_kernel adds them in ascending slice order and applies s.  No atomics, fixed orders.
// ONE launch covers the dA and dB units of all adapters of a call (the jobs travel by value; constant indices only, so they stay in scalar registers).
#include "common.cuh"
#include "mma_dequant.cuh"
#include "launch.h"

namespace gptq {
namespace adapters {

constexpr int THREADS = 256;
constexpr int ROWS = 32;                    // rows of one step: the k of v_mfma_f32_16x16x32
constexpr int COLS = 64;                    // the block of the large dimension; r is padded to the same width
constexpr int STRIDE = 80;                  // 16-bit elements of an LDS row: 160 bytes, rows 0..7 start on banks 0, 40, 16, 56, 32, 8, 48, 24
constexpr int SUM_THREADS = 256;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

struct Job {
    const void* big;                        // [M][L]: x (dA) or dY (dB)
    const void* small;                      // [M][r]: du (dA) or u (dB)
    float* out;                             // [r][K] or [N][r]
    float* part;                            // [S][P][Q] partials (S > 1)
    int L, r;
    int sL, sJ;                             // output strides of the large index and of j
    int S, sps;                             // slices; steps of a slice
    float scale;
    int units, sum_units;                   // workgroups of this job in either kernel
    int pad;
};
struct Args {
    Job j[GPTQ_WGRAD_JOBS];
    int n, M;
};

template <bool SUM>
__device__ __forceinline__ Job locate(const Args& p, int& b) {
    Job j = p.j[0];
    int start = 0;
    const int g = b;
#pragma unroll
    for (int i = 1; i < GPTQ_WGRAD_JOBS; ++i) {
        start += SUM ? p.j[i - 1].sum_units : p.j[i - 1].units;
        if (i < p.n && g >= start) {
            j = p.j[i];
            b = g - start;
        }
    }
    return j;
}

// the operand of one 16-wide block: rows 4 g .. 4 g + 3 and 16 + 4 g .. 16 + 4 g + 3 of its columns, transposed
__device__ __forceinline__ u32x4 tr_operand(const unsigned short* at) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)at);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(at + 16 * STRIDE));
    const u32x2 l = __builtin_bit_cast(u32x2, lo), h = __builtin_bit_cast(u32x2, hi);
    return u32x4{l.x, l.y, h.x, h.y};
}

template <typename T>
__global__ void __launch_bounds__(THREADS) wgrad_kernel(Args p) {
    __shared__ __attribute__((aligned(16))) unsigned short big_s[2][ROWS * STRIDE];
    __shared__ __attribute__((aligned(16))) unsigned short small_s[2][ROWS * STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    const Job j = locate<false>(p, b);
    const int blk = b / j.S, slice = b - blk * j.S;
    const int L = j.L, r = j.r, L0 = blk * COLS;
    const long row0 = (long)slice * j.sps * ROWS;
    const long row1 = min((long)p.M, row0 + (long)j.sps * ROWS);
    const int steps = (int)((row1 - row0 + ROWS - 1) / ROWS);

    // staging: thread t carries 16 bytes of row t / 8 of either tile
    const int srow = tid >> 3, ch = tid & 7;
    const bool bok = L0 + ch * 8 < L, sok = ch * 8 < r;           // L % 8 == 0 and r % 8 == 0: a chunk is inside or outside as a whole
    const T* bp = (const T*)j.big + (bok ? L0 + ch * 8 : 0);
    const T* sp = (const T*)j.small + (sok ? ch * 8 : 0);
    const int soff = srow * STRIDE + ch * 8;
    const u32x4 zero = u32x4{0, 0, 0, 0};

    // transposed reads: lane 4 q + pp of group g gives the address of row 4 g + q, columns 4 pp .. 4 pp + 3 of the block
    const int g = lane >> 4, i = lane & 15;
    const int toff = (4 * g + (i >> 2)) * STRIDE + 4 * (i & 3);

    f32x4 acc[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) acc[jb] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 bv = zero, sv = zero;
    {
        const long m = row0 + srow;
        if (m < row1) {
            if (bok) bv = *(const u32x4*)(bp + (size_t)m * L);
            if (sok) sv = *(const u32x4*)(sp + (size_t)m * r);
        }
    }
    for (int st = 0; st < steps; ++st) {
        unsigned short* bs = big_s[st & 1];
        unsigned short* ss = small_s[st & 1];
        *(u32x4*)(bs + soff) = bv;
        *(u32x4*)(ss + soff) = sv;
        __syncthreads();                                            // two buffers: the next write to this one is behind the next step's barrier
        bv = zero;
        sv = zero;
        const long m = row0 + (long)(st + 1) * ROWS + srow;
        if (m < row1) {
            if (bok) bv = *(const u32x4*)(bp + (size_t)m * L);
            if (sok) sv = *(const u32x4*)(sp + (size_t)m * r);
        }
        const u32x4 a = tr_operand(bs + toff + 16 * wave);
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) acc[jb] = Mma16<T>::run(a, tr_operand(ss + toff + 16 * jb), acc[jb]);
    }

    // accumulator: column (lane & 15) is j within the block, rows 4 (lane >> 4) + reg are four consecutive indices of the large dimension
    const bool direct = j.S == 1;
    float* dst = direct ? j.out : j.part + (size_t)slice * L * r;
    const float f = direct ? j.scale : 1.f;
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
        const int jj = 16 * jb + i;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int l = L0 + 16 * wave + 4 * g + reg;
            if (l < L && jj < r) dst[(size_t)l * j.sL + (size_t)jj * j.sJ] = f * acc[jb][reg];
        }
    }
}

__global__ void __launch_bounds__(SUM_THREADS) wgrad_sum_kernel(Args p) {
    int b = blockIdx.x;
    const Job j = locate<true>(p, b);
    const size_t pq = (size_t)j.L * j.r, e = (size_t)b * SUM_THREADS + threadIdx.x;
    if (e >= pq) return;
    float v = 0.f;
    for (int s = 0; s < j.S; ++s) v += j.part[(size_t)s * pq + e];
    j.out[e] = j.scale * v;
}

}  // namespace adapters

WgradSlices wgrad_slices(int M, int P, int Q) {
    WgradSlices s{1, 0};
    if (M <= 0) return s;
    const long steps = ((long)M + adapters::ROWS - 1) / adapters::ROWS;
    const long blocks = ((long)(P > Q ? P : Q) + adapters::COLS - 1) / adapters::COLS;
    long s0 = steps / 4 > 1 ? steps / 4 : 1;
    const long fill = (512 + blocks - 1) / blocks;
    if (s0 > fill) s0 = fill;
    if (s0 > 64) s0 = 64;
    const long sps = (steps + s0 - 1) / s0;
    s.steps_per_slice = (int)sps;
    s.S = (int)((steps + sps - 1) / sps);
    return s;
}

WgradPlan plan_wgrad(const gptq_lora_t* const* Ls, const gptq_lora_grad_t* const* Gs, int n, int M) {
    WgradPlan pl{};
    for (int i = 0; i < n; ++i) {
        const gptq_lora_t& L = *Ls[i];
        for (int w = 0; w < 2; ++w) {
            const int big = w ? L.N : L.K;
            const WgradSlices s = wgrad_slices(M, w ? L.N : L.r, w ? L.r : L.K);
            const size_t pq = (size_t)big * L.r;
            pl.off[2 * i + w] = pl.bytes;
            if (s.S > 1) pl.bytes += align256(4 * (size_t)s.S * pq);
            const bool asked = !Gs || (w ? Gs[i]->dB : Gs[i]->dA) != nullptr;
            if (!asked || M <= 0) continue;
            pl.sl[2 * i + w] = s;
            pl.jobs += 1;
            pl.wg_wgrad += (long)((big + adapters::COLS - 1) / adapters::COLS) * s.S;
            if (s.S > 1) pl.wg_sum += (long)((pq + adapters::SUM_THREADS - 1) / adapters::SUM_THREADS);
        }
    }
    return pl;
}

hipError_t launch_wgrad(const gptq_lora_t* const* Ls, const gptq_lora_grad_t* const* Gs, int n, const void* x, int M, const WgradPlan& pl, char* ws,
                        hipStream_t st) {
    if (pl.jobs == 0) return hipSuccess;
    if (pl.wg_wgrad > 0x7fffffffL || pl.wg_sum > 0x7fffffffL) return hipErrorInvalidValue;
    adapters::Args p{};
    int k = 0;
    for (int i = 0; i < n; ++i) {
        const gptq_lora_t& L = *Ls[i];
        const gptq_lora_grad_t& G = *Gs[i];
        for (int w = 0; w < 2; ++w) {
            const WgradSlices s = pl.sl[2 * i + w];
            if (s.S == 0) continue;
            adapters::Job& j = p.j[k++];
            j.big = w ? G.dY : x;
            j.small = w ? G.u : (const void*)G.du;
            j.out = w ? G.dB : G.dA;
            j.part = s.S > 1 ? (float*)(ws + pl.off[2 * i + w]) : nullptr;
            j.L = w ? L.N : L.K;
            j.r = L.r;
            j.sL = w ? L.r : 1;
            j.sJ = w ? 1 : L.K;
            j.S = s.S;
            j.sps = s.steps_per_slice;
            j.scale = L.scale;
            j.units = (j.L + adapters::COLS - 1) / adapters::COLS * s.S;
            j.sum_units = s.S > 1 ? (int)(((size_t)j.L * j.r + adapters::SUM_THREADS - 1) / adapters::SUM_THREADS) : 0;
        }
    }
    p.n = k;
    p.M = M;
    if (Ls[0]->dtype == GPTQ_F16) hipLaunchKernelGGL(adapters::wgrad_kernel<f16>, dim3((unsigned)pl.wg_wgrad), dim3(adapters::THREADS), 0, st, p);
    else if (Ls[0]->dtype == GPTQ_BF16) hipLaunchKernelGGL(adapters::wgrad_kernel<bf16>, dim3((unsigned)pl.wg_wgrad), dim3(adapters::THREADS), 0, st, p);
    else return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || pl.wg_sum == 0) return e;
    hipLaunchKernelGGL(adapters::wgrad_sum_kernel, dim3((unsigned)pl.wg_sum), dim3(adapters::SUM_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace gptq
