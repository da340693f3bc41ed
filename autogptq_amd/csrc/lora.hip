// lora.hip -- the LoRA adapter branch beside a quantized linear: out += scale * (x . A^T) . B^T as two launches (gptq_lora_down, gptq_lora_up).
//
// A GPTQ layer cannot merge its adapter (W is int4 on a fixed grid; the reference refuses it: auto_gptq/utils/peft_utils.py:94-98), so every call pays
// the branch at run time.  Nothing here reads packed weights: the base product stays gptq_forward*, these kernels add the rank-r term on top of it.
//   down:  u[m, j]   = T(sum_k x[m, k] * A[j, k])                                      A = lora_A.weight [r, K] as peft stores it
//   up:    out[m, n] = T(float(out[m, n]) + scale * sum_j float(u[m, j]) * float(B[n, j]))   B = lora_B.weight [N, r], in place on the base output
// fp32 products and sums, one rounding each.  Up to 4 adapters that share x go through ONE launch of either kernel (q|k|v, gate|up): the pointer sets
// travel by value in the launch arguments, the grid runs over the concatenated units of all adapters, and a unit's arithmetic depends on nothing but its
// own adapter -- the multi result is bit-identical to single calls.  No atomics, no workgroup waits on another, fixed summation order, no workspace.
//
// Both operands of either product are rows contiguous in the summed index -- the fragments of v_mfma_f32_16x16x32_{f16,bf16} as they lie in memory
// (lane l: row l & 15, k = 8 (l >> 4) + 0..7): 16-byte global loads straight into the matrix core, no LDS staging of operands.
//   down, 9+ rows:  a workgroup is 16 rows of x times one 16-wide block of A rows (r is padded to 16 in registers) times the whole K; its 8 waves
//                   take the 32-wide k-steps round robin and meet once in LDS, summed in wave order.
//   down, 1-8 rows: a workgroup is one row j of A; 512 lanes stride K in 16-byte loads, every lane keeps one fp32 sum per row of x; butterfly across
//                   the wave, then the 8 waves in order through LDS.
//   up, 9+ rows:    B rows are the MFMA's A operand and u rows its B operand, so a lane's four accumulators are four consecutive n of one output
//                   row: an 8-byte read-modify-write.  A wave owns 16 rows x 64 columns, a workgroup 256 columns.  r is zero-padded to 32 / 64 in registers.
//   up, 1-8 rows:   plain VALU: a thread owns one n, reads B[n, :] in 16-byte loads and u (as fp32) from LDS, ascending j.
// The row regime is a launch-uniform branch: one instantiation per kernel and dtype (4 in all).
#include "common.cuh"
#include "mma_dequant.cuh"
#include "launch.h"

namespace gptq {
namespace lora {

constexpr int DOWN_THREADS = 512;           // 8 waves split K
constexpr int DOWN_WAVES = DOWN_THREADS / 64;
constexpr int UP_THREADS = 256;             // 9+ rows: 4 waves x 64 columns
constexpr int UP_GEMV_THREADS = 64;         // 1-8 rows: one n per thread
constexpr int UP_COLS = 256;

struct Set {
    const void* A;
    const void* B;
    void* u;
    void* out;
    int N, r;
    float scale;
    int pad;
};
struct Args {
    Set s[GPTQ_LORA_MAX];
    const void* x;
    int n, M, K, gemv;
};

__host__ __device__ inline int down_units(int r, int gemv) { return gemv ? r : (r + 15) / 16; }
__host__ __device__ inline int up_units(int N, int gemv) { return gemv ? (N + UP_GEMV_THREADS - 1) / UP_GEMV_THREADS : (N + UP_COLS - 1) / UP_COLS; }

// the adapter that owns unit `b` of the concatenated grid, and b relative to it (constant indices only: the sets stay in scalar registers)
template <bool UP>
__device__ __forceinline__ Set locate(const Args& p, int& b) {
    Set s = p.s[0];
    int start = 0;
    const int g = b;
#pragma unroll
    for (int i = 1; i < GPTQ_LORA_MAX; ++i) {
        start += UP ? up_units(p.s[i - 1].N, p.gemv) : down_units(p.s[i - 1].r, p.gemv);
        if (i < p.n && g >= start) {
            s = p.s[i];
            b = g - start;
        }
    }
    return s;
}

template <typename T>
__global__ void __launch_bounds__(DOWN_THREADS) lora_down_kernel(Args p) {
    __shared__ float red[DOWN_WAVES * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K, M = p.M;
    const T* __restrict__ x = (const T*)p.x;
    int b = p.gemv ? blockIdx.x : blockIdx.y;
    const Set s = locate<false>(p, b);
    const T* __restrict__ A = (const T*)s.A;
    T* __restrict__ u = (T*)s.u;

    if (p.gemv) {
        const int j = b;
        const T* a = A + (size_t)j * K;
        float acc[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) acc[m] = 0.f;
        for (int k = tid * 8; k < K; k += DOWN_THREADS * 8) {
            float af[8];
            unpack8<T>(*(const u32x4*)(a + k), af);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                if (m < M) {
                    float xf[8];
                    unpack8<T>(*(const u32x4*)(x + (size_t)m * K + k), xf);
#pragma unroll
                    for (int c = 0; c < 8; ++c) acc[m] = fmaf(xf[c], af[c], acc[m]);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc[m] += __shfl_xor(acc[m], off);
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < 8; ++m) red[wave * 8 + m] = acc[m];
        }
        __syncthreads();
        if (tid < M) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < DOWN_WAVES; ++w) v += red[w * 8 + tid];
            u[(size_t)tid * s.r + j] = DType<T>::from_f32(v);
        }
        return;
    }

    const int m0 = blockIdx.x * 16, j0 = b * 16;
    const int row = lane & 15, kq = lane >> 4;
    const bool xok = m0 + row < M, aok = j0 + row < s.r;
    const char* xp = (const char*)(x + (size_t)(xok ? m0 + row : 0) * K) + kq * 16;
    const char* ap = (const char*)(A + (size_t)(aok ? j0 + row : 0) * K) + kq * 16;
    const u32x4 zero = u32x4{0, 0, 0, 0};
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int steps = K / 32;                                   // 64 bytes of a row per step
    for (int st = wave; st < steps; st += 4 * DOWN_WAVES) {
        u32x4 xa[4], aa[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = st + i * DOWN_WAVES;
            const bool in = t < steps;
            xa[i] = in && xok ? *(const u32x4*)(xp + (size_t)t * 64) : zero;
            aa[i] = in && aok ? *(const u32x4*)(ap + (size_t)t * 64) : zero;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = Mma16<T>::run(xa[i], aa[i], acc);
    }
    // accumulator: column (l & 15) is j, rows 4 (l >> 4) + reg are m
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) red[wave * 256 + (4 * kq + reg) * 16 + row] = acc[reg];
    __syncthreads();
    if (tid < 256) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < DOWN_WAVES; ++w) v += red[w * 256 + tid];
        const int m = m0 + (tid >> 4), j = j0 + (tid & 15);
        if (m < M && j < s.r) u[(size_t)m * s.r + j] = DType<T>::from_f32(v);
    }
}

template <typename T>
__global__ void __launch_bounds__(UP_THREADS) lora_up_kernel(Args p) {
    __shared__ float us[8 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = p.M;
    int b = p.gemv ? blockIdx.x : blockIdx.y;
    const Set s = locate<true>(p, b);
    const int N = s.N, r = s.r;
    const T* __restrict__ B = (const T*)s.B;
    const T* __restrict__ u = (const T*)s.u;
    T* __restrict__ out = (T*)s.out;

    if (p.gemv) {
        for (int i = tid; i < M * r; i += UP_GEMV_THREADS) us[i] = DType<T>::to_f32(u[i]);
        __syncthreads();
        const int n = b * UP_GEMV_THREADS + tid;
        if (n >= N) return;
        float acc[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) acc[m] = 0.f;
        for (int c = 0; c < r; c += 8) {
            float bf[8];
            unpack8<T>(*(const u32x4*)(B + (size_t)n * r + c), bf);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                if (m < M) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[m] = fmaf(us[m * r + c + i], bf[i], acc[m]);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            if (m < M) {
                T* o = out + (size_t)m * N + n;
                *o = DType<T>::from_f32(DType<T>::to_f32(*o) + s.scale * acc[m]);
            }
        }
        return;
    }

    const int m0 = blockIdx.x * 16, n0 = b * UP_COLS + wave * 64;
    if (n0 >= N) return;
    const int row = lane & 15, kq = lane >> 4;
    const bool mok = m0 + row < M;
    const u32x4 zero = u32x4{0, 0, 0, 0};
    const bool two = r > 32;                                    // the second k-step of the matrix core (j = 32..63)
    const int ja = 8 * kq, jb = 32 + 8 * kq;
    const T* up = u + (size_t)(mok ? m0 + row : 0) * r;
    const u32x4 u0 = mok && ja < r ? *(const u32x4*)(up + ja) : zero;
    const u32x4 u1 = mok && jb < r ? *(const u32x4*)(up + jb) : zero;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int nn = n0 + nb * 16;                            // N % 16 == 0: a block is inside or outside as a whole
        const bool nok = nn < N;
        const T* bp = B + (size_t)(nok ? nn + row : 0) * r;
        const u32x4 b0 = nok && ja < r ? *(const u32x4*)(bp + ja) : zero;
        const u32x4 b1 = nok && jb < r ? *(const u32x4*)(bp + jb) : zero;
        f32x4 acc = Mma16<T>::run(b0, u0, f32x4{0.f, 0.f, 0.f, 0.f});
        if (two) acc = Mma16<T>::run(b1, u1, acc);
        // accumulator: column (l & 15) is m, rows 4 (l >> 4) + reg are four consecutive n
        if (nok && mok) {
            T* o = out + (size_t)(m0 + row) * N + nn + 4 * kq;
            const u32x2 old = *(const u32x2*)o;
            const unsigned ow[2] = {old.x, old.y};
            unsigned short h[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float prev = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(ow[c >> 1] >> (16 * (c & 1)))));
                h[c] = __builtin_bit_cast(unsigned short, DType<T>::from_f32(prev + s.scale * acc[c]));
            }
            *(u32x2*)o = u32x2{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
        }
    }
}

static Args make_args(const gptq_lora_t* const* Ls, int n, const void* x, void* const* u, void* const* outs, int M) {
    Args p;
    for (int i = 0; i < GPTQ_LORA_MAX; ++i) {
        Set& s = p.s[i];
        if (i < n) {
            s.A = Ls[i]->A;
            s.B = Ls[i]->B;
            s.u = u[i];
            s.out = outs ? outs[i] : nullptr;
            s.N = Ls[i]->N;
            s.r = Ls[i]->r;
            s.scale = Ls[i]->scale;
        } else {
            s.A = s.B = nullptr;
            s.u = s.out = nullptr;
            s.N = s.r = 0;
            s.scale = 0.f;
        }
        s.pad = 0;
    }
    p.x = x;
    p.n = n;
    p.M = M;
    p.K = Ls[0]->K;
    p.gemv = M <= GPTQ_LORA_GEMV_ROWS ? 1 : 0;
    return p;
}

}  // namespace lora

LoraPlan plan_lora(const gptq_lora_t* const* Ls, int n, int M) {
    LoraPlan pl;
    pl.gemv = M <= GPTQ_LORA_GEMV_ROWS;
    long du = 0, uu = 0;
    for (int i = 0; i < n; ++i) {
        du += lora::down_units(Ls[i]->r, pl.gemv);
        uu += lora::up_units(Ls[i]->N, pl.gemv);
    }
    pl.mtiles = pl.gemv ? 1 : ((long)M + 15) / 16;
    pl.units_down = du;
    pl.units_up = uu;
    pl.wg_down = du * pl.mtiles;
    pl.wg_up = uu * pl.mtiles;
    return pl;
}

hipError_t launch_lora_down(const gptq_lora_t* const* Ls, int n, const void* x, void* const* u, int M, hipStream_t st) {
    const LoraPlan pl = plan_lora(Ls, n, M);
    if (pl.mtiles > 0x7fffffffL || pl.units_down > 65535) return hipErrorInvalidValue;
    const lora::Args p = lora::make_args(Ls, n, x, u, nullptr, M);
    const dim3 grid = pl.gemv ? dim3((unsigned)pl.units_down) : dim3((unsigned)pl.mtiles, (unsigned)pl.units_down);
    const dim3 block(lora::DOWN_THREADS);
    if (Ls[0]->dtype == GPTQ_F16) hipLaunchKernelGGL(lora::lora_down_kernel<f16>, grid, block, 0, st, p);
    else if (Ls[0]->dtype == GPTQ_BF16) hipLaunchKernelGGL(lora::lora_down_kernel<bf16>, grid, block, 0, st, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_lora_up(const gptq_lora_t* const* Ls, int n, const void* const* u, void* const* outs, int M, hipStream_t st) {
    const LoraPlan pl = plan_lora(Ls, n, M);
    if (pl.gemv ? pl.units_up > 0x7fffffffL : (pl.mtiles > 0x7fffffffL || pl.units_up > 65535)) return hipErrorInvalidValue;
    const lora::Args p = lora::make_args(Ls, n, nullptr, (void* const*)u, outs, M);
    const dim3 grid = pl.gemv ? dim3((unsigned)pl.units_up) : dim3((unsigned)pl.mtiles, (unsigned)pl.units_up);
    const dim3 block(pl.gemv ? lora::UP_GEMV_THREADS : lora::UP_THREADS);
    if (Ls[0]->dtype == GPTQ_F16) hipLaunchKernelGGL(lora::lora_up_kernel<f16>, grid, block, 0, st, p);
    else if (Ls[0]->dtype == GPTQ_BF16) hipLaunchKernelGGL(lora::lora_up_kernel<bf16>, grid, block, 0, st, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace gptq
