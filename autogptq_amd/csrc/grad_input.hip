// grad_input.hip -- the input gradient of the quantized linear on the packed weights: dX[M, K] (+)= dY[M, N] . W^T (gptq_grad_input).
//
// W = gptq_dequant(layer) exactly: every weight is T(s * float(q - z)) -- the fp32 product is exact, one rounding to the layer dtype -- as dequant_kernel
// (utils.hip) writes it and the reference's PyTorch route computes it (auto_gptq/nn_modules/qlinear/qlinear_cuda_old.py:295-349).  Products and sums in
// fp32 on the matrix core, one rounding at the store.  The reference's triton backend runs the same product as a transposed dequant-matmul
// (auto_gptq/nn_modules/triton_utils/kernels.py:408-426); its cuda backends materialise W in HBM per call.  Nothing is copied from either.
//
// The reduction runs over N (the layer's outputs), so the output columns are the layer's k and the packing -- 32/bits consecutive k of one column per
// word -- runs along the OUTPUT axis: the kernel transposes while it dequantises.  A workgroup owns BM rows x 128 k of dX and walks N in stages of
// 128 bytes per row (64 n of a 16-bit layer, 32 n of an fp32 one):
//   * dY [BM][stage] is copied to LDS as it is (16-byte loads);
//   * each thread takes 8 consecutive k x 4 consecutive n of the packed rows (one 16-byte load of 4 words, two when 8 k straddle a word: 3 / 8 bits),
//     dequantises them and writes an LDS image laid out [k][n] (n contiguous, 8-byte writes; 16 for fp32);
//   * both images are read with ds_read_b128: lane l takes row l & 15 and the 16-byte slot 4 s + (l >> 4) of k-step s, i.e. 8 consecutive n (4 for
//     fp32) at one row -- the A / B fragments of v_mfma_f32_16x16x32_{f16,bf16} as they are; the fp32 kernel feeds the 4 floats of a slot to four
//     v_mfma_f32_16x16x4_f32 (n = 16 s + 4 (l >> 4) + j on both operands, so the products pair up);
//   * slot s of row r sits at slot s ^ ((r >> 1) & 7): 16 consecutive rows read at one slot land on 16 distinct bank groups.
// Two LDS buffers (one barrier per stage): the next stage's raw words (weights, dY, scale / zero words or g_idx) are loaded into registers before the
// matrix-core work of this one and written to the other buffer behind it.  Group constants: a word's 8 k share one group when g_idx is absent and
// group_size % 8 == 0 (loaded with the stage); otherwise every k looks its group up (g_idx, or k / group_size) -- act-order layers read the checkpoint
// rows in their own order, there is no scattered output and no workspace.
// Epilogue: the fp32 accumulators go through LDS (the same 64 KiB) to rows of 8 consecutive k: 16-byte stores, + dX in fp32 first when accumulating.
// bits, the group mode and the tile height are runtime-uniform: one kernel per dtype (3 instantiations).
#include "common.cuh"
#include "mma_dequant.cuh"
#include "launch.h"

namespace gptq {
namespace gin {

constexpr int THREADS = 256;                // 4 waves: 2 (rows) x 2 (k halves of 64)
constexpr int BK = 128;                     // k (output columns) per workgroup
constexpr int ROW_BYTES = 128;              // one LDS image row per stage: 8 slots of 16 bytes (the row swz() of mma_dequant.cuh lays out)
constexpr int LDS_BYTES = 65536;            // 2 x (BM + BK) x 128 (BM = 128) = the fp32 epilogue tile [128][128]

struct Args {
    const unsigned* qweight;
    const unsigned* qzeros;
    const void* scales;
    const int* g_idx;
    const void* dy;
    void* dx;
    int M, K, N, bits, group_size, zero_mode, bm, nkt, accumulate;
};

// the raw words one thread loads for a stage (consumed by store() after the matrix-core work of the previous stage)
struct Stage {
    u32x4 a[4];          // dY: 16-byte slots of the A image
    u32x4 q0, q1;        // packed words of 4 columns: the word holding the task's first k, and the next one when the 8 k straddle it
    u32x4 sc;            // seq8: scales[g][n .. n + 3] (8 bytes used for a 16-bit layer)
    u32x2 zw;            // seq8: the qzeros word(s) of the 4 columns
    u32x4 gk[2];         // per-k groups: g_idx[k .. k + 7]
};

template <typename T, int RB>
__device__ __forceinline__ void run(const Args& p, char* smem, int m0, int k0) {
    constexpr int ES = (int)sizeof(T);
    constexpr int BN = ROW_BYTES / ES;                    // n per stage
    constexpr int CQ = BN / 4;                            // column quads per stage
    constexpr int BM = RB * 32;
    constexpr int NA = BM * 8 / THREADS;                  // dY slots per thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wk = wave & 1;
    const int M = p.M, K = p.K, N = p.N, bits = p.bits;
    const unsigned maxq = (1u << bits) - 1u;
    const T* __restrict__ dy = (const T*)p.dy;
    const T* __restrict__ scales = (const T*)p.scales;
    const bool seq8 = p.g_idx == nullptr && (p.group_size & 7) == 0;
    const int zrow_words = N / 32 * bits;

    // this thread's dequantisation task: 8 consecutive k (kg) x 4 consecutive n (cq) of every stage
    const int cq = tid % CQ, kg = tid / CQ;
    const int kk = k0 + 8 * kg;
    const bool task = kg < BK / 8 && kk < K;
    const int bo = 8 * ((kk >> 3) & 3) * bits;           // bit offset of the 8 fields inside their 32-value pack
    const int row0 = (kk >> 5) * bits + (bo >> 5), sh = bo & 31;
    const bool two = sh + 8 * bits > 32;
    const int zbit = bits * 4 * cq;                        // + bits * n0 per stage
    const int g_seq = seq8 && task ? kk / p.group_size : 0;

    auto fetch = [&](Stage& s, int n0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int c = tid + THREADS * i, r = c >> 3, sl = c & 7;
            const bool ok = m0 + r < M && n0 + sl * (16 / ES) < N;
            s.a[i] = ok ? *(const u32x4*)((const char*)dy + ((size_t)(m0 + r) * N + n0) * ES + sl * 16) : u32x4{0, 0, 0, 0};
        }
        const int n = n0 + 4 * cq;
        const bool ok = task && n < N;
        s.q0 = ok ? *(const u32x4*)(p.qweight + (size_t)row0 * N + n) : u32x4{0, 0, 0, 0};
        s.q1 = ok && two ? *(const u32x4*)(p.qweight + (size_t)(row0 + 1) * N + n) : u32x4{0, 0, 0, 0};
        if (seq8) {
            if (ok) {
                const T* sp = scales + (size_t)g_seq * N + n;
                if constexpr (ES == 2) { const u32x2 v = *(const u32x2*)sp; s.sc = u32x4{v.x, v.y, 0, 0}; }
                else s.sc = *(const u32x4*)sp;
                const unsigned bit = (unsigned)(bits * n0 + zbit), wi = bit >> 5;
                const unsigned* zr = p.qzeros + (size_t)g_seq * zrow_words;
                s.zw = u32x2{zr[wi], ((bit & 31) + 4u * (unsigned)bits > 32u) ? zr[wi + 1] : 0u};
            }
        } else if (ok && p.g_idx) {
            s.gk[0] = *(const u32x4*)(p.g_idx + kk);
            s.gk[1] = *(const u32x4*)(p.g_idx + kk + 4);
        }
    };

    auto store = [&](const Stage& s, int n0, char* buf) {
        char* As = buf;
        char* Bs = buf + BM * ROW_BYTES;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int c = tid + THREADS * i;
            *(u32x4*)(As + swz(c >> 3, c & 7)) = s.a[i];
        }
        if (kg >= BK / 8) return;
        const int n = n0 + 4 * cq;
        const bool ok = task && n < N;
        float sf[4];
        int z[4];
        auto consts_from = [&](int g) {       // per-k groups: this k's scales / zeros straight from memory
#pragma unroll
            for (int c = 0; c < 4; ++c) sf[c] = DType<T>::to_f32(scales[(size_t)g * N + n + c]);
            zero_points4(p.qzeros + (size_t)g * zrow_words, n, bits, p.zero_mode, z);
        };
        if (seq8 && ok) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if constexpr (ES == 2) {
                    const unsigned w = c < 2 ? s.sc.x : s.sc.y;
                    sf[c] = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(w >> (16 * (c & 1)))));
                } else {
                    sf[c] = as_f32(c == 0 ? s.sc.x : c == 1 ? s.sc.y : c == 2 ? s.sc.z : s.sc.w);
                }
            }
            const unsigned bit = (unsigned)(bits * n0 + zbit);
            const unsigned long long v = (((unsigned long long)s.zw.y << 32) | s.zw.x) >> (bit & 31);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int f = (int)((v >> (bits * c)) & maxq) + 1;
                z[c] = p.zero_mode == GPTQ_ZERO_WRAP ? (f & (int)maxq) : f;
            }
        }
        unsigned long long qv[4];
        qv[0] = (((unsigned long long)s.q1.x << 32) | s.q0.x) >> sh;
        qv[1] = (((unsigned long long)s.q1.y << 32) | s.q0.y) >> sh;
        qv[2] = (((unsigned long long)s.q1.z << 32) | s.q0.z) >> sh;
        qv[3] = (((unsigned long long)s.q1.w << 32) | s.q0.w) >> sh;
        const int boff = cq * 4 * ES;                     // byte offset of the 4 columns inside a 128-byte row
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            T w[4];
            if (ok) {
                if (!seq8) {
                    const unsigned gi = i < 4 ? s.gk[0][i] : s.gk[1][i - 4];
                    consts_from(p.g_idx ? (int)gi : (kk + i) / p.group_size);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int f = (int)((qv[c] >> (bits * i)) & maxq);
                    w[c] = DType<T>::from_f32(sf[c] * (float)(f - z[c]));
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) w[c] = DType<T>::from_f32(0.f);
            }
            const int r = 8 * kg + i;
            char* dst = Bs + swz(r, boff >> 4) + (boff & 15);
            if constexpr (ES == 2) {
                u32x2 o;
                o.x = (unsigned)__builtin_bit_cast(unsigned short, w[0]) | ((unsigned)__builtin_bit_cast(unsigned short, w[1]) << 16);
                o.y = (unsigned)__builtin_bit_cast(unsigned short, w[2]) | ((unsigned)__builtin_bit_cast(unsigned short, w[3]) << 16);
                *(u32x2*)dst = o;
            } else {
                *(u32x4*)dst = u32x4{as_u32(w[0]), as_u32(w[1]), as_u32(w[2]), as_u32(w[3])};
            }
        }
    };

    f32x4 acc[RB][4];
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int BUF = (BM + BK) * ROW_BYTES;
    const int stages = (N + BN - 1) / BN;
    Stage st;
    st.zw = u32x2{0, 0};
    st.sc = st.gk[0] = st.gk[1] = u32x4{0, 0, 0, 0};
    fetch(st, 0);
    store(st, 0, smem);
    __syncthreads();
    const int arow = wm * (BM / 2) + (lane & 15), brow = wk * 64 + (lane & 15);
    for (int it = 0; it < stages; ++it) {
        const bool more = it + 1 < stages;
        if (more) fetch(st, (it + 1) * BN);
        const char* As = smem + (it & 1) * BUF;
        const char* Bs = As + BM * ROW_BYTES;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int sl = 4 * s + (lane >> 4);
            u32x4 a[RB], b[4];
#pragma unroll
            for (int i = 0; i < RB; ++i) a[i] = *(const u32x4*)(As + swz(arow + 16 * i, sl));
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *(const u32x4*)(Bs + swz(brow + 16 * j, sl));
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = Mma16<T>::run(a[i], b[j], acc[i][j]);
        }
        if (more) store(st, (it + 1) * BN, smem + ((it + 1) & 1) * BUF);
        __syncthreads();
    }

    // epilogue: [BM][128] fp32 through LDS (column ^ 16 on odd rows: the 4 rows one write instruction covers fall on both bank halves)
    float* E = (float*)smem;
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wm * (BM / 2) + 16 * i + 4 * (lane >> 4) + r, col = wk * 64 + 16 * j + (lane & 15);
                E[row * BK + (col ^ ((row & 1) << 4))] = acc[i][j][r];
            }
    __syncthreads();
    T* __restrict__ dx = (T*)p.dx;
#pragma unroll
    for (int i = 0; i < BM * 16 / THREADS; ++i) {
        const int item = tid + THREADS * i, row = item >> 4, c8 = (item & 15) * 8;
        const int m = m0 + row, k = k0 + c8;
        if (m >= M || k >= K) continue;
        const float* e = E + row * BK + (c8 ^ ((row & 1) << 4));
        const f32x4 lo = *(const f32x4*)e, hi = *(const f32x4*)(e + 4);
        float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        T* out = dx + (size_t)m * K + k;
        if constexpr (ES == 2) {
            if (p.accumulate) {
                const u32x4 o = *(const u32x4*)out;
                const unsigned ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    v[c] += DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(ow[c >> 1] >> (16 * (c & 1)))));
            }
            unsigned w[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                w[c] = (unsigned)__builtin_bit_cast(unsigned short, DType<T>::from_f32(v[2 * c])) |
                       ((unsigned)__builtin_bit_cast(unsigned short, DType<T>::from_f32(v[2 * c + 1])) << 16);
            *(u32x4*)out = u32x4{w[0], w[1], w[2], w[3]};
        } else {
            f32x4 a = lo, b = hi;
            if (p.accumulate) {
                a += *(const f32x4*)out;
                b += *(const f32x4*)(out + 4);
            }
            *(f32x4*)out = a;
            *(f32x4*)(out + 4) = b;
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(THREADS, 2) grad_input_kernel(Args p) {
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    const int total = gridDim.x;
    const int b = xcd_remap(blockIdx.x, total);        // consecutive k tiles of one row block on one XCD: they share dY in its L2
    const int kt = b % p.nkt, mt = b / p.nkt;
    if (p.bm == 128) run<T, 4>(p, smem, mt * 128, kt * BK);
    else run<T, 2>(p, smem, mt * 64, kt * BK);
}

}  // namespace gin

int grad_input_bm(const gptq_layer_t& L, int M) {
    // 128-row tiles where they still give 256 workgroups (a full round at one per CU), else 64 rows
    const long nkt = (L.K + gin::BK - 1) / gin::BK;
    return ((long)(M + 127) / 128) * nkt >= 256 ? 128 : 64;
}

hipError_t launch_grad_input(const gptq_layer_t& L, const void* dy, void* dx, int M, int accumulate, hipStream_t st) {
    gin::Args p;
    p.qweight = L.qweight;
    p.qzeros = L.qzeros;
    p.scales = L.scales;
    p.g_idx = L.g_idx;
    p.dy = dy;
    p.dx = dx;
    p.M = M;
    p.K = L.K;
    p.N = L.N;
    p.bits = L.bits;
    p.group_size = L.group_size;
    p.zero_mode = L.zero_mode;
    p.bm = grad_input_bm(L, M);
    p.nkt = (L.K + gin::BK - 1) / gin::BK;
    p.accumulate = accumulate ? 1 : 0;
    const long blocks = (long)p.nkt * ((M + p.bm - 1) / p.bm);
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(gin::THREADS);
    switch (L.dtype) {
        case GPTQ_F16: hipLaunchKernelGGL(gin::grad_input_kernel<f16>, grid, block, 0, st, p); break;
        case GPTQ_BF16: hipLaunchKernelGGL(gin::grad_input_kernel<bf16>, grid, block, 0, st, p); break;
        case GPTQ_F32: hipLaunchKernelGGL(gin::grad_input_kernel<float>, grid, block, 0, st, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gptq
