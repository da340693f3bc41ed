// moe_router.hip -- the router in front of a routed mixture-of-experts layer as ONE launch (gptq_moe_router): logits, softmax and top-k.
//
// The router weight is not quantized (the reference's Mixtral lists only w1 / w2 / w3 and the attention projections: auto_gptq/modeling/mixtral.py), so
// this is a dense fp16 / bf16 kernel beside the packed ones, like lora.hip.  For x [T, H] and w [E, H] in the layer dtype D:
//   logits     l[t, e] = D(sum_k x[t, k] * w[e, k])        fp32 products and sums in a fixed order, one rounding; all below is a function of these alone
//   selection  topk times the largest remaining logit, equal logits to the LOWER expert index; emitted in that order (descending logit, then ascending
//              index: sorted=True).  -0 equals +0 and a NaN ranks above every number, as in torch.sort; the comparison runs on a total order of
//              (logit, index) pairs, so the indices are distinct and inside [0, E) whatever the row holds.  These are the experts torch.topk on the
//              fp32 probabilities picks, except where that call's own tie order is undefined (equal logits, and logits whose probabilities round
//              to the same fp32).
//   weights    p_e = exp(l_e - max l) / sum_e exp(l_e - max l) in fp32 (lane-local ascending e, then a butterfly: fixed order); topk_w[t, j] = p_sel(j),
//              with GPTQ_ROUTER_RENORM divided by sum_j p_sel(j) in ascending j.
// No workspace, no atomics, no exchange between workgroups: a workgroup owns its tokens' whole rows of logits, and softmax and selection run in its
// epilogue on the rounded logits in LDS (one wave per token: a lane holds experts lane, lane + 64, lane + 128, lane + 192).
//   9+ tokens:  a workgroup is 16 tokens x all E experts x the whole H: up to sixteen 16-wide expert tiles of v_mfma_f32_16x16x32_{f16,bf16} on fragments
//               loaded as they lie in memory (both operands contiguous in k: lora.hip's down form).  8 waves take the 32-wide k-steps round robin and
//               meet in LDS, summed in wave order, four tiles at a time.  Expert rows >= E and token rows >= T are zero in registers, never loaded or stored.
//   1-8 tokens: a workgroup is one token; its x row is staged once in LDS, waves take experts round robin (four rows in flight per wave), lanes stride k
//               in 16-byte loads, butterfly across the wave.  Wave 0 runs the epilogue.
// The regime is a launch-uniform branch: one instantiation per dtype.  Within a regime a token's bits depend on nothing but its own row.
#include "common.cuh"
#include "launch.h"

namespace gptq {
namespace router {

constexpr int THREADS = 512;
constexpr int WAVES = THREADS / 64;
constexpr int TOKENS = 16;                  // tokens of a workgroup, tiles form
constexpr int CHUNK = 4;                    // expert tiles reduced through LDS at a time
constexpr int RED_FLOATS = WAVES * CHUNK * 256;

struct Args {
    const void* x;
    const void* w;
    void* logits;
    int64_t* idx;
    float* wts;
    int T, H, E, topk, renorm, rows;
};

template <typename T> struct Mma;
template <> struct Mma<f16> {
    static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};
template <> struct Mma<bf16> {
    static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};

template <typename T>
__device__ __forceinline__ void unpack8(u32x4 v, float (&f)[8]) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(w[c >> 1] >> (16 * (c & 1)))));
}

template <typename T>
__device__ __forceinline__ float round_to(float v) { return DType<T>::to_f32(DType<T>::from_f32(v)); }

// a logit as an unsigned key of the selection's total order: ascending with the value, -0 = +0, every NaN on top; never 0 (0 marks "no candidate")
__device__ __forceinline__ unsigned order_key(float v) {
    if (v != v) return 0xffffffffu;
    const unsigned u = as_u32(v + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// softmax and selection of one token by one wave; lg: the token's E rounded logits in LDS (as fp32)
template <typename T>
__device__ __forceinline__ void route_token(const float* lg, const Args& p, size_t t, int lane) {
    const int E = p.E, topk = p.topk;
    float v[4];
    unsigned long long key[4];
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int e = lane + 64 * s;
        const bool ok = e < E;
        v[s] = ok ? lg[e] : -INFINITY;
        key[s] = ok ? ((unsigned long long)order_key(v[s]) << 32) | (0xffffffffu - (unsigned)e) : 0ull;
        mx = fmaxf(mx, v[s]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    float pr[4], sum = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        pr[s] = lane + 64 * s < E ? expf(v[s] - mx) : 0.f;
        sum += pr[s];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
#pragma unroll
    for (int s = 0; s < 4; ++s) pr[s] = pr[s] / sum;

    // topk rounds of a wave-wide arg-max on (logit, index): lane j keeps the j-th choice
    unsigned taken = 0, my_idx = 0;
    float my_p = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < topk) {
            unsigned long long best = 0ull;
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (!((taken >> s) & 1u) && key[s] > best) best = key[s];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const unsigned long long o = __shfl_xor(best, off);
                best = o > best ? o : best;
            }
            const unsigned e = 0xffffffffu - (unsigned)best;      // topk <= E: a candidate is left in every round, so e < E
            float pv = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (e == (unsigned)(lane + 64 * s)) {
                    taken |= 1u << s;
                    pv = pr[s];
                }
            }
            pv = __shfl(pv, (int)(e & 63u));
            if (lane == j) {
                my_idx = e;
                my_p = pv;
            }
        }
    }
    if (p.renorm) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float pj = __shfl(my_p, j);
            if (j < topk) s += pj;
        }
        my_p = my_p / s;
    }
    if (lane < topk) {
        p.idx[t * topk + lane] = (int64_t)my_idx;
        p.wts[t * topk + lane] = my_p;
    }
    if (p.logits) {
        T* lo = (T*)p.logits + t * E;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = lane + 64 * s;
            if (e < E) lo[e] = DType<T>::from_f32(lg[e]);      // exact: lg holds rounded values
        }
    }
}

// the k-steps of one wave (st = wave, wave + 8, ..: ascending, U of them in flight) on up to NT expert tiles
template <typename T, int NT, int U>
__device__ __forceinline__ void tiles_kloop(const char* xp, bool xok, const char* wp, size_t tile_bytes, int E, int row, int steps, int wave, int ntiles,
                                            f32x4 (&acc)[16]) {
    const u32x4 zero = u32x4{0, 0, 0, 0};
    for (int st = wave; st < steps; st += U * WAVES) {
        u32x4 xa[U], wa[U][NT];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int s = st + i * WAVES;
            const bool in = s < steps;
            xa[i] = in && xok ? *(const u32x4*)(xp + (size_t)s * 64) : zero;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const bool wok = n * 16 + row < E;
                wa[i][n] = in && wok ? *(const u32x4*)(wp + (wok ? n * tile_bytes : 0) + (size_t)s * 64) : zero;
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i)
#pragma unroll
            for (int n = 0; n < NT; ++n)
                if (n < ntiles) acc[n] = Mma<T>::run(xa[i], wa[i][n], acc[n]);
    }
}

template <typename T>
__global__ void __launch_bounds__(THREADS) moe_router_kernel(Args p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.H, E = p.E;
    const T* __restrict__ x = (const T*)p.x;
    const T* __restrict__ w = (const T*)p.w;

    if (p.rows) {
        // ---- 1-8 tokens: one token per workgroup ----
        const size_t t = blockIdx.x;
        u32x4* xs = (u32x4*)smem;
        float* lg = (float*)(smem + (size_t)H * sizeof(T));
        const u32x4* xr = (const u32x4*)(x + t * H);
        for (int i = tid; i < H / 8; i += THREADS) xs[i] = xr[i];
        __syncthreads();
        const u32x4 zero = u32x4{0, 0, 0, 0};
        for (int e0 = wave; e0 < E; e0 += 4 * WAVES) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = lane * 8; k0 < H; k0 += 4 * 64 * 8) {
                u32x4 wv[4][4], xv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + u * 64 * 8;
                    const bool in = k < H;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = e0 + i * WAVES;
                        const bool ok = in && e < E;
                        wv[u][i] = ok ? *(const u32x4*)(w + (size_t)(ok ? e : 0) * H + (ok ? k : 0)) : zero;
                    }
                    xv[u] = in ? xs[k >> 3] : zero;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float xf[8];
                    unpack8<T>(xv[u], xf);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float wf[8];
                        unpack8<T>(wv[u][i], wf);
#pragma unroll
                        for (int c = 0; c < 8; ++c) a[i] = fmaf(xf[c], wf[c], a[i]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) a[i] += __shfl_xor(a[i], off);
                const int e = e0 + i * WAVES;
                if (lane == 0 && e < E) lg[e] = round_to<T>(a[i]);
            }
        }
        __syncthreads();
        if (wave == 0) route_token<T>(lg, p, t, lane);
        return;
    }

    // ---- 9+ tokens: 16 tokens x all experts per workgroup ----
    float* red = (float*)smem;                                  // [wave][tile of the chunk][token][expert]
    const int ntiles = (E + 15) >> 4, EP = ntiles * 16;
    float* lg = red + RED_FLOATS;                                // [token][EP]
    const size_t m0 = (size_t)blockIdx.x * TOKENS;
    const int row = lane & 15, kq = lane >> 4;
    const bool xok = m0 + row < (size_t)p.T;
    const char* xp = (const char*)(x + (xok ? m0 + row : 0) * H) + kq * 16;
    const char* wp = (const char*)(w + (size_t)(row < E ? row : 0) * H) + kq * 16;
    const size_t tile_bytes = (size_t)16 * H * sizeof(T);
    const int steps = H / 32;                                   // 64 bytes of a row per step
    f32x4 acc[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ntiles <= 1) tiles_kloop<T, 1, 4>(xp, xok, wp, tile_bytes, E, row, steps, wave, ntiles, acc);
    else if (ntiles <= 4) tiles_kloop<T, 4, 2>(xp, xok, wp, tile_bytes, E, row, steps, wave, ntiles, acc);
    else tiles_kloop<T, 16, 1>(xp, xok, wp, tile_bytes, E, row, steps, wave, ntiles, acc);

    // accumulator: column (l & 15) is the expert of the tile, rows 4 (l >> 4) + reg are tokens
#pragma unroll
    for (int c = 0; c < 16 / CHUNK; ++c) {
        if (c * CHUNK < ntiles) {
            if (c) __syncthreads();                             // the previous chunk has been read
#pragma unroll
            for (int i = 0; i < CHUNK; ++i) {
                const int n = c * CHUNK + i;
                if (n < ntiles) {
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) red[((wave * CHUNK + i) * 16 + 4 * kq + reg) * 16 + row] = acc[n][reg];
                }
            }
            __syncthreads();
            for (int v = tid; v < CHUNK * 256; v += THREADS) {
                const int i = v >> 8, n = c * CHUNK + i;
                if (n < ntiles) {
                    float s = 0.f;
#pragma unroll
                    for (int wv = 0; wv < WAVES; ++wv) s += red[(wv * CHUNK + i) * 256 + (v & 255)];
                    lg[((v >> 4) & 15) * EP + n * 16 + (v & 15)] = round_to<T>(s);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int m = 2 * wave + h;
        if (m0 + m < (size_t)p.T) route_token<T>(lg + m * EP, p, m0 + m, lane);
    }
}

}  // namespace router

RouterPlan plan_moe_router(int T, int H, int E, int topk, int dtype) {
    RouterPlan pl;
    pl.rows = T <= GPTQ_ROUTER_ROWS;
    pl.wg = pl.rows ? T : ((long)T + router::TOKENS - 1) / router::TOKENS;
    const int ntiles = (E + 15) / 16;
    const size_t rows_lds = (size_t)H * dtype_size(dtype) + (((size_t)E * 4 + 15) & ~(size_t)15);
    const size_t tiles_lds = (size_t)router::RED_FLOATS * 4 + (size_t)router::TOKENS * ntiles * 16 * 4;
    pl.lds_bytes = pl.rows ? rows_lds : tiles_lds;
    return pl;
}

hipError_t launch_moe_router(const void* x, const void* w, int T, int H, int E, int topk, int dtype, int renorm, void* logits, int64_t* idx, float* wts,
                             hipStream_t st) {
    const RouterPlan pl = plan_moe_router(T, H, E, topk, dtype);
    if (pl.wg < 1 || pl.wg > 0x7fffffffL || pl.lds_bytes > GPTQ_ROUTER_MAX_LDS) return hipErrorInvalidValue;
    router::Args p;
    p.x = x;
    p.w = w;
    p.logits = logits;
    p.idx = idx;
    p.wts = wts;
    p.T = T;
    p.H = H;
    p.E = E;
    p.topk = topk;
    p.renorm = renorm;
    p.rows = pl.rows ? 1 : 0;
    const dim3 grid((unsigned)pl.wg), block(router::THREADS);
    if (dtype == GPTQ_F16) hipLaunchKernelGGL(router::moe_router_kernel<f16>, grid, block, pl.lds_bytes, st, p);
    else if (dtype == GPTQ_BF16) hipLaunchKernelGGL(router::moe_router_kernel<bf16>, grid, block, pl.lds_bytes, st, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace gptq
