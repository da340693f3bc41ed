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
//
// The GROUPED-SIGMOID form (gptq_moe_router_grouped: DeepSeek-V3 / GLM-4 MoE) is a launch-uniform mode of the same two instantiations: the same two regimes
// and the same sums, but the logits stay fp32 (the reference casts x and w to fp32), and the epilogue is route_token_grouped:
//   scores     s_e = 1 / (1 + expf(-l_e)), c_e = s_e + bias_e (one fp32 add; no bias: c_e = s_e)
//   groups     (G > 1) group g = experts [g Eg, (g + 1) Eg); its score is the largest c plus the second largest (one add); the kg groups with the largest
//              score stay, equal scores to the LOWER group
//   selection  topk times the largest remaining c among the experts of the groups that stay, equal c to the LOWER expert; order_key's total order
//   weights    topk_w[t, j] = s_sel(j) (WITHOUT the bias), with GPTQ_ROUTER_RENORM divided by (sum_j s_sel(j) in ascending j) + 1e-20, then times scale
// Epilogue layout: the wave writes c over the token's logits in LDS; P = 64 / G' lanes per group (G' = G rounded up to a power of two) scan the group's Eg
// values P apart and keep a (largest, second) pair of keys, log2 P shuffle steps merge the pairs; a group's rank is counted over G lane reads of the
// group scores (no butterfly), one ballot marks the groups that stay, and the wave-wide arg-max rounds run on keys cleared outside them.
#include "common.cuh"
#include "mma_dequant.cuh"
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
    // the grouped-sigmoid form (mode = 1); logits is then fp32 [T, E]
    int mode, G, kg, Eg, P;                 // P = 64 / (G rounded up to a power of two): lanes per group
    float scale;
    const float* bias;                      // [E] or NULL
    float* scores;                          // fp32 [T, E] or NULL
};

template <typename T>
__device__ __forceinline__ float round_to(float v) { return DType<T>::to_f32(DType<T>::from_f32(v)); }

// a logit as an unsigned key of the selection's total order: ascending with the value, -0 = +0, every NaN on top; never 0 (0 marks "no candidate")
__device__ __forceinline__ unsigned order_key(float v) {
    if (v != v) return 0xffffffffu;
    const unsigned u = as_u32(v + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// topk rounds of a wave-wide arg-max on (value, index) keys (0: no candidate): lane j keeps the j-th choice and val of it
__device__ __forceinline__ void select_topk(const unsigned long long (&key)[4], const float (&val)[4], int topk, int lane, unsigned& my_idx, float& my_p) {
    unsigned taken = 0;
    my_idx = 0;
    my_p = 0.f;
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
            const unsigned e = 0xffffffffu - (unsigned)best;      // a candidate is left in every round (the plan's bound on topk), so e < E
            float pv = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (e == (unsigned)(lane + 64 * s)) {
                    taken |= 1u << s;
                    pv = val[s];
                }
            }
            pv = __shfl(pv, (int)(e & 63u));
            if (lane == j) {
                my_idx = e;
                my_p = pv;
            }
        }
    }
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

    unsigned my_idx;
    float my_p;
    select_topk(key, pr, topk, lane, my_idx, my_p);
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

// the value behind a key of order_key (a NaN for the NaN key)
__device__ __forceinline__ float key_value(unsigned k) { return as_f32((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// (k1 >= k2) the two largest keys seen: take one more
__device__ __forceinline__ void top2_push(unsigned& k1, unsigned& k2, unsigned k) {
    const unsigned lo = k > k1 ? k1 : k;
    k1 = k > k1 ? k : k1;
    k2 = lo > k2 ? lo : k2;
}

// the grouped-sigmoid form: scores, group choice and selection of one token by one wave; lg: the token's E fp32 logits in LDS, overwritten with c
__device__ __forceinline__ void route_token_grouped(float* lg, const Args& p, size_t t, int lane) {
    const int E = p.E, topk = p.topk;
    float sc[4], c[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int e = lane + 64 * s;
        sc[s] = c[s] = 0.f;
        if (e < E) {
            const float l = lg[e];
            sc[s] = 1.f / (1.f + expf(-l));
            c[s] = p.bias ? sc[s] + p.bias[e] : sc[s];
            if (p.logits) ((float*)p.logits)[t * E + e] = l;
            if (p.scores) p.scores[t * E + e] = sc[s];
        }
    }
    unsigned long long kept = ~0ull;                            // bit g P: group g stays
    if (p.G > 1) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (lane + 64 * s < E) lg[lane + 64 * s] = c[s];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int P = p.P, Eg = p.Eg, g = lane / P, r = lane - g * P;
        unsigned k1 = 0, k2 = 0;                                // Eg >= 2: both are set after the merge
        if (g < p.G)
            for (int j = r; j < Eg; j += P) top2_push(k1, k2, order_key(lg[g * Eg + j]));
        for (int off = 1; off < P; off <<= 1) {
            const unsigned o1 = __shfl_xor(k1, off), o2 = __shfl_xor(k2, off);
            const unsigned hi = k1 > o1 ? k1 : o1, lo = k1 > o1 ? o1 : k1, nx = k2 > o2 ? k2 : o2;
            k1 = hi;
            k2 = lo > nx ? lo : nx;
        }
        const unsigned gk = order_key(key_value(k1) + key_value(k2));
        int rank = 0;                                           // groups ahead of mine: a larger score, or an equal one at a lower index
        for (int h = 0; h < p.G; ++h) {
            const unsigned o = (unsigned)__builtin_amdgcn_readlane((int)gk, h * P);
            rank += (o > gk || (o == gk && h < g)) ? 1 : 0;
        }
        kept = __ballot(g < p.G && rank < p.kg);
    }
    unsigned long long key[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int e = lane + 64 * s;
        const bool ok = e < E && ((kept >> (p.G > 1 ? (e / p.Eg) * p.P : 0)) & 1ull);
        key[s] = ok ? ((unsigned long long)order_key(c[s]) << 32) | (0xffffffffu - (unsigned)e) : 0ull;
    }
    unsigned my_idx;
    float my_p;
    select_topk(key, sc, topk, lane, my_idx, my_p);
    if (p.renorm) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float pj = __shfl(my_p, j);
            if (j < topk) s += pj;
        }
        my_p = my_p / (s + 1e-20f);
    }
    my_p *= p.scale;
    if (lane < topk) {
        p.idx[t * topk + lane] = (int64_t)my_idx;
        p.wts[t * topk + lane] = my_p;
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
                if (n < ntiles) acc[n] = Mma16<T>::run(xa[i], wa[i][n], acc[n]);
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
                if (lane == 0 && e < E) lg[e] = p.mode ? a[i] : round_to<T>(a[i]);
            }
        }
        __syncthreads();
        if (wave == 0) {
            if (p.mode) route_token_grouped(lg, p, t, lane);
            else route_token<T>(lg, p, t, lane);
        }
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
                    lg[((v >> 4) & 15) * EP + n * 16 + (v & 15)] = p.mode ? s : round_to<T>(s);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int m = 2 * wave + h;
        if (m0 + m < (size_t)p.T) {
            if (p.mode) route_token_grouped(lg + m * EP, p, m0 + m, lane);
            else route_token<T>(lg + m * EP, p, m0 + m, lane);
        }
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

static hipError_t launch_router(router::Args p, int dtype, hipStream_t st) {
    const RouterPlan pl = plan_moe_router(p.T, p.H, p.E, p.topk, dtype);
    if (pl.wg < 1 || pl.wg > 0x7fffffffL || pl.lds_bytes > GPTQ_ROUTER_MAX_LDS) return hipErrorInvalidValue;
    p.rows = pl.rows ? 1 : 0;
    const dim3 grid((unsigned)pl.wg), block(router::THREADS);
    if (dtype == GPTQ_F16) hipLaunchKernelGGL(router::moe_router_kernel<f16>, grid, block, pl.lds_bytes, st, p);
    else if (dtype == GPTQ_BF16) hipLaunchKernelGGL(router::moe_router_kernel<bf16>, grid, block, pl.lds_bytes, st, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_moe_router(const void* x, const void* w, int T, int H, int E, int topk, int dtype, int renorm, void* logits, int64_t* idx, float* wts,
                             hipStream_t st) {
    router::Args p = {};
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
    return launch_router(p, dtype, st);
}

// the grouped-sigmoid form: the same plan (grid, LDS) as the softmax form
hipError_t launch_moe_router_grouped(const void* x, const void* w, const float* bias, int T, int H, int E, int topk, int n_group, int topk_group, float scale,
                                     int dtype, int renorm, float* logits, float* scores, int64_t* idx, float* wts, hipStream_t st) {
    if (n_group < 1 || n_group > 32 || E % n_group) return hipErrorInvalidValue;
    int gp = 1;
    while (gp < n_group) gp <<= 1;
    router::Args p = {};
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
    p.mode = 1;
    p.G = n_group;
    p.kg = topk_group;
    p.Eg = E / n_group;
    p.P = 64 / gp;
    p.scale = scale;
    p.bias = bias;
    p.scores = scores;
    return launch_router(p, dtype, st);
}

}  // namespace gptq
