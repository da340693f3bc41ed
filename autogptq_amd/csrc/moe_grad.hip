// moe_grad.hip -- the backward of the routed mixture-of-experts layer on the packed expert weights (gptq_moe_backward): dX and the router-weight gradient.
//
// Forward (moe.hip): g = x_t . W1_e, u = x_t . W3_e, h_r = T(silu(g) * u), z_r = h_r . W2_e, out[t] = T(sum_j w[t, j] z_(t, j)).  Given dOut [T][H] in the
// experts' dtype, for every valid assignment r = (t, j) with expert e (indices outside [0, E) are dropped):
//   d_r      = dOut[t] . W2_e^T                          fp32 sums over H, every W bit-exact to gptq_dequant
//   dw[t, j] = sum_i d_r[i] h_r[i]                       fp32, fixed order (= <dOut[t], z_r>: no Y buffer); h_r = T(silu(g_r) u_r)
//   dg_r     = T(w[t, j] d_r u_r silu'(g_r))             silu'(g) = s (1 + g (1 - s)), s = 1 / (1 + exp(-g)), on fp32, one rounding
//   du_r     = T(w[t, j] d_r silu(g_r))
//   dX[t]    = T(sum_j (dg_r . W1_e^T + du_r . W3_e^T))  fp32, ascending j, one rounding; a token without a valid expert gets a zero row
// The forward saves no activation: g_r, u_r are recomputed from x by the forward's grouped GEMM (its fp32 sums rounded once to T).
// Five launches, no host round trip, no atomics, nothing allocated (capturable in a hipGraph):
//   1. moe_route_kernel (moe.hip) with 64-row tiles: pos, sorted row -> assignment, the tile table.
//   2. moe_gemm_kernel (moe.hip), pair mode with the recompute epilogue: G_sorted, U_sorted [R][I] in T.
//   3. moe_grad_kernel<T>, down stage: a workgroup = one tile (<= 64 rows of one expert) x 128 columns of I; it walks H with dOut rows (gathered through the
//      sorted row's token) as A and W2_e^T as B; the epilogue reads G, U at the tile's rows and columns, overwrites them with dg, du (the thread that reads an
//      element writes it) and writes one fp32 partial of dw per (row, 128-column block).
//   4. moe_grad_kernel<T>, up stage: a workgroup = one tile x 128 columns of H; it walks I through W1_e^T with dg as A, then I through W3_e^T with du as A,
//      into the same accumulators; the fp32 rows go out as DXR [R][H].
//   5. moe_grad_combine_kernel: dX[t] = T(sum_j DXR[pos[t, j]]) in ascending j; dw[t, j] = its partials in ascending block order, 0 for pos < 0.
// The GEMM grids are bounds from (T, topk, E) alone (tiles <= floor(T topk / 64) + min(E, T topk)); workgroups past the routing kernel's tile count return.
//
// moe_grad_kernel walks its reduction axis on the scheme of the dense input-gradient kernel (grad_input.hip, whose header describes the LDS images, the
// swizzle and the fragment reads): stages of 128 bytes per row, A rows copied to LDS as they are, the packed words of the CHECKPOINT rows (qweight with g_idx:
// act-order experts are read in their own order, as gptq_grad_input reads them) dequantised and transposed into the swizzled [k][n] image,
// v_mfma_f32_16x16x32_{f16,bf16}, two LDS buffers and one barrier per stage.  What differs: the A rows come from a per-row pointer (a row past the tile is
// zero, and 16-row blocks the tile does not have are skipped), the weight pointers come from the expert's entry of a device table, and the epilogue is the
// stage's own.  The tile is always 64 rows, so the summation order of every output element is that of the stages: independent of the routing.
#include <string.h>

#include <algorithm>

#include "common.cuh"
#include "mma_dequant.cuh"
#include "launch.h"

namespace gptq {
namespace mgrad {

constexpr int THREADS = 256;                // 4 waves: 2 (rows) x 2 (column halves of 64)
constexpr int BM = 64;                      // tile height (the routing kernel's bm)
constexpr int BK = 128;                     // output columns per workgroup
constexpr int ROW_BYTES = 128;              // one LDS image row per stage: 8 slots of 16 bytes (the row swz() of mma_dequant.cuh lays out)
constexpr int BN = 64;                      // reduction elements per stage (16-bit dtypes)
constexpr int CQ = BN / 4;                  // column quads per stage
constexpr int BUF = (BM + BK) * ROW_BYTES;  // one buffer: A image + B image
constexpr int LDS_BYTES = 2 * BUF;          // 48 KiB >= the fp32 epilogue tile [64][128] (32 KiB)

struct ExpertPtrs {                         // one entry of the backward table: [3 projections][E], the checkpoint rows
    const unsigned* qweight;
    const unsigned* qzeros;
    const void* scales;
    const int* g_idx;                       // NULL: sequential groups
};

struct Args {
    const ExpertPtrs* table;                // [3][E]: W1, W3, W2
    int E, up;                              // up = 0: down stage; 1: up stage
    const void* dout;                       // [T][H]
    const float* w;                         // [T * topk]
    const int* row_assign;
    const int* tile_count;
    const int4* tiles;
    int topk, H, I, nkt;                    // nkt: 128-column blocks of this stage's output
    int bits1, gs1, zm1;                    // gate / up layers
    int bits2, gs2, zm2;                    // down layers
    void* g;                                // [R][I] T: G in, dg out (down stage); dg in (up stage)
    void* u;                                // [R][I] T: U in, du out; du in
    float* dwp;                             // [R][nblk_i] or NULL
    float* dxr;                             // [R][H]
};

struct Weights {                            // one layer as dX = A . W^T sees it: K output columns, N reduction elements
    const unsigned* qweight;
    const unsigned* qzeros;
    const void* scales;
    const int* g_idx;
    int K, N, bits, group_size, zero_mode;
};

// the raw words one thread loads for a stage (consumed by store() after the matrix-core work of the previous stage)
struct Stage {
    u32x4 a[2];          // A: 16-byte slots of the A image
    u32x4 q0, q1;        // packed words of 4 columns: the word holding the task's first k, and the next one when the 8 k straddle it
    u32x2 sc;            // seq8: scales[g][n .. n + 3]
    u32x2 zw;            // seq8: the qzeros word(s) of the 4 columns
    u32x4 gk[2];         // per-k groups: g_idx[k .. k + 7]
};

// acc += A[64][N] . W^T[N][k0 .. k0 + 127]: a0 / a1 are the rows (tid >> 3) and (tid >> 3) + 32 of A (NULL: a row the tile does not have, read as zero), rb
// the number of 16-row blocks the tile has.  Ends behind a barrier: the LDS is free again.
template <typename T>
__device__ __forceinline__ void walk(const Weights& p, const T* a0, const T* a1, int rb, char* smem, int k0, f32x4 (&acc)[2][4]) {
    const T* const arow[2] = {a0, a1};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wk = wave & 1;
    const int K = p.K, N = p.N, bits = p.bits;
    const unsigned maxq = (1u << bits) - 1u;
    const T* __restrict__ scales = (const T*)p.scales;
    const bool seq8 = p.g_idx == nullptr && (p.group_size & 7) == 0;
    const int zrow_words = N / 32 * bits;

    // this thread's dequantisation task: 8 consecutive k (kg) x 4 consecutive n (cq) of every stage
    const int cq = tid % CQ, kg = tid / CQ;
    const int kk = k0 + 8 * kg;
    const bool task = kk < K;                              // (kg < BK / 8 for every thread: 256 / 16 = 16 groups)
    const int bo = 8 * ((kk >> 3) & 3) * bits;            // bit offset of the 8 fields inside their 32-value pack
    const int row0 = (kk >> 5) * bits + (bo >> 5), sh = bo & 31;
    const bool two = sh + 8 * bits > 32;
    const int zbit = bits * 4 * cq;                        // + bits * n0 per stage
    const int g_seq = seq8 && task ? kk / p.group_size : 0;

    auto fetch = [&](Stage& s, int n0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            s.a[i] = arow[i] ? *(const u32x4*)((const char*)(arow[i] + n0) + (tid & 7) * 16) : u32x4{0, 0, 0, 0};
        const int n = n0 + 4 * cq;
        s.q0 = task ? *(const u32x4*)(p.qweight + (size_t)row0 * N + n) : u32x4{0, 0, 0, 0};
        s.q1 = task && two ? *(const u32x4*)(p.qweight + (size_t)(row0 + 1) * N + n) : u32x4{0, 0, 0, 0};
        if (seq8) {
            if (task) {
                s.sc = *(const u32x2*)(scales + (size_t)g_seq * N + n);
                const unsigned bit = (unsigned)(bits * n0 + zbit), wi = bit >> 5;
                const unsigned* zr = p.qzeros + (size_t)g_seq * zrow_words;
                s.zw = u32x2{zr[wi], ((bit & 31) + 4u * (unsigned)bits > 32u) ? zr[wi + 1] : 0u};
            }
        } else if (task && p.g_idx) {
            s.gk[0] = *(const u32x4*)(p.g_idx + kk);
            s.gk[1] = *(const u32x4*)(p.g_idx + kk + 4);
        }
    };

    auto store = [&](const Stage& s, int n0, char* buf) {
        char* As = buf;
        char* Bs = buf + BM * ROW_BYTES;
#pragma unroll
        for (int i = 0; i < 2; ++i) *(u32x4*)(As + swz((tid >> 3) + 32 * i, tid & 7)) = s.a[i];
        const int n = n0 + 4 * cq;
        float sf[4];
        int z[4];
        auto consts_from = [&](int g) {       // per-k groups: this k's scales / zeros straight from memory
#pragma unroll
            for (int c = 0; c < 4; ++c) sf[c] = DType<T>::to_f32(scales[(size_t)g * N + n + c]);
            zero_points4(p.qzeros + (size_t)g * zrow_words, n, bits, p.zero_mode, z);
        };
        if (seq8 && task) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned w = c < 2 ? s.sc.x : s.sc.y;
                sf[c] = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(w >> (16 * (c & 1)))));
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
        const int boff = cq * 8;                          // byte offset of the 4 columns inside a 128-byte row
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            T w[4];
            if (task) {
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
            u32x2 o;
            o.x = (unsigned)__builtin_bit_cast(unsigned short, w[0]) | ((unsigned)__builtin_bit_cast(unsigned short, w[1]) << 16);
            o.y = (unsigned)__builtin_bit_cast(unsigned short, w[2]) | ((unsigned)__builtin_bit_cast(unsigned short, w[3]) << 16);
            *(u32x2*)(Bs + swz(r, boff >> 4) + (boff & 15)) = o;
        }
    };

    const int stages = N / BN;                             // N is a multiple of 64
    Stage st;
    st.zw = st.sc = u32x2{0, 0};
    st.gk[0] = st.gk[1] = u32x4{0, 0, 0, 0};
    fetch(st, 0);
    store(st, 0, smem);
    __syncthreads();
    const int arow_l = wm * (BM / 2) + (lane & 15), brow = wk * 64 + (lane & 15);
    for (int it = 0; it < stages; ++it) {
        const bool more = it + 1 < stages;
        if (more) fetch(st, (it + 1) * BN);
        const char* As = smem + (it & 1) * BUF;
        const char* Bs = As + BM * ROW_BYTES;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int sl = 4 * s + (lane >> 4);
            u32x4 a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *(const u32x4*)(As + swz(arow_l + 16 * i, sl));
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *(const u32x4*)(Bs + swz(brow + 16 * j, sl));
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (2 * wm + i >= rb) continue;           // a 16-row block the tile does not have (uniform over the wave)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = Mma16<T>::run(a[i], b[j], acc[i][j]);
            }
        }
        if (more) store(st, (it + 1) * BN, smem + ((it + 1) & 1) * BUF);
        __syncthreads();
    }
}

template <typename T>
__device__ __forceinline__ float elem(unsigned w, int hi) {
    return DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(w >> (16 * hi))));
}
template <typename T>
__device__ __forceinline__ unsigned pack2(float a, float b) {
    return (unsigned)__builtin_bit_cast(unsigned short, DType<T>::from_f32(a)) | ((unsigned)__builtin_bit_cast(unsigned short, DType<T>::from_f32(b)) << 16);
}

template <typename T>
__global__ void __launch_bounds__(THREADS, 2) moe_grad_kernel(Args p) {
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    const int b = xcd_remap(blockIdx.x, gridDim.x);    // consecutive column blocks of one tile on one XCD: they share the A rows in its L2
    const int kt = b % p.nkt, tile = b / p.nkt;
    if (tile >= *p.tile_count) return;
    const int4 tl = p.tiles[tile];
    const int e = tl.x, row0 = tl.y, rows = tl.z;
    const int rb = (rows + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wk = wave & 1;
    const int k0 = kt * BK;
    const int H = p.H, I = p.I;

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // down stage: dOut rows (through the sorted row's token) x W2_e^T; up stage: dg rows x W1_e^T, then du rows x W3_e^T into the same accumulators
    const int passes = p.up ? 2 : 1;
    for (int ps = 0; ps < passes; ++ps) {
        const ExpertPtrs ep = p.table[(p.up ? ps : 2) * p.E + e];
        Weights W;
        W.qweight = ep.qweight; W.qzeros = ep.qzeros; W.scales = ep.scales; W.g_idx = ep.g_idx;
        if (p.up) { W.K = H; W.N = I; W.bits = p.bits1; W.group_size = p.gs1; W.zero_mode = p.zm1; }
        else { W.K = I; W.N = H; W.bits = p.bits2; W.group_size = p.gs2; W.zero_mode = p.zm2; }
        const T* arow[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = (tid >> 3) + 32 * i;
            if (r >= rows) arow[i] = nullptr;
            else if (p.up) arow[i] = (const T*)(ps ? p.u : p.g) + (size_t)(row0 + r) * I;
            else arow[i] = (const T*)p.dout + (size_t)(p.row_assign[row0 + r] / p.topk) * H;
        }
        walk<T>(W, arow[0], arow[1], rb, smem, k0, acc);
    }

    // epilogue: [64][128] fp32 through LDS (column ^ 16 on odd rows: the 4 rows one write instruction covers fall on both bank halves)
    float* E = (float*)smem;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wm * (BM / 2) + 16 * i + 4 * (lane >> 4) + r, col = wk * 64 + 16 * j + (lane & 15);
                E[row * BK + (col ^ ((row & 1) << 4))] = acc[i][j][r];
            }
    __syncthreads();
    const int KO = p.up ? H : I;                           // this stage's output columns
#pragma unroll
    for (int i = 0; i < BM * 16 / THREADS; ++i) {
        const int item = tid + THREADS * i, row = item >> 4, c8 = (item & 15) * 8;   // the 16 lanes of a row are consecutive lanes of one wave
        const int k = k0 + c8;
        const bool live = row < rows && k < KO;
        float v[8];
        {
            const float* ep = E + row * BK + (c8 ^ ((row & 1) << 4));
            const f32x4 lo = *(const f32x4*)ep, hi = *(const f32x4*)(ep + 4);
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        }
        if (p.up) {
            if (live) {
                float* out = p.dxr + (size_t)(row0 + row) * H + k;
                *(f32x4*)out = f32x4{v[0], v[1], v[2], v[3]};
                *(f32x4*)(out + 4) = f32x4{v[4], v[5], v[6], v[7]};
            }
            continue;
        }
        float part = 0.f;
        if (live) {
            const size_t at = (size_t)(row0 + row) * I + k;
            const u32x4 gw = *(const u32x4*)((const T*)p.g + at), uw = *(const u32x4*)((const T*)p.u + at);
            const float wt = p.w[p.row_assign[row0 + row]];
            const unsigned gws[4] = {gw.x, gw.y, gw.z, gw.w}, uws[4] = {uw.x, uw.y, uw.z, uw.w};
            float dg[8], du[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float gv = elem<T>(gws[c >> 1], c & 1), uv = elem<T>(uws[c >> 1], c & 1);
                const float den = 1.f + __expf(-gv);
                const float sg = 1.f / den, silu = gv / den;
                const float h = DType<T>::to_f32(DType<T>::from_f32(silu * uv));      // h_r as the forward's epilogue forms and rounds it
                part += v[c] * h;
                const float wd = wt * v[c];
                dg[c] = wd * uv * (sg * (1.f + gv * (1.f - sg)));
                du[c] = wd * silu;
            }
            *(u32x4*)((T*)p.g + at) = u32x4{pack2<T>(dg[0], dg[1]), pack2<T>(dg[2], dg[3]), pack2<T>(dg[4], dg[5]), pack2<T>(dg[6], dg[7])};
            *(u32x4*)((T*)p.u + at) = u32x4{pack2<T>(du[0], du[1]), pack2<T>(du[2], du[3]), pack2<T>(du[4], du[5]), pack2<T>(du[6], du[7])};
        }
        if (p.dwp) {                                       // (uniform) the row's 128 columns: 8 per lane in ascending order, then a fixed tree over its 16 lanes
            part += __shfl_xor(part, 8);
            part += __shfl_xor(part, 4);
            part += __shfl_xor(part, 2);
            part += __shfl_xor(part, 1);
            if ((item & 15) == 0 && row < rows) p.dwp[(size_t)(row0 + row) * p.nkt + kt] = part;
        }
    }
}

struct CombineArgs {
    const int* pos;
    const float* dxr;                           // [R][H]
    const float* dwp;                           // [R][nblk]
    void* dx;                                   // [T][H] or NULL
    float* dw;                                  // [T][topk] or NULL
    int T, topk, H, nblk, dtype;
    long dx_items;                              // T * H / 4 when dx, else 0
};

__global__ void __launch_bounds__(256) moe_grad_combine_kernel(CombineArgs p) {
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item < p.dx_items) {
        const int quads = p.H / 4;
        const int t = (int)(item / quads), c4 = 4 * (int)(item % quads);
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < p.topk; ++j) {
            const int r = p.pos[t * p.topk + j];
            if (r < 0) continue;
            acc += *(const f32x4*)(p.dxr + (size_t)r * p.H + c4);
        }
        unsigned short o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            o[c] = p.dtype == GPTQ_F16 ? __builtin_bit_cast(unsigned short, DType<f16>::from_f32(acc[c]))
                                       : __builtin_bit_cast(unsigned short, DType<bf16>::from_f32(acc[c]));
        *(u32x2*)((unsigned short*)p.dx + (size_t)t * p.H + c4) = u32x2{o[0] | ((unsigned)o[1] << 16), o[2] | ((unsigned)o[3] << 16)};
        return;
    }
    const long a = item - p.dx_items;
    if (!p.dw || a >= (long)p.T * p.topk) return;
    const int r = p.pos[a];
    float s = 0.f;
    if (r >= 0)
        for (int bk = 0; bk < p.nblk; ++bk) s += p.dwp[(size_t)r * p.nblk + bk];
    p.dw[a] = s;
}

}  // namespace mgrad

MoeGradPlan plan_moe_grad(int E, int T, int topk, int H, int I, int dtype) {
    MoeGradPlan pl{};
    const long R = (long)T * topk;
    pl.tiles = (int)(R / mgrad::BM + std::min<long>(E, R));
    pl.nblk_i = (I + mgrad::BK - 1) / mgrad::BK;
    pl.nblk_h = (H + mgrad::BK - 1) / mgrad::BK;
    const size_t es = dtype_size(dtype);
    size_t o = append_route_layout(pl, GPTQ_WORKSPACE_HEADER_BYTES, E, pl.tiles, R);      // the header of a shared workspace belongs to the other entry points: left as it is
    pl.off_g = o; o += align256((size_t)R * I * es);
    pl.off_u = o; o += align256((size_t)R * I * es);
    pl.off_dwp = o; o += align256(4 * (size_t)R * pl.nblk_i);
    pl.off_dxr = o; o += align256(4 * (size_t)R * H);
    pl.bytes = o;
    return pl;
}

size_t moe_grad_table_entry_bytes() { return sizeof(mgrad::ExpertPtrs); }

void moe_grad_table_entry(const gptq_layer_t& L, void* dst) {
    mgrad::ExpertPtrs p;
    p.qweight = L.qweight;
    p.qzeros = L.qzeros;
    p.scales = L.scales;
    p.g_idx = L.g_idx;
    memcpy(dst, &p, sizeof(p));
}

hipError_t launch_moe_grad(const gptq_moe_t& m, const void* table, const void* grad_table, const MoeGradPlan& pl, const void* x, const int64_t* idx,
                           const float* w, const void* dout, int T, int topk, void* dx, float* dw, char* ws, hipStream_t st) {
    const gptq_layer_t& G = *m.gate[0];
    const gptq_layer_t& D = *m.down[0];
    const int E = m.E, H = G.K, I = G.N;
    int* const tile_count = (int*)(ws + pl.off_tile_count);
    int4* const tiles = (int4*)(ws + pl.off_tiles);
    int* const pos = (int*)(ws + pl.off_pos);
    int* const row_assign = (int*)(ws + pl.off_rows);
    hipError_t e = launch_moe_route(idx, T, topk, E, mgrad::BM, (int*)(ws + pl.off_offsets), tile_count, tiles, pos, row_assign, st);
    if (e != hipSuccess) return e;
    if ((e = launch_moe_recompute(m, table, x, row_assign, tile_count, tiles, pl.tiles, T, topk, ws + pl.off_g, ws + pl.off_u, st)) != hipSuccess) return e;

    mgrad::Args a;
    a.table = (const mgrad::ExpertPtrs*)grad_table;
    a.E = E; a.up = 0; a.dout = dout; a.w = w; a.row_assign = row_assign; a.tile_count = tile_count; a.tiles = tiles;
    a.topk = topk; a.H = H; a.I = I; a.nkt = pl.nblk_i;
    a.bits1 = G.bits; a.gs1 = G.group_size; a.zm1 = G.zero_mode;
    a.bits2 = D.bits; a.gs2 = D.group_size; a.zm2 = D.zero_mode;
    a.g = ws + pl.off_g; a.u = ws + pl.off_u;
    a.dwp = dw ? (float*)(ws + pl.off_dwp) : nullptr;
    a.dxr = (float*)(ws + pl.off_dxr);
    auto stage = [&](const mgrad::Args& s, long blocks) -> hipError_t {
        if (blocks <= 0) return hipSuccess;
        if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
        if (G.dtype == GPTQ_F16) hipLaunchKernelGGL(mgrad::moe_grad_kernel<f16>, dim3((unsigned)blocks), dim3(mgrad::THREADS), 0, st, s);
        else hipLaunchKernelGGL(mgrad::moe_grad_kernel<bf16>, dim3((unsigned)blocks), dim3(mgrad::THREADS), 0, st, s);
        return hipGetLastError();
    };
    if ((e = stage(a, (long)pl.tiles * pl.nblk_i)) != hipSuccess) return e;
    if (dx) {
        a.up = 1; a.nkt = pl.nblk_h;
        if ((e = stage(a, (long)pl.tiles * pl.nblk_h)) != hipSuccess) return e;
    }

    mgrad::CombineArgs c;
    c.pos = pos; c.dxr = a.dxr; c.dwp = a.dwp; c.dx = dx; c.dw = dw;
    c.T = T; c.topk = topk; c.H = H; c.nblk = pl.nblk_i; c.dtype = G.dtype;
    c.dx_items = dx ? (long)T * (H / 4) : 0;
    const long items = c.dx_items + (dw ? (long)T * topk : 0);
    hipLaunchKernelGGL(mgrad::moe_grad_combine_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, c);
    return hipGetLastError();
}

}  // namespace gptq
