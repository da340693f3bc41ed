// moe.hip -- routed mixture-of-experts layers on the packed expert weights (gptq_moe_forward): every row of the grouped GEMMs may belong to another expert.
//
// What one call computes (T tokens, topk assignments r = (t, j) each, expert e = top_k_index[t, j]; indices outside [0, E) are dropped):
//   g = x_t . W1_e,  u = x_t . W3_e          fp32 sums, every W bit-exact to gptq_dequant
//   h_r = T(silu(g) * u)                     silu and the product on fp32, one rounding (the SILU_MUL epilogue's convention)
//   y_r = w[t, j] * (h_r . W2_e)             fp32; routing weights read as fp32
//   out[t] = T(sum_j y_(t, j))               ascending j, one rounding; a token without a valid expert gets 0
// Four launches, no host round trip (capturable in a hipGraph):
//   1. moe_route_kernel (one workgroup): per-expert counts and offsets, pos[t, j] (the sorted row of the assignment, or -1), sorted row -> assignment, and a
//      table of tiles (expert, first row, rows <= BM) with its count.  Rows of one expert keep the order of their assignments (t * topk + j): ranks come from
//      per-wave counts in LDS and a shuffle scan inside the wave, no floating point, no ordering race.
//   2. moe_gemm_kernel<T>, pair mode: W1 and W3 over the same 64 columns of the tile in one workgroup, silu * mul -> H_sorted [R][I] in T.
//   3. moe_gemm_kernel<T>, down mode: H_sorted . W2 -> Y [ksplit][R][H] fp32 (K slices of the down projection when the tiles alone do not fill the chip).
//   4. moe_combine_kernel: out[t] = T(sum_j w[t, j] * sum_s Y[s][pos[t, j]]): fixed orders, so results are bit-reproducible and independent of the tiling.
// The GEMM grid is a bound computed from (T, topk, E) alone -- tiles <= floor(T topk / BM) + min(E, T topk) -- times the column blocks (times the K slices);
// workgroups past the tile count the routing kernel wrote return at once.
//
// moe_gemm_kernel: a workgroup = one tile (up to 64 rows of one expert) x 64 columns x its K range; its 4 waves take the 32-deep k-steps of the range in turn
// (wave w: steps w, w + 4, ...) and meet once, through LDS, in wave order.  Per k-step a lane (column quad cq = lane & 15, k-slot ks = lane >> 4)
//   * loads the 16 bytes qweight[k0 / 8 + ks][n0 + 4 cq .. + 3] of the checkpoint rows (qweight_seq for act-order experts): at 4 bits each word is the 8
//     consecutive k of one column that lane (n = lane & 15, k-slot = lane >> 4) of v_mfma_f32_16x16x32_{f16,bf16} takes -- 4 words = 4 MFMAs, column c of
//     the quad in MFMA c; at 8 bits a fragment is two words (rows k0 / 4 + 2 ks, + 1);
//   * dequantises them with the magic-number form of the panel / rows kernels (Deq1, Deq1_8: w - z exact in packed fp16, times the scale with one
//     rounding: bit-exact W).  On checkpoint words that form yields the k of a fragment in the order (0,4,1,5,2,6,3,7) (8 bits: (0,2,1,3,4,6,5,7)), so
//     the A fragment is permuted the same way (4 v_perm_b32) -- the MFMA pairs A and B element by element;
//     2 and 3 bits (GPTQ_MOE_LOW_BIT): the lane cuts its 8 fields out of the step's rows -- 3 bits: bits 24 ks .. 24 ks + 23 of the column's 96 (rows
//     3 st + lo and 3 st + min(lo + 1, 2), lo = 24 ks >> 5: two 16-byte loads and one v_alignbit_b32 per column), 2 bits: half ks & 1 of row
//     2 st + (ks >> 1) -- moves fields 0..3 | 4..7 to the two halves of a register and reads them in place (Deq1_3's readers, Deq1_2): the
//     4-bit k order, so order_a is the 4-bit one;
//   * reads its A fragment (row lane & 15 of each 16-row block of the tile, 8 consecutive k) straight from global memory: x gathered through the sorted row's
//     token (pair mode) or the H_sorted row (down mode); act-order experts gather the 8 columns through the expert's perm (W3 through its own when it has
//     another order than W1; a checkpoint's gate / up share one).  Rows past the tile repeat its
//     last row (results discarded), so the loop has no branches on the row count.
// Groups: group_size is a multiple of 32 (or covers K), so a 32-deep step lies in one group: group = k0 / group_size, uniform over the wave (for act-order
// experts k0 is the position in the re-sequenced rows).  bits, the group mode, the rows of the tile and the epilogue are runtime-uniform: two instantiations.
// The four zero points of a lane are 4 fields at bit bits * n of the group's qzeros row: one word, except the 3-bit quads with n % 32 in {8, 20}, which
// straddle two (the second word is read only then: the last quad of a row never straddles, N being a multiple of 64).
#include <string.h>

#include <algorithm>

#include "common.cuh"
#include "launch.h"
#include "mma_dequant.cuh"           // Mma16<T>, Scale4<T>, Deq1<T> / Deq1_8<T> / Deq1_3<T> / Deq1_2<T>: the magic-number dequantisation

namespace gptq {
namespace moe {

constexpr int THREADS = 256;
constexpr int BN = 64;
constexpr int MAX_ROWS = 64;                    // tile height bound (4 blocks of 16 rows)
constexpr int ROUTE_THREADS = 1024;

struct ExpertPtrs {                             // one entry of the device table: [3 projections][E]
    const unsigned* qweight;                    // qweight_seq when the expert is act-order, else qweight
    const unsigned* qzeros;
    const void* scales;
    const int* perm;                            // NULL: sequential groups
};

struct RouteArgs {
    const long long* idx;
    int T, topk, E, bm;
    int* offsets;                               // [E + 1]
    int* tile_count;
    int4* tiles;                                // (expert, first row, rows, 0)
    int* pos;                                   // [T * topk]
    int* row_assign;                            // [T * topk]: sorted row -> t * topk + j
};

__global__ void __launch_bounds__(ROUTE_THREADS) moe_route_kernel(RouteArgs p) {
    __shared__ int cnt[256], base[256], off[257];
    __shared__ int wcnt[ROUTE_THREADS / 64][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = p.T * p.topk, E = p.E;
    if (tid < E) cnt[tid] = 0;
    __syncthreads();
    for (int a = tid; a < R; a += ROUTE_THREADS) {
        const long long e = p.idx[a];
        if (e >= 0 && e < E) atomicAdd(&cnt[(int)e], 1);          // integer counts: the order of the increments does not matter
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0, tl = 0;
        for (int e = 0; e < E; ++e) {
            off[e] = o;
            o += cnt[e];
            base[e] = tl;                                         // (first tile of expert e, for the table below)
            tl += (cnt[e] + p.bm - 1) / p.bm;
        }
        off[E] = o;
        *p.tile_count = tl;
    }
    __syncthreads();
    if (tid <= E) p.offsets[tid] = off[tid];
    if (tid < E) {
        const int c = cnt[tid], nt = (c + p.bm - 1) / p.bm;
        for (int i = 0; i < nt; ++i) p.tiles[base[tid] + i] = int4{tid, off[tid] + i * p.bm, min(p.bm, c - i * p.bm), 0};
    }
    __syncthreads();
    if (tid < E) base[tid] = 0;                                  // rows of expert e placed so far
    for (int c0 = 0; c0 < R; c0 += ROUTE_THREADS) {
        for (int i = tid; i < (ROUTE_THREADS / 64) * 256; i += ROUTE_THREADS) (&wcnt[0][0])[i] = 0;
        const int a = c0 + tid;
        int e = -1;
        if (a < R) {
            const long long v = p.idx[a];
            e = (v >= 0 && v < E) ? (int)v : -1;
        }
        // rank among the lanes of this wave with the same expert, and whether this lane is the wave's last one for it
        int below = 0, above = 0;
        for (int s = 0; s < 64; ++s) {
            const int es = __shfl(e, s);
            below += (s < lane && es == e) ? 1 : 0;
            above += (s > lane && es == e) ? 1 : 0;
        }
        __syncthreads();
        if (e >= 0 && above == 0) wcnt[wave][e] = below + 1;
        __syncthreads();
        if (a < R) {
            if (e >= 0) {
                int rank = base[e] + below;
                for (int w = 0; w < wave; ++w) rank += wcnt[w][e];
                const int r = off[e] + rank;
                p.pos[a] = r;
                p.row_assign[r] = a;
            } else {
                p.pos[a] = -1;
            }
        }
        __syncthreads();
        if (tid < E) {
            int add = 0;
            for (int w = 0; w < ROUTE_THREADS / 64; ++w) add += wcnt[w][tid];
            base[tid] += add;
        }
        __syncthreads();
    }
}

struct GemmArgs {
    const ExpertPtrs* table;                    // entries of the first projection (pair mode: W1; W3 is table + E)
    int E;
    int pair;                                   // 1: W1 / W3 + silu * mul -> H (T); 0: one projection -> Y (fp32); 2: W1 / W3 -> G, U (T): the backward's recompute
    const void* a;                              // pair: x [T][K]; down: H_sorted [R][K]
    const int* row_assign;
    int topk;
    const int* tile_count;
    const int4* tiles;
    int K, N, bits, group_size, zero_mode;
    int nblk, ksplit, steps_per_split;          // column blocks; K slices and 32-deep steps per slice
    void* out;                                  // pair: H_sorted [R][N] (T); down: Y [ksplit][rstride][N] fp32; pair == 2: G_sorted [R][N] (T)
    int rstride;
    void* out2;                                 // pair == 2: U_sorted [R][N] (T)
};

// A fragment of one lane: 8 consecutive k of one row, put in the order the dequantised B fragment has
__device__ __forceinline__ u32x4 order_a(u32x4 v, int bits) {
    if (bits != 8)      // 2, 3, 4 bits: (0,4,1,5,2,6,3,7)
        return u32x4{__builtin_amdgcn_perm(v.z, v.x, 0x05040100u), __builtin_amdgcn_perm(v.z, v.x, 0x07060302u),
                     __builtin_amdgcn_perm(v.w, v.y, 0x05040100u), __builtin_amdgcn_perm(v.w, v.y, 0x07060302u)};
    return u32x4{__builtin_amdgcn_perm(v.y, v.x, 0x05040100u), __builtin_amdgcn_perm(v.y, v.x, 0x07060302u),   // 8 bits: (0,2,1,3,4,6,5,7)
                 __builtin_amdgcn_perm(v.w, v.z, 0x05040100u), __builtin_amdgcn_perm(v.w, v.z, 0x07060302u)};
}

template <typename T>
struct Proj {                                   // one projection's weights for the lane's 4 columns: loads and dequantisation
    const unsigned* qw;
    const unsigned* qz;
    const T* sc;
    int gcur;
    Scale4<T> s4;                         // the 4 columns' scales
    f16x2 k[4][4];                              // column c's constants -(2^m + z), shared by the widths: 4 bits k[c][0..1] (Deq1's c1, c2), 8 bits k[c][0],
                                                // 3 bits k[c][0..2] (Deq1_3's c0..c2), 2 bits k[c][0..3] (Deq1_2's c0..c3); the rest is never read

    __device__ __forceinline__ void group(const GemmArgs& p, int g, int n) {
        if (g == gcur) return;
        gcur = g;
        s4.setup(*(const u32x2*)(sc + (size_t)g * p.N + n));                  // 4 scales (8 bytes)
        const int zrow = p.N / 32 * p.bits;
        const unsigned bit = (unsigned)(p.bits * n), wi = bit >> 5, sh = bit & 31u;
        const unsigned* __restrict__ zr = qz + (size_t)g * zrow;
        unsigned zw = zr[wi] >> sh;                                           // 4 fields (n % 4 == 0): inside one word at 2, 4 and 8 bits
        if (sh + 4u * (unsigned)p.bits > 32u) zw |= zr[wi + 1] << (32u - sh); // 3 bits, n % 32 in {8, 20}: they straddle (never the last quad of a row: N % 64 == 0)
        const unsigned maxq = (1u << p.bits) - 1u;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            int zi = (int)((zw >> (p.bits * c)) & maxq) + 1;
            if (p.zero_mode == GPTQ_ZERO_WRAP) zi &= (int)maxq;
            const unsigned z = (unsigned)zi;
            k[c][0] = as_f16x2(z * 0x00010001u + 0xE400E400u);                // -(1024 + z): every width
            if (p.bits == 4) {
                const f16x2 k960 = {(f16)960.f, (f16)960.f};
                k[c][1] = k[c][0] + k960;                                     // -(64 + z)
            } else if (p.bits == 3) {
                k[c][1] = as_f16x2(z * 0x00080008u + 0xD800D800u);            // -(128 + z)
                k[c][2] = as_f16x2(z * 0x00400040u + 0xCC00CC00u);            // -(16 + z)
            } else if (p.bits == 2) {
                k[c][1] = as_f16x2(z * 0x00040004u + 0xDC00DC00u);            // -(256 + z)
                k[c][2] = as_f16x2(z * 0x00100010u + 0xD400D400u);            // -(64 + z)
                k[c][3] = as_f16x2(z * 0x00400040u + 0xCC00CC00u);            // -(16 + z)
            }
        }
    }
    // the lane's fields of one step: 4 bits one row of words (8 k each); 8 bits rows k0 / 4 + 2 ks, + 1; 3 bits the step's rows 3 st + lo, + hi that hold
    // bits 24 ks .. 24 ks + 23 of the columns' 96 (hi is clamped: k-slot 3 must not read the next step's row); 2 bits row 2 st + (ks >> 1)
    __device__ __forceinline__ void load(const GemmArgs& p, int k0, int ks, int n, u32x4& q0, u32x4& q1) const {
        if (p.bits == 4) {
            q0 = *(const u32x4*)(qw + (size_t)(k0 / 8 + ks) * p.N + n);
        } else if (p.bits == 8) {
            const size_t r = (size_t)(k0 / 4 + 2 * ks);
            q0 = *(const u32x4*)(qw + r * p.N + n);
            q1 = *(const u32x4*)(qw + (r + 1) * p.N + n);
        } else if (p.bits == 3) {
            const int lo = (24 * ks) >> 5, hi = min(lo + 1, 2);
            const size_t r = (size_t)(k0 / 32) * 3;
            q0 = *(const u32x4*)(qw + (r + lo) * p.N + n);
            q1 = *(const u32x4*)(qw + (r + hi) * p.N + n);
        } else {
            q0 = *(const u32x4*)(qw + (size_t)(k0 / 16 + (ks >> 1)) * p.N + n);
        }
    }
    __device__ __forceinline__ u32x4 frag(const GemmArgs& p, int c, int ks, const u32x4& q0, const u32x4& q1) const {
        f16x2 h0, h1, h2, h3;
        if (p.bits == 4) {                      // Deq1: (0,4) (1,5) (2,6) (3,7)
            const unsigned q = q0[c], q8 = q >> 8;
            const f16x2 r16 = {(f16)0.0625f, (f16)0.0625f};
            h0 = as_f16x2(and_or(q, 0x000f000fu, 0x64006400u)) + k[c][0];
            h1 = as_f16x2(and_or(q, 0x00f000f0u, 0x64006400u)) * r16 + k[c][1];
            h2 = as_f16x2(and_or(q8, 0x000f000fu, 0x64006400u)) + k[c][0];
            h3 = as_f16x2(and_or(q8, 0x00f000f0u, 0x64006400u)) * r16 + k[c][1];
        } else if (p.bits == 8) {               // Deq1_8: (0,2) (1,3) (4,6) (5,7)
            h0 = as_f16x2(and_or(q0[c], 0x00ff00ffu, 0x64006400u)) + k[c][0];
            h1 = as_f16x2(and_or(q0[c] >> 8, 0x00ff00ffu, 0x64006400u)) + k[c][0];
            h2 = as_f16x2(and_or(q1[c], 0x00ff00ffu, 0x64006400u)) + k[c][0];
            h3 = as_f16x2(and_or(q1[c] >> 8, 0x00ff00ffu, 0x64006400u)) + k[c][0];
        } else if (p.bits == 3) {               // the 24-bit window, fields 0..3 | 4..7 moved to bit 0 / 3 / 6 / 9 of the halves: Deq1_3's in-place readers
            const unsigned v = __builtin_amdgcn_alignbit(q1[c], q0[c], (unsigned)(24 * ks) & 31u) & 0xffffffu;
            const unsigned w = (v & 0xfffu) | ((v >> 12) << 16);
            Deq1_3<T> d;
            d.c0 = k[c][0]; d.c1 = k[c][1]; d.c2 = k[c][2];
            h0 = d.p0(w); h1 = d.p1(w); h2 = d.p2(w); h3 = d.p1(w >> 6);
        } else {                                // half ks & 1 of the word, its bytes moved to the halves: Deq1_2's readers
            const unsigned v = q0[c] >> (16 * (ks & 1));
            const unsigned w = (v & 0xffu) | ((v & 0xff00u) << 8);
            Deq1_2<T> d;
            d.c0 = k[c][0]; d.c1 = k[c][1]; d.c2 = k[c][2]; d.c3 = k[c][3];
            h0 = d.p0(w); h1 = d.p1(w); h2 = d.p2(w); h3 = d.p3(w);
        }
        return u32x4{s4.mul(h0, c), s4.mul(h1, c), s4.mul(h2, c), s4.mul(h3, c)};
    }
};

template <typename T>
__global__ void __launch_bounds__(THREADS) moe_gemm_kernel(GemmArgs p) {
    __shared__ __attribute__((aligned(16))) float red[4][MAX_ROWS][BN];          // 64 KiB: the waves' partial sums
    const int b = blockIdx.x;
    const int s = b % p.ksplit, rest = b / p.ksplit;
    const int cb = rest % p.nblk, tile = rest / p.nblk;
    if (tile >= *p.tile_count) return;
    const int4 tl = p.tiles[tile];
    const int e = tl.x, row0 = tl.y, rows = tl.z;
    const int rb = (rows + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ks = lane >> 4, cq = lane & 15;
    const int n0 = cb * BN, n = n0 + 4 * cq;
    const int K = p.K;

    const ExpertPtrs eg = p.table[e];
    const int* __restrict__ perm = eg.perm;
    const int* __restrict__ permu = nullptr;    // W3's own activation order when it differs from W1's (a checkpoint's gate / up share one)
    Proj<T> pg, pu;
    pg.qw = eg.qweight; pg.qz = eg.qzeros; pg.sc = (const T*)eg.scales; pg.gcur = -1;
    if (p.pair) {
        const ExpertPtrs eu = p.table[p.E + e];
        pu.qw = eu.qweight; pu.qz = eu.qzeros; pu.sc = (const T*)eu.scales; pu.gcur = -1;
        if (eu.perm != perm) permu = eu.perm;
    }
    const bool sep = p.pair && permu != nullptr;

    // the lane's A rows: row lane & 15 of each 16-row block (clamped to the tile's last row)
    const T* arow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = row0 + min(16 * i + (lane & 15), rows - 1);
        arow[i] = p.pair ? (const T*)p.a + (size_t)(p.row_assign[r] / p.topk) * K : (const T*)p.a + (size_t)r * K;
    }

    f32x4 ag[4][4], au[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) ag[i][c] = au[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int steps = K / 32;
    const int st0 = s * p.steps_per_split, st1 = min(steps, st0 + p.steps_per_split);
    for (int st = st0 + wave; st < st1; st += 4) {
        const int k0 = 32 * st;
        const int g = k0 / p.group_size;
        u32x4 qg0, qg1 = u32x4{0, 0, 0, 0}, qu0 = u32x4{0, 0, 0, 0}, qu1 = u32x4{0, 0, 0, 0};
        pg.load(p, k0, ks, n, qg0, qg1);
        if (p.pair) pu.load(p, k0, ks, n, qu0, qu1);
        u32x4 a[4], a3[4];
        const int kk = k0 + 8 * ks;
        auto gather = [&](const int* pm, const T* r) -> u32x4 {
            const int4 p0 = *(const int4*)(pm + kk), p1 = *(const int4*)(pm + kk + 4);
            const unsigned short h[8] = {__builtin_bit_cast(unsigned short, r[p0.x]), __builtin_bit_cast(unsigned short, r[p0.y]),
                                         __builtin_bit_cast(unsigned short, r[p0.z]), __builtin_bit_cast(unsigned short, r[p0.w]),
                                         __builtin_bit_cast(unsigned short, r[p1.x]), __builtin_bit_cast(unsigned short, r[p1.y]),
                                         __builtin_bit_cast(unsigned short, r[p1.z]), __builtin_bit_cast(unsigned short, r[p1.w])};
            return u32x4{h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16)};
        };
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < rb) {
                a[i] = order_a(perm ? gather(perm, arow[i]) : *(const u32x4*)(arow[i] + kk), p.bits);
                if (sep) a3[i] = order_a(gather(permu, arow[i]), p.bits);
            }
        }
        pg.group(p, g, n);
        if (p.pair) pu.group(p, g, n);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32x4 bg = pg.frag(p, c, ks, qg0, qg1);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < rb) ag[i][c] = Mma16<T>::run(a[i], bg, ag[i][c]);
            if (p.pair) {
                const u32x4 bu = pu.frag(p, c, ks, qu0, qu1);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < rb) au[i][c] = Mma16<T>::run(sep ? a3[i] : a[i], bu, au[i][c]);
            }
        }
    }

    // the waves meet in LDS; each thread sums 4-column pieces of the tile in wave order
    auto publish = [&](f32x4 (&acc)[4][4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= rb) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * i + 4 * (lane >> 4) + r;
                *(f32x4*)&red[wave][row][4 * cq] = f32x4{acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
            }
        }
    };
    constexpr int PIECES = MAX_ROWS * BN / 4 / THREADS;        // 4 pieces of 4 columns per thread
    f32x4 sg[PIECES];
    publish(ag);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < PIECES; ++m) {
        const int q = tid + THREADS * m, row = q >> 4, c4 = 4 * (q & 15);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row < rows) {
            v = *(const f32x4*)&red[0][row][c4];
            v += *(const f32x4*)&red[1][row][c4];
            v += *(const f32x4*)&red[2][row][c4];
            v += *(const f32x4*)&red[3][row][c4];
        }
        sg[m] = v;
    }
    if (!p.pair) {
        float* __restrict__ y = (float*)p.out + (size_t)s * p.rstride * p.N;
#pragma unroll
        for (int m = 0; m < PIECES; ++m) {
            const int q = tid + THREADS * m, row = q >> 4, c4 = 4 * (q & 15);
            if (row < rows) *(f32x4*)(y + (size_t)(row0 + row) * p.N + n0 + c4) = sg[m];
        }
        return;
    }
    __syncthreads();
    publish(au);
    __syncthreads();
    T* __restrict__ h = (T*)p.out;
#pragma unroll
    for (int m = 0; m < PIECES; ++m) {
        const int q = tid + THREADS * m, row = q >> 4, c4 = 4 * (q & 15);
        if (row >= rows) continue;
        f32x4 u = *(const f32x4*)&red[0][row][c4];
        u += *(const f32x4*)&red[1][row][c4];
        u += *(const f32x4*)&red[2][row][c4];
        u += *(const f32x4*)&red[3][row][c4];
        unsigned short o[4];
        if (p.pair == 2) {                      // the sums themselves, rounded once each
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = __builtin_bit_cast(unsigned short, DType<T>::from_f32(u[c]));
            *(u32x2*)((T*)p.out2 + (size_t)(row0 + row) * p.N + n0 + c4) = u32x2{o[0] | ((unsigned)o[1] << 16), o[2] | ((unsigned)o[3] << 16)};
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = __builtin_bit_cast(unsigned short, DType<T>::from_f32(sg[m][c]));
            *(u32x2*)(h + (size_t)(row0 + row) * p.N + n0 + c4) = u32x2{o[0] | ((unsigned)o[1] << 16), o[2] | ((unsigned)o[3] << 16)};
            continue;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float gv = sg[m][c];
            o[c] = __builtin_bit_cast(unsigned short, DType<T>::from_f32(gv / (1.f + __expf(-gv)) * u[c]));
        }
        *(u32x2*)(h + (size_t)(row0 + row) * p.N + n0 + c4) = u32x2{o[0] | ((unsigned)o[1] << 16), o[2] | ((unsigned)o[3] << 16)};
    }
}

struct CombineArgs {
    const int* pos;
    const float* w;
    const float* y;                             // [ksplit][rstride][H]
    void* out;                                  // [T][H]
    int T, topk, H, ksplit, rstride, dtype;
};

__global__ void __launch_bounds__(256) moe_combine_kernel(CombineArgs p) {
    const int quads = p.H / 4;
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long)p.T * quads) return;
    const int t = (int)(item / quads), c4 = 4 * (int)(item % quads);
    const size_t slice = (size_t)p.rstride * p.H;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < p.topk; ++j) {
        const int r = p.pos[t * p.topk + j];
        if (r < 0) continue;
        const float* yr = p.y + (size_t)r * p.H + c4;
        f32x4 v = *(const f32x4*)yr;
        for (int s = 1; s < p.ksplit; ++s) v += *(const f32x4*)(yr + s * slice);
        acc += p.w[t * p.topk + j] * v;
    }
    unsigned short o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        o[c] = p.dtype == GPTQ_F16 ? __builtin_bit_cast(unsigned short, DType<f16>::from_f32(acc[c]))
                                   : __builtin_bit_cast(unsigned short, DType<bf16>::from_f32(acc[c]));
    *(u32x2*)((unsigned short*)p.out + (size_t)t * p.H + c4) = u32x2{o[0] | ((unsigned)o[1] << 16), o[2] | ((unsigned)o[3] << 16)};
}

}  // namespace moe

MoePlan plan_moe(int E, int T, int topk, int H, int I, int dtype) {
    MoePlan pl{};
    const long R = (long)T * topk;
    const long hit = std::min<long>(E, R);
    const long avg = hit > 0 ? (R + hit - 1) / hit : 0;          // rows per hit expert when the routing is even
    pl.bm = avg <= 16 ? 16 : avg <= 32 ? 32 : 64;
    pl.bn = moe::BN;
    pl.tiles = (int)(R / pl.bm + hit);
    // K slices of the down projection: only while its tiles x column blocks stay under two workgroups per CU, and each slice keeps >= 8 steps per wave
    const long wg2 = (long)pl.tiles * (H / moe::BN);
    const int steps = I / 32;
    pl.ksplit = 1;
    while (wg2 * pl.ksplit * 2 <= 512 && pl.ksplit < 8 && steps / (pl.ksplit * 2) >= 32) pl.ksplit *= 2;
    pl.steps_per_split = (steps + pl.ksplit - 1) / pl.ksplit;
    const size_t es = dtype_size(dtype);
    size_t o = append_route_layout(pl, GPTQ_WORKSPACE_HEADER_BYTES, E, pl.tiles, R);      // the header of a shared workspace belongs to the other entry points: left as it is
    pl.off_h = o; o += align256((size_t)R * I * es);
    pl.off_y = o; o += align256((size_t)pl.ksplit * R * H * 4);
    pl.bytes = o;
    return pl;
}

// host-side launch helpers of the routing and the combine kernel (moe_rows.hip launches them around its own GEMMs)
hipError_t launch_moe_route(const int64_t* idx, int T, int topk, int E, int bm, int* offsets, int* tile_count, void* tiles, int* pos, int* row_assign,
                            hipStream_t st) {
    moe::RouteArgs ra;
    ra.idx = (const long long*)idx;
    ra.T = T; ra.topk = topk; ra.E = E; ra.bm = bm;
    ra.offsets = offsets;
    ra.tile_count = tile_count;
    ra.tiles = (int4*)tiles;
    ra.pos = pos;
    ra.row_assign = row_assign;
    hipLaunchKernelGGL(moe::moe_route_kernel, dim3(1), dim3(moe::ROUTE_THREADS), 0, st, ra);
    return hipGetLastError();
}

hipError_t launch_moe_combine(const int* pos, const float* w, const float* y, void* out, int T, int topk, int H, int ksplit, int rstride, int dtype,
                              hipStream_t st) {
    moe::CombineArgs c;
    c.pos = pos; c.w = w; c.y = y; c.out = out;
    c.T = T; c.topk = topk; c.H = H; c.ksplit = ksplit; c.rstride = rstride; c.dtype = dtype;
    const long items = (long)T * (H / 4);
    hipLaunchKernelGGL(moe::moe_combine_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, c);
    return hipGetLastError();
}

hipError_t launch_moe(const gptq_moe_t& m, const void* table, const MoePlan& pl, const void* x, const int64_t* idx, const float* w, int T, int topk,
                      void* out, char* ws, hipStream_t st) {
    const gptq_layer_t& G = *m.gate[0];
    const gptq_layer_t& D = *m.down[0];
    const int E = m.E, H = G.K, I = G.N;
    const int R = T * topk;
    int* const tile_count = (int*)(ws + pl.off_tile_count);
    int4* const tiles = (int4*)(ws + pl.off_tiles);
    int* const pos = (int*)(ws + pl.off_pos);
    int* const row_assign = (int*)(ws + pl.off_rows);
    hipError_t e = launch_moe_route(idx, T, topk, E, pl.bm, (int*)(ws + pl.off_offsets), tile_count, tiles, pos, row_assign, st);
    if (e != hipSuccess) return e;

    moe::GemmArgs g;
    g.table = (const moe::ExpertPtrs*)table;
    g.E = E; g.pair = 1; g.a = x; g.row_assign = row_assign; g.topk = topk;
    g.tile_count = tile_count; g.tiles = tiles;
    g.K = H; g.N = I; g.bits = G.bits; g.group_size = G.group_size; g.zero_mode = G.zero_mode;
    g.nblk = I / moe::BN; g.ksplit = 1; g.steps_per_split = H / 32;
    g.out = ws + pl.off_h; g.rstride = R; g.out2 = nullptr;
    auto gemm = [&](const moe::GemmArgs& a, long blocks) -> hipError_t {
        if (blocks <= 0) return hipSuccess;
        if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
        if (G.dtype == GPTQ_F16) hipLaunchKernelGGL(moe::moe_gemm_kernel<f16>, dim3((unsigned)blocks), dim3(moe::THREADS), 0, st, a);
        else hipLaunchKernelGGL(moe::moe_gemm_kernel<bf16>, dim3((unsigned)blocks), dim3(moe::THREADS), 0, st, a);
        return hipGetLastError();
    };
    if ((e = gemm(g, (long)pl.tiles * g.nblk)) != hipSuccess) return e;

    moe::GemmArgs d = g;
    d.table = (const moe::ExpertPtrs*)table + 2 * (size_t)E;
    d.pair = 0; d.a = ws + pl.off_h;
    d.K = I; d.N = H; d.bits = D.bits; d.group_size = D.group_size; d.zero_mode = D.zero_mode;
    d.nblk = H / moe::BN; d.ksplit = pl.ksplit; d.steps_per_split = pl.steps_per_split;
    d.out = ws + pl.off_y;
    if ((e = gemm(d, (long)pl.tiles * d.nblk * d.ksplit)) != hipSuccess) return e;

    return launch_moe_combine(pos, w, (const float*)(ws + pl.off_y), out, T, topk, H, pl.ksplit, R, G.dtype, st);
}

hipError_t launch_moe_recompute(const gptq_moe_t& m, const void* table, const void* x, const int* row_assign, const int* tile_count, const void* tiles,
                                int tiles_bound, int T, int topk, void* g_out, void* u_out, hipStream_t st) {
    const gptq_layer_t& G = *m.gate[0];
    moe::GemmArgs g;
    g.table = (const moe::ExpertPtrs*)table;
    g.E = m.E; g.pair = 2; g.a = x; g.row_assign = row_assign; g.topk = topk;
    g.tile_count = tile_count; g.tiles = (const int4*)tiles;
    g.K = G.K; g.N = G.N; g.bits = G.bits; g.group_size = G.group_size; g.zero_mode = G.zero_mode;
    g.nblk = G.N / moe::BN; g.ksplit = 1; g.steps_per_split = G.K / 32;
    g.out = g_out; g.rstride = T * topk; g.out2 = u_out;
    const long blocks = (long)tiles_bound * g.nblk;
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    if (G.dtype == GPTQ_F16) hipLaunchKernelGGL(moe::moe_gemm_kernel<f16>, dim3((unsigned)blocks), dim3(moe::THREADS), 0, st, g);
    else hipLaunchKernelGGL(moe::moe_gemm_kernel<bf16>, dim3((unsigned)blocks), dim3(moe::THREADS), 0, st, g);
    return hipGetLastError();
}

size_t moe_table_entry_bytes() { return sizeof(moe::ExpertPtrs); }

void moe_table_entry(const gptq_layer_t& L, void* dst) {
    moe::ExpertPtrs p;
    p.qweight = L.qweight_seq ? L.qweight_seq : L.qweight;
    p.qzeros = L.qzeros;
    p.scales = L.scales;
    p.perm = L.qweight_seq ? L.perm : nullptr;
    memcpy(dst, &p, sizeof(p));
}

}  // namespace gptq
