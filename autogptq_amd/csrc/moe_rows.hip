// moe_rows.hip -- routed mixture-of-experts layers at batched-decode row counts (gptq_moe_batch_forward): 5..64 tokens on the experts' DECODE COPY.
//
// What one call computes: the formulas and the ARITHMETIC CONTRACT of the grouped path (moe.hip): every W bit-exact to gptq_dequant, products and sums in fp32
// on the matrix core, h rounded once, out[t] = T(sum_j w[t, j] * y_(t, j)) in ascending j with one rounding; assignments outside [0, E) are dropped.
// Four launches, no host round trip (capturable):
//   1. moe_route_kernel (moe.hip) with bm = 16: sorted rows, pos, row_assign and the tile table (expert, first row, rows <= 16) with its count.
//   2. moe_rows_kernel<T, BITS>, pair form: a workgroup = one tile x 2 adjacent 16-column strips of W1_e AND the same 2 strips of W3_e x the whole K;
//      silu * mul on the fp32 sums -> H_sorted [R][I] in T.
//   3. moe_rows_kernel<T, BITS>, down form: a workgroup = one tile x 4 adjacent strips of W2_e x the whole K -> Y [R][H] fp32.
//   4. moe_combine_kernel (moe.hip), one slice.
// The grid is the bound tiles <= floor(T topk / 16) + min(E, T topk) times the strip groups; workgroups past the tile count the routing kernel wrote return
// at once (the strip group is the fast index: they are the end of the grid).
//
// moe_rows_kernel is the dense rows kernel (gemm_rows_kernel.cuh, RB = 1) with the expert, the rows and the strips looked up per workgroup.  The waves split
// the 128-deep chunks of K into contiguous ranges and meet once in LDS, in wave order.  Per chunk a wave
//   * loads NS = 4 strip-chunks of the copy (1 KiB each at 4 bits, two 64-deep halves at 8; lane = 32 consecutive k of one column) and their constants
//     (qconst_tiled records) from the expert's entries of the decode table: inline-asm loads behind hand-counted s_waitcnt vmcnt, a ring of DW chunks in flight;
//   * stages its 16 rows x 128 k of the A operand by LDS DMA into wave-private double buffers (no barrier in the K loop).  The DMA's per-lane global address
//     gathers the rows: row r of the tile is x[row_assign[first + r] / topk] (pair form) or H_sorted[first + r] (down form); the XOR swizzle against the
//     256-byte row pitch is applied on the global side, as in the rows kernel.  Rows past the tile's count repeat its last row and are not stored;
//   * dequantises with Deq1 / Deq1_8 (bit-exact W, one rounding) and runs v_mfma_f32_16x16x32_{f16,bf16} (Mma16).
// No K slices, no atomics: every output is one fixed-order sum -- bit-reproducible, and a token's row depends only on that token's x, indices and weights
// (the fp32 sum of a row does not depend on which other rows share its tile: the MFMA rows are independent).
// The pair / down form, the group mode and the number of staged planes are run-time uniform: T x BITS = four instantiations.
//
// 2- AND 3-BIT EXPERTS (opt-in: GPTQ_MOE_LOW_BIT_BATCH in gptq_moe_t.flags): moe_rows_lowbit_kernel<T, 2 | 3>, the same body (moe_rows_body.inc, included
// into both kernel templates) with three template constants: the strip-chunk of the copy is 768 / 512 bytes instead of 1024, a lane's share 12 / 8 bytes
// instead of 16, fetched by ONE global_load_dwordx3 / dwordx2 into a ring element of that size, and dequantised in place by Deq1_3::frag(words, ks) /
// Deq1_2::frag(word[ks >> 1] >> 8 (ks & 1)) -- MFMA step ks gets the lane's k = 8 ks .. 8 ks + 7 in the order the A operand has them, as at 4 bits.
// The constant record (48 bytes, one-byte zero-point), the group offsets, the x side, the ring depth, the loads per chunk (3 NS: the vmcnt counts) and the
// reduction are the 4-bit form's.  Four more instantiations under a name of their own, so that "moe_rows_kernel" keeps meaning the 4- / 8-bit forms, whose
// code objects are instruction for instruction what they were.  Registers (read off the code object): 124 (fp16) / 125 (bf16) VGPRs at both widths, no
// scratch, no spill: the 4-bit form's 128-register compilation, two workgroups per CU.
//
// ACT-ORDER experts (the copy is made of the re-sequenced rows): one small untyped 2-byte gather pre-pass, moe_gather_rows_kernel,
// rows_out[r][i] = rows_in[src(r)][perm_e(r)[i]], runs before the pair stage (x through W1_e's perm into plane 0 and through W3_e's perm into plane 1 -- gate
// and up of an expert may have different activation orders; the pair form then stages BOTH planes, W1's strips multiply plane 0 and W3's plane 1) and again
// between the stages (H_sorted through W2_e's perm): six launches.  Plain experts do not pay for it.  Built instead of an LDS -> LDS gather inside the K loop
// because a chunk's 128 positions of perm point anywhere in the row: the wave would have to stage whole rows (16 x K x 2 bytes: 448 KiB at K = 14336), not
// chunks, which is what the decode kernel does for ONE row and does not scale to 16.
//
// GEOMETRY (cost model in the style of plan_rows).  Per chunk and strip a workgroup pulls 1 KiB of weights (HBM) and, per chunk, 4 KiB of rows (L2); with NS
// strips behind one staged chunk the row traffic is 4 / NS KiB per KiB of weights.  NS = 4: a workgroup pulls 2x its weight bytes in all; at the measured
// 105 - 125 GB/s per CU the 256 CUs pull ~14 TB/s of weights, above the 8 TB/s HBM gives, so the row pulls hide.  NS = 2 would halve the headroom below HBM
// speed; NS = 8 needs 8 x 4 (x 2 at 8 bits) registers per ring slot x DW slots plus 8 accumulators: past 128 VGPRs, and half the workgroups.
// Dequant issue: 13 VALU per 8 weights = 208 per lane and chunk at NS = 4 against 16 MFMAs (8 passes each): ~340 cycles per chunk and wave, 4 KiB per
// 340 cycles and wave; a CU needs 16 waves (2 workgroups of 8) for 105 GB/s at 2.4 GHz -- 8 waves x 8 KiB of x buffers = 64 KiB of LDS, two workgroups
// per CU (act-order pair form: two planes, 128 KiB, one workgroup).  Waves: min(8, chunks / 2) so that every wave runs at least two chunks behind its ring.
// Pair form: both projections in every wave (2 + 2 strips behind the same staged chunk) rather than half the waves each: the halves would stage the same
// rows twice.  Rounds: +~2 us per round of 256 workgroups x 2; Mixtral at T = 16 (<= 10 tiles): pair 10 x 448 = 4480 workgroups of 128 KiB, down 10 x 64 =
// 640 of 448 KiB.
#include <string.h>

#include <algorithm>

#include "common.cuh"
#include "launch.h"
#include "mma_dequant.cuh"           // DeqSel: Deq1<T> / Deq1_8<T> / Deq1_3<T>, Deq1_2<T>; Mma16<T>
#include "moe_entry.cuh"             // moerows::Entry, load_entry

namespace gptq {
namespace moerows {

constexpr int NS = 4;                           // strip-chunks per wave and chunk (pair: 2 of W1 + 2 of W3; down: 4 of W2)
constexpr int MAX_WAVES = 8;
constexpr int BM = 16;
constexpr int XB = 4096;                        // 16 rows x 128 k x 2 bytes
constexpr int MAX_LDS = 160 * 1024;

// The dense form (pair == 2, 2 bits only) reads no table: the four fields that describe the tables carry the layer instead (the second name of each union; the
// layout, and with it the 3- / 4- / 8-bit kernels' argument block, is what it was)
struct Args {
    union { const Entry* table;                 // entries of the first projection (pair: W1; W3 is table + E)
            const unsigned* dense_tq; };        // dense: the layer's qweight_tiled
    union { int E; int dense_M; };              // dense: rows of x / out
    int pair;                                   // 0: down, 1: pair, 2: dense (moe_rows_lowbit_kernel<T, 2> only)
    const void* a;                              // rows of the A operand [.][K]; planes > 1: plane q at a + q * plane_bytes
    size_t plane_bytes;
    const int* row_assign;                      // non-NULL: row r of the tile is a[row_assign[first + r] / topk]; NULL: a[first + r]
    int topk, planes;
    union { const int* tile_count; const void* dense_bias; };      // dense: bias [N] (T) or NULL
    union { const int4* tiles; const void* dense_cst; };           // dense: the layer's qconst_tiled
    int K, N, chunks, groups, gshift, gm, cpw, nsg;
    void* out;                                  // pair: H_sorted [R][N] (T); down: Y [R][N] fp32; dense: out [M][N] (T)
};

// 2 / 3 bits (opt-in: GPTQ_MOE_LOW_BIT_BATCH): the copy of utils.hip prepack_decode_weights_kernel read in place -- Deq1_3::frag(words, ks) as the dense rows
// kernel does, Deq1_2::frag(word[ks >> 1] >> 8 (ks & 1)): pair p = (k 16 w + 2 p, + 1) sits at bit 2 p of the halves of word w, so fields 0..3 of the
// (shifted) word are k = 8 ks .. 8 ks + 7 of the lane's 32 in the order the A operand has them
template <typename T, int BITS> struct DeqOf { typedef typename DeqSel<T, BITS>::type type; };
template <typename T> struct DeqOf<T, 2> { typedef Deq1_2<T> type; };

// 2 / 3 / 4 bits: compiled for 128 registers (two 8-wave workgroups per CU); 8 bits: a ring slot is twice as large -- 256 registers, one workgroup per CU
template <typename T, int BITS>
__global__ void __launch_bounds__(BITS == 8 ? 512 : 1024) moe_rows_kernel(Args p) {
    static_assert(BITS == 4 || BITS == 8, "2 and 3 bits: moe_rows_lowbit_kernel");
#include "moe_rows_body.inc"
}
// the opt-in widths under a name of their own: what counts or lints "moe_rows_kernel" keeps meaning the 4- and 8-bit forms
template <typename T, int BITS>
__global__ void __launch_bounds__(1024) moe_rows_lowbit_kernel(Args p) {
    static_assert(BITS == 2 || BITS == 3, "4 and 8 bits: moe_rows_kernel");
#include "moe_rows_body.inc"
}

// act-order pre-pass, untyped 2-byte elements: out[plane][r][i] = in[src(r)][perm[i]], perm = that of expert e(r)'s entry of projection (first + plane);
// src(r) = row_assign[r] / topk (topk > 0: the token's row of x) or r (topk = 0: H_sorted).  A thread = one 16-byte piece.  Entries without a perm: a copy.
struct GatherArgs {
    const Entry* table;
    const long long* idx;
    const int* row_assign;
    const int* offsets;                         // [E + 1]: offsets[E] = sorted rows in use
    const unsigned short* in;
    unsigned short* out;                        // [planes][R][K]
    int E, topk, K, R;
};

__global__ void __launch_bounds__(256) moe_gather_rows_kernel(GatherArgs p) {
    const int r = blockIdx.y, plane = blockIdx.z;
    if (r >= p.offsets[p.E]) return;
    const int piece = blockIdx.x * 256 + threadIdx.x;
    if (piece >= (p.K >> 3)) return;
    const int a = p.row_assign[r];
    const int e = (int)p.idx[a];                               // a sorted row in use belongs to a valid expert
    const int* __restrict__ perm = p.table[(size_t)plane * p.E + e].perm;
    const unsigned short* __restrict__ src = p.in + (size_t)(p.topk ? a / p.topk : r) * p.K;
    u32x4 o;
    if (perm) {
        const int4 pa = *(const int4*)(perm + piece * 8), pb = *(const int4*)(perm + piece * 8 + 4);
        o[0] = (unsigned)src[pa.x] | ((unsigned)src[pa.y] << 16);
        o[1] = (unsigned)src[pa.z] | ((unsigned)src[pa.w] << 16);
        o[2] = (unsigned)src[pb.x] | ((unsigned)src[pb.y] << 16);
        o[3] = (unsigned)src[pb.z] | ((unsigned)src[pb.w] << 16);
    } else {
        o = *(const u32x4*)(src + piece * 8);
    }
    *(u32x4*)(p.out + ((size_t)plane * p.R + r) * p.K + piece * 8) = o;
}

template <typename T, int BITS>
static hipError_t launch_one(const Args& a, long blocks, int waves, int lds, hipStream_t st) {
    if constexpr (BITS == 2 || BITS == 3) hipLaunchKernelGGL((moe_rows_lowbit_kernel<T, BITS>), dim3((unsigned)blocks), dim3(waves * 64), lds, st, a);
    else hipLaunchKernelGGL((moe_rows_kernel<T, BITS>), dim3((unsigned)blocks), dim3(waves * 64), lds, st, a);
    return hipGetLastError();
}
static hipError_t launch_any(int dtype, int bits, const Args& a, long blocks, int waves, int lds, hipStream_t st) {
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    if (dtype != GPTQ_F16 && dtype != GPTQ_BF16) return hipErrorInvalidValue;
    const bool h = dtype == GPTQ_F16;
    switch (bits) {
        case 2: return h ? launch_one<f16, 2>(a, blocks, waves, lds, st) : launch_one<bf16, 2>(a, blocks, waves, lds, st);
        case 3: return h ? launch_one<f16, 3>(a, blocks, waves, lds, st) : launch_one<bf16, 3>(a, blocks, waves, lds, st);
        case 4: return h ? launch_one<f16, 4>(a, blocks, waves, lds, st) : launch_one<bf16, 4>(a, blocks, waves, lds, st);
        case 8: return h ? launch_one<f16, 8>(a, blocks, waves, lds, st) : launch_one<bf16, 8>(a, blocks, waves, lds, st);
    }
    return hipErrorInvalidValue;                                // (the entry point's check lets no other width through)
}

static int group_mode(const gptq_layer_t& L) {                  // what the rows family takes: 0 = 128 2^n or one group, 1 = 64, 2 = 32
    if (L.group_size >= 128) {
        if (L.group_size >= L.K) return 0;
        const int q = L.group_size / 128;
        return (L.group_size % 128 == 0 && (q & (q - 1)) == 0) ? 0 : -1;
    }
    return L.group_size == 64 ? 1 : (L.group_size == 32 ? 2 : -1);
}

}  // namespace moerows

bool moe_batch_group_ok(const gptq_layer_t& L) { return moerows::group_mode(L) >= 0; }

MoeBatchPlan plan_moe_batch(const gptq_moe_t& m, int T, int topk) {
    MoeBatchPlan pl{};
    const gptq_layer_t& G = *m.gate[0];
    const int E = m.E, H = G.K, I = G.N;
    const long R = (long)T * topk;
    pl.bm = moerows::BM;
    pl.s = moerows::NS;
    pl.tiles = (int)(R / moerows::BM + std::min<long>(E, R));
    pl.act_pair = any_perm_of(m.gate, E) || any_perm_of(m.up, E);
    pl.act_down = any_perm_of(m.down, E);
    auto waves_for = [](int K) { return std::max(1, std::min(moerows::MAX_WAVES, K / 128 / 2)); };
    pl.waves_pair = waves_for(H);
    pl.waves_down = waves_for(I);
    pl.cpw_pair = (H / 128 + pl.waves_pair - 1) / pl.waves_pair;
    pl.cpw_down = (I / 128 + pl.waves_down - 1) / pl.waves_down;
    pl.waves_pair = (H / 128 + pl.cpw_pair - 1) / pl.cpw_pair;      // no wave without a chunk
    pl.waves_down = (I / 128 + pl.cpw_down - 1) / pl.cpw_down;
    pl.lds_pair = pl.waves_pair * 2 * (pl.act_pair ? 2 : 1) * moerows::XB;      // >= the waves' sums (waves x NS x 1 KiB)
    pl.lds_down = pl.waves_down * 2 * moerows::XB;
    pl.launches = T > 0 ? 4 + (pl.act_pair ? 1 : 0) + (pl.act_down ? 1 : 0) : 0;
    const size_t es = dtype_size(G.dtype);
    size_t o = append_route_layout(pl, GPTQ_WORKSPACE_HEADER_BYTES, E, pl.tiles, R);      // the header of a shared workspace belongs to the other entry points: left as it is
    pl.off_h = o; o += align256((size_t)R * I * es);
    pl.off_y = o; o += align256((size_t)R * H * 4);
    pl.off_xg = o; o += align256(2 * (size_t)R * H * es);            // act-order: x through W1's / W3's perm (two planes)
    pl.off_hg = o; o += align256((size_t)R * I * es);                // act-order: H_sorted through W2's perm
    pl.bytes = o;
    return pl;
}

hipError_t launch_moe_gather_rows(const void* table, int planes, int topk, const int64_t* idx, const int* row_assign, const int* offsets, const void* in,
                                  void* out, int E, int K, int R, hipStream_t st) {
    moerows::GatherArgs ga;
    ga.table = (const moerows::Entry*)table; ga.idx = (const long long*)idx; ga.row_assign = row_assign; ga.offsets = offsets;
    ga.in = (const unsigned short*)in; ga.out = (unsigned short*)out;
    ga.E = E; ga.topk = topk; ga.K = K; ga.R = R;
    hipLaunchKernelGGL(moerows::moe_gather_rows_kernel, dim3((K / 8 + 255) / 256, R, planes), dim3(256), 0, st, ga);
    return hipGetLastError();
}

hipError_t launch_moe_batch(const gptq_moe_t& m, const void* table, const MoeBatchPlan& pl, const void* x, const int64_t* idx, const float* w, int T, int topk,
                            void* out, char* ws, hipStream_t st) {
    const gptq_layer_t& G = *m.gate[0];
    const gptq_layer_t& D = *m.down[0];
    const int E = m.E, H = G.K, I = G.N;
    const int R = T * topk;
    int* const offsets = (int*)(ws + pl.off_offsets);
    int* const tile_count = (int*)(ws + pl.off_tile_count);
    int* const pos = (int*)(ws + pl.off_pos);
    int* const row_assign = (int*)(ws + pl.off_rows);
    hipError_t e = launch_moe_route(idx, T, topk, E, pl.bm, offsets, tile_count, ws + pl.off_tiles, pos, row_assign, st);
    if (e != hipSuccess) return e;

    const moerows::Entry* const tab = (const moerows::Entry*)table;
    auto gather = [&](const moerows::Entry* t, int planes, int tk, const void* in, void* o, int K) -> hipError_t {
        return launch_moe_gather_rows(t, planes, tk, idx, row_assign, offsets, in, o, E, K, R, st);
    };
    auto fill = [&](moerows::Args& a, const gptq_layer_t& L, int cpw, int s) {
        a.E = E; a.topk = topk;
        a.tile_count = tile_count; a.tiles = (const int4*)(ws + pl.off_tiles);
        a.K = L.K; a.N = L.N; a.chunks = L.K / 128;
        a.groups = (L.K + L.group_size - 1) / L.group_size;
        a.gshift = 31;
        if (L.group_size >= 128 && L.group_size < L.K) a.gshift = __builtin_ctz((unsigned)(L.group_size / 128));
        a.gm = moerows::group_mode(L);
        a.cpw = cpw; a.nsg = L.N / 16 / s;
    };

    moerows::Args g{};
    g.table = tab; g.pair = 1;
    if (pl.act_pair) {
        if ((e = gather(tab, 2, topk, x, ws + pl.off_xg, H)) != hipSuccess) return e;
        g.a = ws + pl.off_xg; g.plane_bytes = (size_t)R * H * 2; g.row_assign = nullptr; g.planes = 2;
    } else {
        g.a = x; g.plane_bytes = 0; g.row_assign = row_assign; g.planes = 1;
    }
    g.out = ws + pl.off_h;
    fill(g, G, pl.cpw_pair, moerows::NS / 2);
    if ((e = moerows::launch_any(G.dtype, G.bits, g, (long)pl.tiles * g.nsg, pl.waves_pair, pl.lds_pair, st)) != hipSuccess) return e;

    moerows::Args d{};
    d.table = tab + 2 * (size_t)E; d.pair = 0;
    if (pl.act_down) {
        if ((e = gather(tab + 2 * (size_t)E, 1, 0, ws + pl.off_h, ws + pl.off_hg, I)) != hipSuccess) return e;
        d.a = ws + pl.off_hg;
    } else {
        d.a = ws + pl.off_h;
    }
    d.plane_bytes = 0; d.row_assign = nullptr; d.planes = 1;
    d.out = ws + pl.off_y;
    fill(d, D, pl.cpw_down, moerows::NS);
    if ((e = moerows::launch_any(D.dtype, D.bits, d, (long)pl.tiles * d.nsg, pl.waves_down, pl.lds_down, st)) != hipSuccess) return e;

    return launch_moe_combine(pos, w, (const float*)(ws + pl.off_y), out, T, topk, H, 1, R, G.dtype, st);
}

// ---- the dense form (one flagged 2-bit QuantLinear layer; moe_rows_body.inc) ---------------------------------------------------------------------
// What the down form takes: fp16 / bf16, K a whole number of 128-deep chunks, N a whole number of NS-strip groups, a group size of the rows family; 32-bit x
// offsets per lane (gemm_rows.hip); act-order layers with their re-sequenced rows (the copy is made of them; the caller permutes x)
bool dense_rows_int2_ok(const gptq_layer_t& L, int M) {
    if (!copy_rows_int2(L) || (L.dtype != GPTQ_F16 && L.dtype != GPTQ_BF16) || L.epilogue != GPTQ_EPI_NONE) return false;
    if (L.g_idx != nullptr && !(L.perm && L.qweight_seq)) return false;
    if (L.K % 128 || L.N % (16 * moerows::NS) || moerows::group_mode(L) < 0) return false;
    if ((size_t)M * L.K * 2 >= ((size_t)1 << 32)) return false;
    return M >= 1 && M <= 1024;
}

RowsPlan plan_dense_rows_int2(const gptq_layer_t& L, int M) {
    RowsPlan pl{};
    if (!dense_rows_int2_ok(L, M)) return pl;
    const int chunks = L.K / 128;
    pl.rb = 1; pl.s = moerows::NS; pl.xbufs = 2;
    pl.waves = std::max(1, std::min(moerows::MAX_WAVES, chunks / 2));      // plan_moe_batch's: every wave runs at least two chunks behind its ring
    pl.cpw = (chunks + pl.waves - 1) / pl.waves;
    pl.waves = (chunks + pl.cpw - 1) / pl.cpw;                             // no wave without a chunk
    pl.npm = (M + moerows::BM - 1) / moerows::BM;
    pl.nsg = L.N / (16 * moerows::NS);
    pl.lds_bytes = (size_t)pl.waves * 2 * moerows::XB;                     // >= the waves' sums (waves x NS x 1 KiB)
    pl.ok = true;
    return pl;
}

hipError_t launch_dense_rows_int2(const gptq_layer_t& L, const void* x, void* out, int M, const RowsPlan& pl, hipStream_t st) {
    if (!pl.ok || !dense_rows_int2_ok(L, M)) return hipErrorInvalidValue;
    moerows::Args a{};
    a.dense_tq = L.qweight_tiled; a.dense_cst = L.qconst_tiled; a.dense_bias = L.bias; a.dense_M = M;
    a.pair = 2;
    a.a = x; a.plane_bytes = 0; a.row_assign = nullptr; a.topk = 1; a.planes = 1;
    a.K = L.K; a.N = L.N; a.chunks = L.K / 128;
    a.groups = (L.K + L.group_size - 1) / L.group_size;
    a.gshift = 31;
    if (L.group_size >= 128 && L.group_size < L.K) a.gshift = __builtin_ctz((unsigned)(L.group_size / 128));
    a.gm = moerows::group_mode(L);
    a.cpw = pl.cpw; a.nsg = pl.nsg;
    a.out = out;
    return moerows::launch_any(L.dtype, 2, a, (long)pl.npm * pl.nsg, pl.waves, (int)pl.lds_bytes, st);
}

// grants > 64 KiB of dynamic LDS (act-order pair form: two planes of x buffers)
hipError_t init_moe_batch_device() {
    hipError_t e = hipSuccess;
    auto grant = [&](auto kern) { hipError_t r = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, moerows::MAX_LDS); if (e == hipSuccess) e = r; };
    grant(moerows::moe_rows_kernel<f16, 4>); grant(moerows::moe_rows_kernel<f16, 8>);
    grant(moerows::moe_rows_kernel<bf16, 4>); grant(moerows::moe_rows_kernel<bf16, 8>);
    grant(moerows::moe_rows_lowbit_kernel<f16, 3>); grant(moerows::moe_rows_lowbit_kernel<f16, 2>);
    grant(moerows::moe_rows_lowbit_kernel<bf16, 3>); grant(moerows::moe_rows_lowbit_kernel<bf16, 2>);
    return e;
}

}  // namespace gptq
