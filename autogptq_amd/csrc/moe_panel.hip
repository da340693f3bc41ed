// moe_panel.hip -- routed mixture-of-experts layers at prompt row counts (gptq_moe_prefill_forward): any T, used above 64 tokens, on the experts' DECODE COPY.
//
// What one call computes: the formulas and the ARITHMETIC CONTRACT of the grouped path (moe.hip): every W bit-exact to gptq_dequant, products and sums in fp32
// on the matrix core, h rounded once, out[t] = T(sum_j w[t, j] * y_(t, j)) in ascending j with one rounding; assignments outside [0, E) are dropped.
// Five launches, no host round trip (capturable):
//   1. moe_route_kernel (moe.hip) with bm = 64: sorted rows, pos, row_assign and the tile table (expert, first row, rows <= 64) with its count.
//   2. moe_gather_rows_kernel (moe_rows.hip): x into sorted order, x_sorted [R][H].  Plain experts: its copy form, one plane; act-order experts: two planes,
//      through W1_e's and W3_e's perm (the copy is made of the re-sequenced rows), as on the batch path.
//   3. moe_panel_kernel<T, BITS>, pair form: a workgroup = one tile x NT / 2 adjacent 32-column blocks of W1_e AND the same blocks of W3_e x the whole K;
//      silu * mul on the fp32 sums -> H_sorted [R][I] in T.
//   4. (act-order down projections only: moe_gather_rows_kernel, H_sorted through W2_e's perm.)
//   5. moe_panel_kernel<T, BITS>, down form: a workgroup = one tile x NT blocks of W2_e x the whole K -> Y [R][H] fp32.
//   6. moe_combine_kernel (moe.hip), one slice.
// The grid is the bound tiles <= floor(T topk / 64) + min(E, T topk) times the column tiles; workgroups past the tile count the routing kernel wrote return
// at once (the column tile is the fast index: they are the end of the grid).
//
// moe_panel_kernel is the dense panel body (gemm_panel_kernel.cuh: MT = 2, its PART form) with the expert and the rows looked up per workgroup: 64 rows x
// 32 NT columns x the WHOLE K, the waves are K parts with wave-private x buffers (no barrier in the K loop) that meet once in LDS, in wave order;
// v_mfma_f32_32x32x16.  NT is a constant per packing (4 at 4 bits, 2 at 8 bits: a ring slot is twice as large), the ring holds DW = 2 (4 bits) or 3 (8 bits) steps of weights.
// The sorted copy of x (launch 2) costs R H 4 bytes of traffic against a GEMM of milliseconds and keeps the panel body's staging: a contiguous row pitch,
// 8 rows per DMA, no per-lane row offsets in a kernel that lives in 256 registers.  A tile's rows past its count repeat its last row (the PART clamp: DMA i
// fetches rows 8 min(i, imax) + min(r8, rlast)), so every load stays inside the tile -- also in the last tile of the buffer -- and they are never stored.
//
// ROW INDEPENDENCE.  The K split is a function of the layer alone: 8 waves (act-order pair form: 4 waves -- two planes of x buffers are 32 KiB per wave),
// steps per wave = ceil(K / 64 / waves); waves past the last step add zeros.  Nothing depends on T or on the tile a row lands in, and the rows of an MFMA
// are independent: a token's output bits depend only on its own x, indices and weights.  No K slices, no atomics: bit-reproducible.
// The pair / down form, the group shift and the number of planes are run-time uniform: T x BITS = four instantiations.
//
// 2- AND 3-BIT EXPERTS (opt-in: GPTQ_MOE_LOW_BIT_PREFILL in gptq_moe_t.flags): moe_panel_lowbit_kernel<T, 2 | 3>, the same body (moe_panel_body.inc,
// included into both kernel templates) with the constants of the narrower copy: a strip-chunk is 768 / 512 bytes instead of 1024, a 64-deep step 384 / 256,
// a lane's share 12 / 8 bytes, fetched by ONE global_load_dwordx3 / dwordx2 into a ring element of that size and dequantised in place by
// Deq1_3::frag(words, ks) / Deq1_2::frag(word[ks >> 1] >> 8 (ks & 1)) -- MFMA step ks gets the lane's k = 8 ks .. 8 ks + 7 in the order the A
// operand has them, as at 4 bits.  NT = 4, DW = 2, the constant record (48 bytes, one-byte zero-point), the x side, the loads per step (4 + 8 where a
// group begins: the vmcnt counts) and the reduction are the 4-bit form's.  Four more instantiations under a name of their own, so that "moe_panel_kernel"
// keeps meaning the 4- / 8-bit forms, whose code objects are instruction for instruction what they were.  Registers (read off the code object): 232 (fp16) /
// 234 (bf16) VGPRs at 3 bits, 228 / 226 at 2 bits, no scratch, no spill: inside the 256 of two waves per SIMD.
#include <string.h>

#include <algorithm>

#include "common.cuh"
#include "launch.h"
#include "mma_dequant.cuh"           // DeqSel: Deq1<T> / Deq1_8<T> / Deq1_3<T>, Deq1_2<T>; Mma32<T>
#include "moe_entry.cuh"             // moerows::Entry, load_entry

namespace gptq {
namespace moepanel {

constexpr int BM = 64;
constexpr int XB = BM * 128;                    // one plane of one x buffer: 64 rows x 64 k x 2 bytes
constexpr int LDS_BYTES = 128 * 1024;           // 8 waves x 2 buffers x 1 plane = 4 waves x 2 x 2 planes; the cross-wave sum reuses it
constexpr int UB = 16;                          // accumulator units (float4 per lane) per batch of the cross-wave sum: 16 x 8 waves x 1 KiB
constexpr int nt_of(int bits) { return bits == 8 ? 2 : 4; }

// The dense form (pair == 2, 2 bits only) reads no table: the four fields that describe the tables carry the layer instead (the second name of each union; the
// layout, and with it the 3- / 4- / 8-bit kernels' argument block, is what it was)
struct Args {
    union { const moerows::Entry* table;        // entries of the first projection (pair: W1; W3 is table + E)
            const unsigned* dense_tq; };        // dense: the layer's qweight_tiled
    union { int E; int dense_M; };              // dense: rows of x / out
    int pair;                                   // 0: down, 1: pair, 2: dense (moe_panel_lowbit_kernel<T, 2> only)
    const void* a;                              // sorted rows of the A operand [planes][R][K]; plane q at a + q * plane_bytes
    size_t plane_bytes;
    int planes;
    union { const int* tile_count; const void* dense_bias; };      // dense: bias [N] (T) or NULL
    union { const int4* tiles; const void* dense_cst; };           // dense: the layer's qconst_tiled
    int K, N, chunks, groups, gsh, steps, spw, nct;
    void* out;                                  // pair: H_sorted [R][N] (T); down: Y [R][N] fp32; dense: out [M][N] (T)
};

// 2 bits: the two-word lanes of the copy (DeqSel has the 3-, 4- and 8-bit forms) -- moerows::DeqOf of moe_rows.hip, restated for this file
template <typename T, int BITS> struct DeqOf { typedef typename DeqSel<T, BITS>::type type; };
template <typename T> struct DeqOf<T, 2> { typedef Deq1_2<T> type; };

template <typename T, int BITS>
__global__ void __launch_bounds__(512, 1) moe_panel_kernel(Args p) {
    static_assert(BITS == 4 || BITS == 8, "2 and 3 bits: moe_panel_lowbit_kernel");
#include "moe_panel_body.inc"
}
// the opt-in widths under a name of their own: what counts or lints "moe_panel_kernel" keeps meaning the 4- and 8-bit forms
template <typename T, int BITS>
__global__ void __launch_bounds__(512, 1) moe_panel_lowbit_kernel(Args p) {
    static_assert(BITS == 2 || BITS == 3, "4 and 8 bits: moe_panel_kernel");
#include "moe_panel_body.inc"
}

template <typename T, int BITS>
static hipError_t launch_one(const Args& a, long blocks, int waves, hipStream_t st) {
    if constexpr (BITS == 2 || BITS == 3) hipLaunchKernelGGL((moe_panel_lowbit_kernel<T, BITS>), dim3((unsigned)blocks), dim3(waves * 64), LDS_BYTES, st, a);
    else hipLaunchKernelGGL((moe_panel_kernel<T, BITS>), dim3((unsigned)blocks), dim3(waves * 64), LDS_BYTES, st, a);
    return hipGetLastError();
}
static hipError_t launch_any(int dtype, int bits, const Args& a, long blocks, int waves, hipStream_t st) {
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    if (dtype != GPTQ_F16 && dtype != GPTQ_BF16) return hipErrorInvalidValue;
    const bool h = dtype == GPTQ_F16;
    switch (bits) {
        case 2: return h ? launch_one<f16, 2>(a, blocks, waves, st) : launch_one<bf16, 2>(a, blocks, waves, st);
        case 3: return h ? launch_one<f16, 3>(a, blocks, waves, st) : launch_one<bf16, 3>(a, blocks, waves, st);
        case 4: return h ? launch_one<f16, 4>(a, blocks, waves, st) : launch_one<bf16, 4>(a, blocks, waves, st);
        case 8: return h ? launch_one<f16, 8>(a, blocks, waves, st) : launch_one<bf16, 8>(a, blocks, waves, st);
    }
    return hipErrorInvalidValue;                                // (the entry point's check lets no other width through)
}

static int group_shift(const gptq_layer_t& L) {                 // group of the 64-deep step kt = min(kt >> gsh, groups - 1); -1: not served
    if (L.group_size >= L.K) return 30;
    if (L.group_size % 64) return -1;
    const int q = L.group_size / 64;
    if (q & (q - 1)) return -1;
    return __builtin_ctz((unsigned)q);
}

}  // namespace moepanel

bool moe_prefill_group_ok(const gptq_layer_t& L) { return moepanel::group_shift(L) >= 0; }

MoePrefillPlan plan_moe_prefill(const gptq_moe_t& m, int T, int topk) {
    using namespace moepanel;
    MoePrefillPlan pl{};
    const gptq_layer_t& G = *m.gate[0];
    const int E = m.E, H = G.K, I = G.N;
    const long R = (long)T * topk;
    pl.bm = BM;
    pl.tiles = (int)(R / BM + std::min<long>(E, R));
    pl.act_pair = any_perm_of(m.gate, E) || any_perm_of(m.up, E);
    pl.act_down = any_perm_of(m.down, E);
    pl.nt_pair = nt_of(G.bits) / 2;
    pl.nt_down = nt_of(G.bits);
    pl.waves_pair = pl.act_pair ? 4 : 8;                         // a function of the layers alone: so is every summation order
    pl.waves_down = 8;
    pl.spw_pair = (H / 64 + pl.waves_pair - 1) / pl.waves_pair;  // (fewer steps than waves: the last waves run empty)
    pl.spw_down = (I / 64 + pl.waves_down - 1) / pl.waves_down;
    pl.lds_pair = pl.lds_down = LDS_BYTES;
    pl.launches = T > 0 ? 5 + (pl.act_down ? 1 : 0) : 0;
    const size_t es = dtype_size(G.dtype);
    size_t o = append_route_layout(pl, GPTQ_WORKSPACE_HEADER_BYTES, E, pl.tiles, R);      // the header of a shared workspace belongs to the other entry points: left as it is
    pl.off_xs = o; o += align256((pl.act_pair ? 2 : 1) * (size_t)R * H * es);      // x in sorted order (act-order: through W1's / W3's perm, two planes)
    pl.off_h = o; o += align256((size_t)R * I * es);
    pl.off_y = o; o += align256((size_t)R * H * 4);
    pl.off_hg = o; o += pl.act_down ? align256((size_t)R * I * es) : 0;            // act-order: H_sorted through W2's perm
    pl.bytes = o;
    return pl;
}

hipError_t launch_moe_prefill(const gptq_moe_t& m, const void* table, const MoePrefillPlan& pl, const void* x, const int64_t* idx, const float* w, int T, int topk,
                              void* out, char* ws, hipStream_t st) {
    using namespace moepanel;
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
    auto fill = [&](Args& a, const gptq_layer_t& L, int spw, int cols) {
        a.E = E;
        a.tile_count = tile_count; a.tiles = (const int4*)(ws + pl.off_tiles);
        a.K = L.K; a.N = L.N;
        a.chunks = L.bits == 8 ? L.K / 64 : L.K / 128;        // the decode copy's chunks per strip (2, 3 and 4 bits: 128 deep; the bytes per chunk are the kernel's)
        a.groups = (L.K + L.group_size - 1) / L.group_size;
        a.gsh = group_shift(L);
        a.steps = L.K / 64; a.spw = spw; a.nct = L.N / cols;
    };

    const int planes = pl.act_pair ? 2 : 1;
    if ((e = launch_moe_gather_rows(tab, planes, topk, idx, row_assign, offsets, x, ws + pl.off_xs, E, H, R, st)) != hipSuccess) return e;
    Args g{};
    g.table = tab; g.pair = 1;
    g.a = ws + pl.off_xs; g.plane_bytes = (size_t)R * H * 2; g.planes = planes;
    g.out = ws + pl.off_h;
    fill(g, G, pl.spw_pair, 32 * pl.nt_pair);
    if ((e = launch_any(G.dtype, G.bits, g, (long)pl.tiles * g.nct, pl.waves_pair, st)) != hipSuccess) return e;

    Args d{};
    d.table = tab + 2 * (size_t)E; d.pair = 0;
    if (pl.act_down) {
        if ((e = launch_moe_gather_rows(tab + 2 * (size_t)E, 1, 0, idx, row_assign, offsets, ws + pl.off_h, ws + pl.off_hg, E, I, R, st)) != hipSuccess) return e;
        d.a = ws + pl.off_hg;
    } else {
        d.a = ws + pl.off_h;
    }
    d.plane_bytes = 0; d.planes = 1;
    d.out = ws + pl.off_y;
    fill(d, D, pl.spw_down, 32 * pl.nt_down);
    if ((e = launch_any(D.dtype, D.bits, d, (long)pl.tiles * d.nct, pl.waves_down, st)) != hipSuccess) return e;

    return launch_moe_combine(pos, w, (const float*)(ws + pl.off_y), out, T, topk, H, 1, R, G.dtype, st);
}

// ---- the dense form (one flagged 2-bit QuantLinear layer; moe_panel_body.inc) --------------------------------------------------------------------
// What the down form takes: fp16 / bf16, K a whole number of 128-deep chunks of the copy, N a whole number of 32 NT-column tiles, a group size of 64 2^n or one
// group; act-order layers with their re-sequenced rows (the copy is made of them; the caller permutes x).  The lane offsets are 32-bit: one strip's bytes.
bool dense_panel_int2_ok(const gptq_layer_t& L, int M) {
    if (!copy_rows_int2(L) || (L.dtype != GPTQ_F16 && L.dtype != GPTQ_BF16) || L.epilogue != GPTQ_EPI_NONE) return false;
    if (L.g_idx != nullptr && !(L.perm && L.qweight_seq)) return false;
    if (L.K % 128 || L.N % (32 * moepanel::nt_of(2)) || moepanel::group_shift(L) < 0) return false;
    return M >= 1 && M <= GPTQ_MOE_PREFILL_MAX_ROWS;
}

PanelPlan plan_dense_panel_int2(const gptq_layer_t& L, int M) {
    PanelPlan pl{};
    if (!dense_panel_int2_ok(L, M)) return pl;
    pl.mt = 2; pl.nt = moepanel::nt_of(2); pl.kp = 8;            // the K split is a function of the layer alone (ROW INDEPENDENCE above)
    pl.nbm = (M + moepanel::BM - 1) / moepanel::BM;
    pl.nbn = L.N / (32 * pl.nt);
    pl.spw = (L.K / 64 + pl.kp - 1) / pl.kp;                     // (fewer steps than waves: the last waves run empty)
    pl.lds_bytes = moepanel::LDS_BYTES;
    pl.ok = true;
    return pl;
}

hipError_t launch_dense_panel_int2(const gptq_layer_t& L, const void* x, void* out, int M, const PanelPlan& pl, hipStream_t st) {
    if (!pl.ok || !dense_panel_int2_ok(L, M)) return hipErrorInvalidValue;
    moepanel::Args a{};
    a.dense_tq = L.qweight_tiled; a.dense_cst = L.qconst_tiled; a.dense_bias = L.bias; a.dense_M = M;
    a.pair = 2;
    a.a = x; a.plane_bytes = 0; a.planes = 1;
    a.K = L.K; a.N = L.N;
    a.chunks = L.K / 128;
    a.groups = (L.K + L.group_size - 1) / L.group_size;
    a.gsh = moepanel::group_shift(L);
    a.steps = L.K / 64; a.spw = pl.spw; a.nct = pl.nbn;
    a.out = out;
    return moepanel::launch_any(L.dtype, 2, a, (long)pl.nbm * pl.nbn, pl.kp, st);
}

// grants the 128 KiB of dynamic LDS the kernel runs in
hipError_t init_moe_prefill_device() {
    hipError_t e = hipSuccess;
    auto grant = [&](auto kern) { hipError_t r = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, moepanel::LDS_BYTES); if (e == hipSuccess) e = r; };
    grant(moepanel::moe_panel_kernel<f16, 4>); grant(moepanel::moe_panel_kernel<f16, 8>);
    grant(moepanel::moe_panel_kernel<bf16, 4>); grant(moepanel::moe_panel_kernel<bf16, 8>);
    grant(moepanel::moe_panel_lowbit_kernel<f16, 3>); grant(moepanel::moe_panel_lowbit_kernel<f16, 2>);
    grant(moepanel::moe_panel_lowbit_kernel<bf16, 3>); grant(moepanel::moe_panel_lowbit_kernel<bf16, 2>);
    return e;
}

}  // namespace gptq
