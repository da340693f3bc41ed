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
#include <string.h>

#include <algorithm>

#include "common.cuh"
#include "launch.h"
#include "gemm_wide_common.cuh"      // wide::Mma<T>
#include "gemm_rows_kernel.cuh"      // rowsk::Deq1<T> / Deq1_8<T>
#include "moe_entry.cuh"             // moerows::Entry, load_entry

namespace gptq {
namespace moepanel {

constexpr int BM = 64;
constexpr int XB = BM * 128;                    // one plane of one x buffer: 64 rows x 64 k x 2 bytes
constexpr int LDS_BYTES = 128 * 1024;           // 8 waves x 2 buffers x 1 plane = 4 waves x 2 x 2 planes; the cross-wave sum reuses it
constexpr int UB = 16;                          // accumulator units (float4 per lane) per batch of the cross-wave sum: 16 x 8 waves x 1 KiB
constexpr int nt_of(int bits) { return bits == 8 ? 2 : 4; }

struct Args {
    const moerows::Entry* table;                // entries of the first projection (pair: W1; W3 is table + E)
    int E, pair;
    const void* a;                              // sorted rows of the A operand [planes][R][K]; plane q at a + q * plane_bytes
    size_t plane_bytes;
    int planes;
    const int* tile_count;
    const int4* tiles;
    int K, N, chunks, groups, gsh, steps, spw, nct;
    void* out;                                  // pair: H_sorted [R][N] (T); down: Y [R][N] fp32
};

template <typename T, int BITS>
__global__ void __launch_bounds__(512, 1) moe_panel_kernel(Args p) {
    constexpr int MT = 2, NT = nt_of(BITS), HB = NT / 2, NX = 4 * MT;
    constexpr int NH = BITS == 8 ? 2 : 1;                      // 16-byte loads per column block and step
    constexpr unsigned STEP_B = BITS == 8 ? 1024u : 512u, SLOT_B = BITS == 8 ? 512u : 256u, COL_B = 16u;
    constexpr unsigned STRIP_CH = 1024u, REC = BITS == 8 ? 64u : 48u;
    constexpr int NWL = NT * NH;                               // weight loads of a step; + 2 NT where constants are loaded
    // register sets of packed weights.  3 (8 bits, NT = 2): W(kt + 2) is issued inside step kt; 2 (4 bits, NT = 4: the accumulators alone are 128 registers):
    // at the end of the step, into the set it just consumed
    constexpr int DW = BITS == 8 ? 3 : 2;
    constexpr int UNITS = 4 * MT * NT;                         // float4s per lane of the accumulator tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int ct = blockIdx.x % p.nct, tile = blockIdx.x / p.nct;
    if (tile >= *p.tile_count) return;
    const int4 tl = p.tiles[tile];
    const int e = __builtin_amdgcn_readfirstlane(tl.x), row0 = __builtin_amdgcn_readfirstlane(tl.y), rows = __builtin_amdgcn_readfirstlane(tl.z);
    const int pair = p.pair, planes = p.planes;
    const int n0 = ct * 32 * (pair ? HB : NT);
    // rows past the tile's count re-read its last row: DMA i fetches rows 8 min(i, imax) + min(r8, rlast) (the panel body's PART form)
    const int imax = (rows - 1) >> 3, rlast = (rows - 1) & 7;

    const moerows::Entry e0 = moerows::load_entry(p.table + e);
    const moerows::Entry e1 = pair ? moerows::load_entry(p.table + p.E + e) : e0;
    const char* wbase[NT];
    const char* cbase[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const bool up = pair && nt >= HB;
        const int nb = n0 + 32 * (up ? nt - HB : nt);
        wbase[nt] = (const char*)(up ? e1.tq : e0.tq) + (size_t)(nb >> 4) * p.chunks * STRIP_CH;
        cbase[nt] = (const char*)(up ? e1.cst : e0.cst) + (size_t)(nb >> 4) * p.groups * REC;
    }
    const unsigned wlane = (unsigned)(l31 >> 4) * (unsigned)p.chunks * STRIP_CH + (unsigned)half * SLOT_B + (unsigned)(l31 & 15) * COL_B;
    const unsigned clane = (unsigned)(l31 >> 4) * (unsigned)p.groups * REC;
    const unsigned slane = clane + (unsigned)(l31 & 15) * 2u, zlane = clane + 32u + (unsigned)(l31 & 15) * (BITS == 8 ? 2u : 1u);

    char* const xbuf = smem + (size_t)wave * 2 * planes * XB;  // buffer b, plane q: xbuf + (b planes + q) XB
    const unsigned xbuf_lds = lds_addr_of(xbuf);
    // x DMA i (8 rows x 128 bytes): lane (r8 = lane >> 3, kc = lane & 7) lands at LDS row 8 i + r8, slot kc, and fetches piece kc ^ (((8 i + r8) >> 1) & 7)
    unsigned xoff[2], xoff_last[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const unsigned r8 = (unsigned)lane >> 3, kc = (unsigned)lane & 7u;
        xoff[par] = r8 * (unsigned)p.K * 2u + ((kc ^ (4u * par + (r8 >> 1))) * 16u);
        xoff_last[par] = min(r8, (unsigned)rlast) * (unsigned)p.K * 2u + ((kc ^ (4u * par + (r8 >> 1))) * 16u);      // (the swizzle follows the LDS row, the address the clamped source row)
    }
    const char* const xrow0 = (const char*)p.a + (size_t)row0 * p.K * 2;
    const size_t x8 = (size_t)8 * p.K * 2;
    // A fragment of row block mt, MFMA step ks: piece 4 half + ks of row 32 mt + l31, stored at slot piece ^ ((row >> 1) & 7)
    unsigned aoff[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) aoff[ks] = (unsigned)(l31 * 128 + (((half * 4 + ks) ^ ((l31 >> 1) & 7)) * 16));
    const unsigned a3off = planes > 1 ? (unsigned)XB : 0u;     // W3's blocks read plane 1 when there is one

    struct Buf { u32x4 w[NT][NH]; unsigned cs[NT], cz[NT]; };
    Buf q[DW];
    // every register of the ring starts as its own opaque definition: the compiler cannot share one between two loads' destinations and split them with a
    // copy behind the first load
#pragma unroll
    for (int j = 0; j < DW; ++j)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int h = 0; h < NH; ++h) asm volatile("; ring slot" : "=v"(q[j].w[nt][h]));
            asm volatile("v_mov_b32 %0, 0" : "=v"(q[j].cs[nt]));
            asm volatile("v_mov_b32 %0, 0" : "=v"(q[j].cz[nt]));
        }
    const int k0 = wave * p.spw, k1 = min(k0 + p.spw, p.steps);
    // constants only where a group begins (and at the wave's first step).  "+v": a step without constants leaves the registers as they are
    const int gsh = p.gsh, gmask = (1 << gsh) - 1;
    auto has_c = [&](int kt) -> bool { return kt == k0 || (kt & gmask) == 0; };
    auto issue_w = [&](int kt, Buf& B) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const char* wsrc = wbase[nt] + (size_t)kt * STEP_B;      // 4 bits: chunk kt / 2, k-slots 2 (kt & 1) + half; 8 bits: chunk kt, k-slots 2 half, + 1
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(B.w[nt][0]) : "v"(wlane), "s"(wsrc) : "memory");
            if constexpr (BITS == 8) asm volatile("global_load_dwordx4 %0, %1, %2 offset:256" : "=v"(B.w[nt][1]) : "v"(wlane), "s"(wsrc) : "memory");
        }
        if (has_c(kt)) {
            const int g = min(kt >> gsh, p.groups - 1);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const char* csrc = cbase[nt] + (size_t)g * REC;
                asm volatile("global_load_ushort %0, %1, %2" : "+v"(B.cs[nt]) : "v"(slane), "s"(csrc) : "memory");
                if constexpr (BITS == 8) asm volatile("global_load_ushort %0, %1, %2" : "+v"(B.cz[nt]) : "v"(zlane), "s"(csrc) : "memory");
                else asm volatile("global_load_ubyte %0, %1, %2" : "+v"(B.cz[nt]) : "v"(zlane), "s"(csrc) : "memory");
            }
        }
    };
    auto issue_x = [&](int kt, int buf, int i0, int i1) __attribute__((always_inline)) {      // DMAs [i0, i1) of step kt's rows (every plane) into buffer buf
        const char* xsrc = xrow0 + (size_t)kt * 128;
        const unsigned l0 = __builtin_amdgcn_readfirstlane(xbuf_lds + (unsigned)(buf * planes * XB));
#pragma unroll
        for (int i = i0; i < i1; ++i) {
            const unsigned xo = i >= imax ? xoff_last[i & 1] : xoff[i & 1];
            const char* xs = xsrc + (size_t)min(i, imax) * x8;
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(l0 + (unsigned)(i * 1024)), "v"(xo), "s"(xs) : "memory");
            if (planes > 1) {
                const char* xs1 = xs + p.plane_bytes;
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(l0 + (unsigned)(XB + i * 1024)), "v"(xo), "s"(xs1) : "memory");
            }
        }
    };
    // the registers pass through a statement behind the wait so that no use of them is scheduled in front of it
    auto claim = [&](Buf& B) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int h = 0; h < NH; ++h) asm volatile("" : "+v"(B.w[nt][h])::"memory");
            asm volatile("" : "+v"(B.cs[nt]), "+v"(B.cz[nt])::"memory");
        }
    };

    typename rowsk::DeqSel<T, BITS>::type dq[NT];              // the current group's constants (set up where a group begins)
    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    if (k0 < k1) {
        // VMEM queue of the wave, oldest first, at the top of step kt: [W(kt), X(kt), W(kt + 1)] -> s_waitcnt vmcnt(loads of W(kt + 1)) leaves exactly that
        // in flight; inside the step X(kt + 1) goes first (under MFMA steps 0 and 1, half each) and W(kt + 2) behind it (DW = 3: at step 2; DW = 2: at the end of the step).  Steps past the wave's
        // range are clamped to its last step (redundant loads, no branches).
        const int kl = k1 - 1;
        issue_w(k0, q[0]);
        issue_x(k0, 0, 0, NX);
        issue_w(min(k0 + 1, kl), q[1]);
        for (int kb = k0; kb < k1; kb += DW) {
#pragma unroll
            for (int j = 0; j < DW; ++j) {
                const int kt = kb + j;
                if (kt >= k1) break;
                const int buf = (kt - k0) & 1;
                const int ktx = min(kt + 1, kl), ktw = min(kt + 2, kl);
                if (has_c(ktx)) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWL + 2 * NT) : "memory");      // W(kt + 1) stays in flight: with or without constants
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWL) : "memory");
                claim(q[j]);
                if (has_c(kt)) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) dq[nt].setup(q[j].cs[nt], q[j].cz[nt]);
                }
                const char* xb = xbuf + buf * planes * XB;
                // the 8 weights k = 32 half + 8 ks + 0..7 of column block nt, dequantised (bit-exact W)
                auto frag_of = [&](int nt, int ks) __attribute__((always_inline)) -> u32x4 {
                    if constexpr (BITS == 4) return dq[nt].frag(q[j].w[nt][0][ks]);
                    else return dq[nt].frag(q[j].w[nt][ks >> 1][2 * (ks & 1)], q[j].w[nt][ks >> 1][2 * (ks & 1) + 1]);
                };
                // A fragments by half h = 2 ks + (the second HB blocks: W3's in the pair form, which read plane 1 when there is one)
                auto load_a = [&](int h, u32x4* dst) __attribute__((always_inline)) {
                    const char* src = xb + ((h & 1) ? a3off : 0u) + aoff[h >> 1];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) dst[mt] = *(const u32x4*)(src + mt * 4096);
                };
                u32x4 a[2][MT], bq[2];
                load_a(0, a[0]);
                bq[0] = frag_of(0, 0);
                // software pipeline over the 4 NT (MFMA step, column block) pairs: the NEXT pair's B fragment is dequantised between the MT MFMAs of this pair
#pragma unroll
                for (int i = 0; i < 4 * NT; ++i) {
                    const int ks = i / NT, nt = i % NT, h = i / HB;
                    if (i % HB == 0) {
                        __builtin_amdgcn_sched_barrier(0);     // (the scheduler otherwise strings the MFMAs of one accumulator across the steps: dependent chains)
                        if (h + 1 < 8) load_a(h + 1, a[(h + 1) & 1]);
                        if (nt == 0) {
                            if (ks == 0) issue_x(ktx, buf ^ 1, 0, NX / 2);
                            if (ks == 1) issue_x(ktx, buf ^ 1, NX / 2, NX);
                            if (DW == 3 && ks == 2) issue_w(ktw, q[(j + 2) % DW]);
                        }
                    }
                    if (i + 1 < 4 * NT) bq[(i + 1) & 1] = frag_of((i + 1) % NT, (i + 1) / NT);
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = wide::Mma<T>::run(a[h & 1][mt], bq[i & 1], acc[mt][nt]);
                    if (i + 1 < 4 * NT) {                     // MFMA, its share of the next fragment's VALU, MFMA, ...
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 7, 0);
                    }
                }
                if (DW == 2) issue_w(ktw, q[j]);
            }
        }
        // The clamped loads of the last steps are still in flight and nothing below reads their registers: every register set passes through a statement
        // BEHIND a full wait, so it stays allocated until the loads are in -- nothing is in flight into a register the epilogue reuses.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < DW; ++j) claim(q[j]);
    }

    // ---- the K parts meet in LDS (wave order), silu * mul, store ---------------------------------------------------------------------------------
    // unit u = ((mt, rq), nt): the float4 acc[mt][nt][4 rq .. 4 rq + 3] of every lane = rows 32 mt + 8 rq + 4 half + 0..3 of the block's column l31 (C/D layout
    // of the 32x32 MFMA).  A batch of UB units: every wave writes its float4s ([unit][wave][lane]: 1 KiB per unit and wave), then the waves share the
    // batch's units (pair form: its (gate, up) pairs -- blocks nt and nt + HB of one (mt, rq)) and sum each over all waves in wave order.
    __syncthreads();                                           // every wave's x DMAs have landed (the wait above): the buffers are about to be overwritten
    float* const red = (float*)smem;
    const int N = p.N;
    constexpr int UBC = UB < UNITS ? UB : UNITS;
    auto wsum = [&](int lu) -> f32x4 {
        f32x4 s = *(const f32x4*)(red + ((size_t)(lu * nw) * 64 + lane) * 4);
        for (int w = 1; w < nw; ++w) s += *(const f32x4*)(red + ((size_t)(lu * nw + w) * 64 + lane) * 4);
        return s;
    };
#pragma unroll
    for (int b0 = 0; b0 < UNITS; b0 += UBC) {
        if (b0) __syncthreads();
#pragma unroll
        for (int u = b0; u < b0 + UBC; ++u) {
            const int mt = u / (4 * NT), rq = (u / NT) % 4, nt = u % NT;
            const f32x16& c = acc[mt][nt];
            const f32x4 v = {c[rq * 4], c[rq * 4 + 1], c[rq * 4 + 2], c[rq * 4 + 3]};
            *(f32x4*)(red + ((size_t)((u - b0) * nw + wave) * 64 + lane) * 4) = v;
        }
        __syncthreads();
        if (pair) {
            for (int it = wave; it < UBC / 2; it += nw) {
                const int lu = (it / HB) * NT + it % HB, u = b0 + lu;
                const int mt = u / (4 * NT), rq = (u / NT) % 4;
                const f32x4 sg = wsum(lu), su = wsum(lu + HB);
                const int n = n0 + 32 * (it % HB) + l31;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = 32 * mt + 8 * rq + 4 * half + i;
                    const float gv = sg[i];
                    if (row < rows) ((T*)p.out)[(size_t)(row0 + row) * N + n] = DType<T>::from_f32(gv / (1.f + __expf(-gv)) * su[i]);
                }
            }
        } else {
            for (int lu = wave; lu < UBC; lu += nw) {
                const int u = b0 + lu;
                const int mt = u / (4 * NT), rq = (u / NT) % 4, nt = u % NT;
                const f32x4 s = wsum(lu);
                const int n = n0 + 32 * nt + l31;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = 32 * mt + 8 * rq + 4 * half + i;
                    if (row < rows) ((float*)p.out)[(size_t)(row0 + row) * N + n] = s[i];
                }
            }
        }
    }
}

template <typename T, int BITS>
static hipError_t launch_one(const Args& a, long blocks, int waves, hipStream_t st) {
    hipLaunchKernelGGL((moe_panel_kernel<T, BITS>), dim3((unsigned)blocks), dim3(waves * 64), LDS_BYTES, st, a);
    return hipGetLastError();
}
static hipError_t launch_any(int dtype, int bits, const Args& a, long blocks, int waves, hipStream_t st) {
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    if (dtype == GPTQ_F16) return bits == 4 ? launch_one<f16, 4>(a, blocks, waves, st) : launch_one<f16, 8>(a, blocks, waves, st);
    return bits == 4 ? launch_one<bf16, 4>(a, blocks, waves, st) : launch_one<bf16, 8>(a, blocks, waves, st);
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
        a.chunks = L.bits == 8 ? L.K / 64 : L.K / 128;        // the decode copy's chunks per strip
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

// grants the 128 KiB of dynamic LDS the kernel runs in
hipError_t init_moe_prefill_device() {
    hipError_t e = hipSuccess;
    auto grant = [&](auto kern) { hipError_t r = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, moepanel::LDS_BYTES); if (e == hipSuccess) e = r; };
    grant(moepanel::moe_panel_kernel<f16, 4>); grant(moepanel::moe_panel_kernel<f16, 8>);
    grant(moepanel::moe_panel_kernel<bf16, 4>); grant(moepanel::moe_panel_kernel<bf16, 8>);
    return e;
}

}  // namespace gptq
