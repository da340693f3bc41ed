// moe_panel_body.inc -- the body of moe_panel_kernel<T, BITS> (4 / 8 bits) and moe_panel_lowbit_kernel<T, BITS> (2 / 3 bits), included into both
// (moe_panel.hip: the design, the names it uses).  In scope: T, BITS, Args p.  Text inclusion rather than a shared __device__ function: the 4- and 8-bit
// kernels keep their code objects instruction for instruction (moe_rows_body.inc: an inlined function body changed the scalar prologue and the registers).
//
// DENSE form (2 bits only, p.pair == 2, launch-uniform: launch_dense_panel_int2): one QuantLinear layer on its decode copy.  No tables: tile t is rows
// [64 t, min(64 t + 64, M)) of x [M][K], the copy / constants / bias / M are launch arguments (Args: dense_tq, dense_cst, dense_bias, dense_M), the K loop is
// the down form's (NT column blocks, one plane) and the store is out[m][n] = T(sum + bias[n]) into out [M][N].
//
// What the width changes (utils.hip prepack_decode_weights_kernel: a chunk of the copy = [4 k-slots][16 columns][WPL words], 128 k deep; 8 bits: 64 k):
//                 8 bits   4 bits   3 bits   2 bits
//   STRIP_CH       1024     1024      768      512     bytes of one chunk of one 16-column strip
//   STEP_B         1024      512      384      256     bytes of a 64-deep step of a strip
//   SLOT_B          512      256      192      128     offset of the lane's half (k-slot 2 (kt & 1) + half; 8 bits: k-slots 2 half, + 1)
//   COL_B            16       16       12        8     a lane's bytes of a k-slot: ONE dwordx4 / dwordx4 / dwordx3 / dwordx2 (8 bits: NH = 2 of them)
// The last byte a lane reads: (steps - 1) STEP_B + SLOT_B + 15 COL_B + COL_B = steps STEP_B = chunks STRIP_CH -- the end of its strip.
    constexpr int MT = 2, NT = nt_of(BITS), HB = NT / 2, NX = 4 * MT;
    constexpr int NH = BITS == 8 ? 2 : 1;                      // weight loads per column block and step
    constexpr unsigned COL_B = BITS == 3 ? 12u : (BITS == 2 ? 8u : 16u);
    constexpr unsigned STEP_B = BITS == 8 ? 1024u : 32u * COL_B, SLOT_B = BITS == 8 ? 512u : 16u * COL_B;
    constexpr unsigned STRIP_CH = BITS == 8 ? 1024u : 64u * COL_B, REC = BITS == 8 ? 64u : 48u;      // (2 / 3 bits: the 4-bit record, a one-byte zero-point)
    constexpr int NWL = NT * NH;                               // weight loads of a step (ONE per column block at 2, 3 and 4 bits); + 2 NT where constants are loaded
    // register sets of packed weights.  3 (8 bits, NT = 2): W(kt + 2) is issued inside step kt; 2 (2, 3, 4 bits, NT = 4: the accumulators alone are 128 registers):
    // at the end of the step, into the set it just consumed
    constexpr int DW = BITS == 8 ? 3 : 2;
    constexpr int UNITS = 4 * MT * NT;                         // float4s per lane of the accumulator tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int ct = blockIdx.x % p.nct, tile = blockIdx.x / p.nct;
    bool dense = false;                                        // (a constant everywhere but at 2 bits)
    if constexpr (BITS == 2) dense = p.pair == 2;
    int4 tl;
    if (dense) {
        tl = int4{0, tile * BM, min(BM, p.dense_M - tile * BM), 0};      // the grid is exactly the tiles: none is empty
    } else {
        if (tile >= *p.tile_count) return;
        tl = p.tiles[tile];
    }
    const int e = __builtin_amdgcn_readfirstlane(tl.x), row0 = __builtin_amdgcn_readfirstlane(tl.y), rows = __builtin_amdgcn_readfirstlane(tl.z);
    const int pair = dense ? 0 : p.pair, planes = p.planes;
    const int n0 = ct * 32 * (pair ? HB : NT);
    // rows past the tile's count re-read its last row: DMA i fetches rows 8 min(i, imax) + min(r8, rlast) (the panel body's PART form)
    const int imax = (rows - 1) >> 3, rlast = (rows - 1) & 7;

    const moerows::Entry e0 = dense ? moerows::Entry{p.dense_tq, p.dense_cst, nullptr, nullptr} : moerows::load_entry(p.table + e);
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

    // a lane's words of one k-slot of the copy, written by ONE load (no copies between the load and the wait): 3 words at 3 bits, 2 at 2 bits
    using WV = std::conditional_t<BITS == 3, u32x3, std::conditional_t<BITS == 2, u32x2, u32x4>>;
    struct Buf { WV w[NT][NH]; unsigned cs[NT], cz[NT]; };
    Buf q[DW];
    // every register of the ring starts as its own opaque definition: the compiler cannot share one between two loads' destinations and split them with a
    // copy behind the first load (DESIGN 4.5)
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
            const char* wsrc = wbase[nt] + (size_t)kt * STEP_B;      // 2, 3, 4 bits: chunk kt / 2, k-slots 2 (kt & 1) + half; 8 bits: chunk kt, k-slots 2 half, + 1
            if constexpr (BITS == 3) asm volatile("global_load_dwordx3 %0, %1, %2" : "=v"(B.w[nt][0]) : "v"(wlane), "s"(wsrc) : "memory");
            else if constexpr (BITS == 2) asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(B.w[nt][0]) : "v"(wlane), "s"(wsrc) : "memory");
            else asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(B.w[nt][0]) : "v"(wlane), "s"(wsrc) : "memory");
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

    typename DeqOf<T, BITS>::type dq[NT];                      // the current group's constants (set up where a group begins)
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
        // The counts, recounted per width: W(.) is NWL = NT NH weight loads -- 4 bits: 4 x 1 dwordx4; 3 bits: 4 x 1 dwordx3; 2 bits: 4 x 1 dwordx2;
        // 8 bits: 2 x 2 dwordx4 -- = 4 at every width, plus 2 NT constant loads (one ushort of scale and one ubyte / ushort of zero-point per column
        // block: 8 at 2, 3 and 4 bits, 4 at 8) when the step begins a group.
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
                if (has_c(ktx)) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWL + 2 * NT) : "memory");      // W(kt + 1) stays in flight: with constants 4 + 8 = 12 (8 bits: 4 + 4 = 8)
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWL) : "memory");                           // ... without: 4
                claim(q[j]);
                if (has_c(kt)) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) dq[nt].setup(q[j].cs[nt], q[j].cz[nt]);
                }
                const char* xb = xbuf + buf * planes * XB;
                // the 8 weights k = 32 half + 8 ks + 0..7 of column block nt, dequantised (bit-exact W)
                auto frag_of = [&](int nt, int ks) __attribute__((always_inline)) -> u32x4 {
                    if constexpr (BITS == 4) return dq[nt].frag(q[j].w[nt][0][ks]);
                    else if constexpr (BITS == 3) return dq[nt].frag(q[j].w[nt][0], ks);
                    else if constexpr (BITS == 2) return dq[nt].frag(q[j].w[nt][0][ks >> 1] >> (8 * (ks & 1)));
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
                    for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = Mma32<T>::run(a[h & 1][mt], bq[i & 1], acc[mt][nt]);
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
        } else if (dense) {
            for (int lu = wave; lu < UBC; lu += nw) {
                const int u = b0 + lu;
                const int mt = u / (4 * NT), rq = (u / NT) % 4, nt = u % NT;
                const f32x4 s = wsum(lu);
                const int n = n0 + 32 * nt + l31;
                const float b = p.dense_bias ? DType<T>::to_f32(((const T*)p.dense_bias)[n]) : 0.f;      // (a 2-byte load: no dwordx4 in this kernel but the x DMAs)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = 32 * mt + 8 * rq + 4 * half + i;
                    if (row < rows) ((T*)p.out)[(size_t)(row0 + row) * N + n] = DType<T>::from_f32(s[i] + b);
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
