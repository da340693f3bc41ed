// moe_rows_body.inc -- the body of moe_rows_kernel<T, BITS> (4 / 8 bits) and moe_rows_lowbit_kernel<T, BITS> (2 / 3 bits), included into both (moe_rows.hip:
// the design, the names it uses).  In scope: T, BITS, Args p.  Text inclusion rather than a shared __device__ function: the 4- and 8-bit kernels keep their
// code objects instruction for instruction (an inlined function body changed their scalar prologue and register assignment).
//
// DENSE form (2 bits only, p.pair == 2, launch-uniform: launch_dense_rows_int2): one QuantLinear layer on its decode copy.  No tables: tile t is rows
// [16 t, min(16 t + 16, M)) of x [M][K], the copy / constants / bias / M are launch arguments (Args: dense_tq, dense_cst, dense_bias, dense_M), the K loop is
// the down form's (NS strips behind one staged chunk, one plane, rows as they lie) and the store is out[m][n] = T(sum + bias[n]) into out [M][N].
    constexpr int NH = BITS == 8 ? 2 : 1;                      // chunks of the copy per 128-deep chunk of the rows
    constexpr unsigned REC = BITS == 8 ? 64u : 48u;            // constant record (2 / 3 bits: the 4-bit record, a one-byte zero-point)
    constexpr unsigned WCH = BITS == 3 ? 768u : (BITS == 2 ? 512u : 1024u), WLANE = BITS == 3 ? 12u : (BITS == 2 ? 8u : 16u);      // strip-chunk of the copy, a lane's bytes of it
    constexpr int NDMA = 4, NW = 3 * NH * NS;                  // DMA instructions of one plane of a chunk; a chunk's weight + constant loads (ONE weight load per
                                                               // strip and half at every width + scale + zero-point: 3 NH NS)
    constexpr int DW = 2;                                      // ring of chunks in flight per wave (4 bits: 48 registers, 8 bits: 96, 3 bits: 40, 2 bits: 32)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
    const int sgi = blockIdx.x % p.nsg, tile = blockIdx.x / p.nsg;
    // 2 bits: p.pair == 2 is the dense form.  PAIR is p.pair itself at every other width (the condition folds in the front end: those kernels read the
    // argument where and as often as they did)
#define PAIR (BITS == 2 ? p.pair == 1 : p.pair != 0)
    bool dense = false;
    if constexpr (BITS == 2) dense = p.pair == 2;
    int4 tl;
    if constexpr (BITS == 2) {
        if (dense) {
            tl = int4{0, tile * BM, min(BM, p.dense_M - tile * BM), 0};      // the grid is exactly the tiles: none is empty
        } else {
            if (tile >= *p.tile_count) return;
            tl = p.tiles[tile];
        }
    } else {
        if (tile >= *p.tile_count) return;
        tl = p.tiles[tile];
    }
    const int e = __builtin_amdgcn_readfirstlane(tl.x), row0 = __builtin_amdgcn_readfirstlane(tl.y), rows = __builtin_amdgcn_readfirstlane(tl.z);
    const int S = PAIR ? NS / 2 : NS, s0 = sgi * S;
    const int planes = p.planes;
    const int r = lane & 15, g = lane >> 4;

    Entry e0;
    if constexpr (BITS == 2) e0 = dense ? Entry{p.dense_tq, p.dense_cst, nullptr, nullptr} : load_entry(p.table + e);
    else e0 = load_entry(p.table + e);
    const Entry e1 = PAIR ? load_entry(p.table + p.E + e) : e0;
    const char* wb[NS];
    const char* cb[NS];
#pragma unroll
    for (int v = 0; v < NS; ++v) {
        const bool up = PAIR && v >= NS / 2;
        const int strip = s0 + (up ? v - NS / 2 : v);
        wb[v] = (const char*)(up ? e1.tq : e0.tq) + (size_t)strip * (size_t)(p.chunks * NH) * WCH;
        cb[v] = (const char*)(up ? e1.cst : e0.cst) + (size_t)strip * (size_t)p.groups * REC;
    }

    char* const xbuf = smem + (size_t)wave * 2 * planes * XB;      // buffer b, plane q: xbuf + (b planes + q) XB
    const unsigned xbuf_lds = lds_addr_of(xbuf);
    // DMA i of a plane (4 rows x 256 bytes): lane (rr = lane >> 4, slot = lane & 15) fetches piece slot ^ (row & 15) of row 4 i + rr, so that LDS slot s of row R
    // holds piece s ^ (R & 15) (gemm_rows_kernel.cuh); the row itself is looked up here
    unsigned xoff[NDMA];
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
        const int row = 4 * i + g;
        const int sr = row0 + min(row, rows - 1);              // rows past the tile repeat its last one (their outputs are not stored)
        const int m = p.row_assign ? p.row_assign[sr] / p.topk : sr;
        xoff[i] = (unsigned)m * (unsigned)p.K * 2u + (unsigned)((r ^ (row & 15)) * 16);
    }
    unsigned aoff[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int piece = BITS == 8 ? 8 * (w >> 1) + 2 * g + (w & 1) : 4 * g + w;
        aoff[w] = (unsigned)(r * 256 + ((piece ^ r) * 16));
    }
    const unsigned a3off = planes > 1 ? (unsigned)XB : 0u;     // W3's strips read plane 1 when there is one
    const unsigned wlane = (unsigned)lane * WLANE;
    const int gm = p.gm;
    const unsigned glane = BITS == 8 ? (gm == 2 ? (unsigned)(g >> 1) * REC : 0u) : (gm == 2 ? (unsigned)g * REC : (gm == 1 ? (unsigned)(g >> 1) * REC : 0u));
    const unsigned slane = glane + (unsigned)r * 2u, zlane = glane + 32u + (unsigned)r * (BITS == 8 ? 2u : 1u);
    const int c0 = wave * p.cpw, c1 = min(c0 + p.cpw, p.chunks);

    // a lane's words of one chunk of the copy, written by ONE load (no copies between the load and the wait): 3 words at 3 bits, 2 at 2 bits
    using WV = std::conditional_t<BITS == 3, u32x3, std::conditional_t<BITS == 2, u32x2, u32x4>>;
    struct Buf { WV wq[NS][NH]; unsigned cs[NS][NH], cz[NS][NH]; };
    Buf q[DW];
    // every register of the ring starts as its own opaque definition: the compiler cannot share one between two loads' destinations and split them with a
    // copy behind the first load (DESIGN 4.5)
#pragma unroll
    for (int j = 0; j < DW; ++j)
#pragma unroll
        for (int v = 0; v < NS; ++v)
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                asm volatile("; ring slot" : "=v"(q[j].wq[v][h]));
                asm volatile("v_mov_b32 %0, 0" : "=v"(q[j].cs[v][h]));
                asm volatile("v_mov_b32 %0, 0" : "=v"(q[j].cz[v][h]));
            }
    auto issue_w = [&](int c, Buf& B) __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < NS; ++v) {
            const char* const wv = wb[v];
            const char* const cv = cb[v];
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const char* wsrc = wv + (size_t)(c * NH + h) * WCH;
                const int grp = gm == 0 ? min(c >> p.gshift, p.groups - 1) : (BITS == 8 ? (gm == 1 ? 2 * c + h : 4 * c + 2 * h) : (gm == 1 ? 2 * c : 4 * c));
                const char* csrc = cv + (size_t)grp * REC;
                if constexpr (BITS == 3) asm volatile("global_load_dwordx3 %0, %1, %2" : "=v"(B.wq[v][h]) : "v"(wlane), "s"(wsrc) : "memory");
                else if constexpr (BITS == 2) asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(B.wq[v][h]) : "v"(wlane), "s"(wsrc) : "memory");
                else asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(B.wq[v][h]) : "v"(wlane), "s"(wsrc) : "memory");
                asm volatile("global_load_ushort %0, %1, %2" : "=v"(B.cs[v][h]) : "v"(slane), "s"(csrc) : "memory");
                if constexpr (BITS == 8) asm volatile("global_load_ushort %0, %1, %2" : "=v"(B.cz[v][h]) : "v"(zlane), "s"(csrc) : "memory");
                else asm volatile("global_load_ubyte %0, %1, %2" : "=v"(B.cz[v][h]) : "v"(zlane), "s"(csrc) : "memory");
            }
        }
    };
    // DMAs [i0, i1) of chunk c's rows (every plane) into buffer b
    auto issue_x = [&](int c, int b, int i0, int i1) __attribute__((always_inline)) {
        const char* xsrc = (const char*)p.a + (size_t)c * 256;
        const unsigned l0 = __builtin_amdgcn_readfirstlane(xbuf_lds + (unsigned)(b * planes * XB));
#pragma unroll
        for (int i = i0; i < i1; ++i) {
            const unsigned xo = xoff[i];
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(l0 + (unsigned)(i * 1024)), "v"(xo), "s"(xsrc) : "memory");
            if (planes > 1) {
                const char* xsrc1 = xsrc + p.plane_bytes;
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(l0 + (unsigned)(XB + i * 1024)), "v"(xo), "s"(xsrc1) : "memory");
            }
        }
    };
    // the registers pass through a statement behind the wait so that no use of them is scheduled in front of it
    auto claim = [&](Buf& B) __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < NS; ++v)
#pragma unroll
            for (int h = 0; h < NH; ++h) asm volatile("" : "+v"(B.wq[v][h]), "+v"(B.cs[v][h]), "+v"(B.cz[v][h])::"memory");
    };

    f32x4 acc[NS];
#pragma unroll
    for (int v = 0; v < NS; ++v) acc[v] = f32x4{0.f, 0.f, 0.f, 0.f};

    // chunk in buffer b; the NEXT chunk's DMAs (cn, into the other buffer) are issued a quarter at a time behind the MFMAs of each step (gemm_rows_kernel.cuh)
    auto compute = [&](const Buf& B, int b, int cn, bool has_x) __attribute__((always_inline)) {
        typename DeqOf<T, BITS>::type dq[NS][NH];
#pragma unroll
        for (int v = 0; v < NS; ++v)
#pragma unroll
            for (int h = 0; h < NH; ++h) dq[v][h].setup(B.cs[v][h], B.cz[v][h]);
        const char* xb = xbuf + b * planes * XB;
        u32x4 a1[4], a3[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            a1[w] = *(const u32x4*)(xb + aoff[w]);
            a3[w] = *(const u32x4*)(xb + a3off + aoff[w]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
#pragma unroll
            for (int v = 0; v < NS; ++v) {
                u32x4 bq;
                if constexpr (BITS == 4) bq = dq[v][0].frag(B.wq[v][0][w]);
                else if constexpr (BITS == 3) bq = dq[v][0].frag(B.wq[v][0], w);
                else if constexpr (BITS == 2) bq = dq[v][0].frag(B.wq[v][0][w >> 1] >> (8 * (w & 1)));
                else bq = dq[v][w >> 1].frag(B.wq[v][w >> 1][2 * (w & 1)], B.wq[v][w >> 1][2 * (w & 1) + 1]);
                acc[v] = Mma16<T>::run(v < NS / 2 ? a1[w] : a3[w], bq, acc[v]);
            }
            if (has_x) issue_x(cn, b ^ 1, w, w + 1);
        }
    };

    if (c0 < c1) {
#pragma unroll
        for (int j = 0; j < DW; ++j)
            if (c0 + j < c1) issue_w(c0 + j, q[j]);
        issue_x(c0, 0, 0, NDMA);
        for (int cbase = c0; cbase < c1; cbase += DW) {
#pragma unroll
            for (int j = 0; j < DW; ++j) {
                const int c = cbase + j;
                if (c >= c1) break;
                // VMEM queue, oldest first: W(c0 .. c0 + DW - 1), x(c0) | x(c0 + 1) under the MFMAs of c0, W(c0 + DW) | x(c0 + 2), W(c0 + DW + 1) | ...
                // chunk c needs x(c) and everything older (W(c) is); behind x(c) there is only W(c + DW - 1), issued at the end of the previous iteration
                // W(.) is NW instructions at every width: per strip and half one weight load (dwordx4 / x3 at 3 bits / x2 at 2 bits -- the ring element is
                // that load's whole destination), one ushort of scale, one ubyte / ushort of zero-point = 3 NH NS: 12 at 2, 3 and 4 bits, 24 at 8.  vmcnt(NW)
                // therefore leaves exactly W(c + DW - 1) in flight; the first chunk and the last DW - 1 (no younger W behind their x) wait for everything
                const bool has_w = c > c0 && c + DW - 1 < c1;
                if (has_w) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                claim(q[j]);
                compute(q[j], j & 1, c + 1, c + 1 < c1);
                if (c + DW < c1) issue_w(c + DW, q[j]);
            }
        }
    }
    // every destination register of the ring passes through a statement behind a full wait: nothing is in flight into a register the epilogue reuses
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < DW; ++j) claim(q[j]);

    // ---- the waves' sums meet in LDS (wave order), epilogue, store ------------------------------------------------------------------------------
    __syncthreads();                                           // every wave is done with its x buffers
    float* const red = (float*)smem;                           // [wave][v][lane] float4
#pragma unroll
    for (int v = 0; v < NS; ++v) *(f32x4*)(red + ((size_t)(wave * NS + v) * 64 + lane) * 4) = acc[v];
    __syncthreads();
    auto wsum = [&](int v, int l) -> f32x4 {
        f32x4 s = *(const f32x4*)(red + ((size_t)v * 64 + l) * 4);
        for (int w = 1; w < nw; ++w) s += *(const f32x4*)(red + ((size_t)(w * NS + v) * 64 + l) * 4);
        return s;
    };
    const int N = p.N;
    for (int item = tid; item < S * 64; item += (int)blockDim.x) {
        const int l = item & 63, v = item >> 6;
        const int n = (s0 + v) * 16 + (l & 15);
        const f32x4 sg = wsum(v, l);
        if constexpr (BITS == 2) {
            if (dense) {
                const float b = p.dense_bias ? DType<T>::to_f32(((const T*)p.dense_bias)[n]) : 0.f;      // (a 2-byte load: no dwordx4 in this kernel but the x DMAs)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = 4 * (l >> 4) + i;
                    if (row < rows) ((T*)p.out)[(size_t)(row0 + row) * N + n] = DType<T>::from_f32(sg[i] + b);
                }
                continue;
            }
        }
        if (PAIR) {
            const f32x4 su = wsum(v + NS / 2, l);
#pragma unroll
            for (int i = 0; i < 4; ++i) {                      // C/D layout of the 16x16 MFMA: row = 4 (lane >> 4) + i, column = lane & 15
                const int row = 4 * (l >> 4) + i;
                const float gv = sg[i];
                if (row < rows) ((T*)p.out)[(size_t)(row0 + row) * N + n] = DType<T>::from_f32(gv / (1.f + __expf(-gv)) * su[i]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 4 * (l >> 4) + i;
                if (row < rows) ((float*)p.out)[(size_t)(row0 + row) * N + n] = sg[i];
            }
        }
    }
#undef PAIR
