// gemv_tiled_kernel.cuh -- the decode-copy kernel and its launch templates, included by four translation units: gemv_tiled.hip (plain layers, XM = 0),
// gemv_tiled_act.hip (act-order layers, XM = 1), gemv_tiled_peer.hip (plain layers with the tensor-parallel epilogue, XM = 3) and gemv_tiled_pair.hip
// ([gate | up] layers with the fused SiLU * mul epilogue, XM = 4) -- separate only for build time, and so that the plain kernels carry nothing of the
// other forms.  Description: gemv_tiled.hip.
#pragma once
#include <cstddef>

#include "gemv_shared.cuh"

namespace gptq {

// Kernel arguments, laid out for a short head: everything a workgroup needs to form its first weight address and to issue its x and constant DMAs
// -- the layer boundaries, the geometry, and the weight / constant pointers of ALL four layers -- sits in the first 128 bytes and is loaded in ONE batch of scalar
// loads at entry; the layer is then chosen by scalar compares and selects, no load is indexed by it in front of the first weight load.  What only the tail
// and the bias request need of the layer (TiledSeg) is one dependent load issued BEHIND the first weight burst; the K-slice words and the tensor-parallel
// epilogue lie behind that.  (Before: the layer's pointers were a second, dependent scalar-load round trip in front of the weight loads; the first version
// walked GemvStreamParams::seg[] with a dependent kernarg load per step and divided by ksplit: five round trips, ~1 us per launch against the lab kernel.)
struct TiledSeg {
    const void* bias;
    void* out;
    int N, col0;             // columns of this layer; its first column in the concatenated partial slab
};
// Tensor-parallel epilogue (gptq_forward_scatter; protocol: peer.hip): the owner workgroup of a strip stores its [M][16] outputs at the rank's column
// offset of EVERY rank's exchange buffer of this call's parity; the rank's arrival flag is raised by the collect launch behind this kernel.
struct PeerEpi {
    char* xbuf[2][GPTQ_PEER_MAX];
    unsigned* flags[GPTQ_PEER_MAX];
    unsigned* state;         // [0] gathers completed (the epoch)
    int world, rank;
    unsigned row_bytes, col_off_bytes, owners, pad_;
};
struct TiledParams {
    // ---- bytes 0 .. 127: the entry batch
    int blk_end[3];          // cumulative strip count up to and including layer i (unused entries: INT_MAX); a fourth layer is reached by the first three compares
    int act;                 // PAIR kernels: the gptq_epilogue_t of the layer (gated_act; is_plain_act: split mode, both halves stored) -- in the entry batch, in the word no kernel read (it held blk_end[3] = INT_MAX)
    const void* x;
    int M, K;
    int chunks, chunks_per_split, ksplit, gu_shift, groups, xstride, waves;
    union {
        int pair_strips;     // PAIR kernels: strips of one half of the [gate | up] layer (N / 32)
        unsigned xstep1;     // plain 4-bit fp16 kernels: 0 = x and the constants are staged in ONE step; else what the first of TWO steps stages, in 16-byte pieces --
    };                       // bits 0..15 of a row of x (the workgroup's first pass: waves * U chunks), bits 16..31 of the constants (the groups that range touches)
    const unsigned* tq[4];   // qweight_tiled of layer i
    const void* cst[4];      // qconst_tiled
    // ---- act-order kernels: part of their entry batch
    const int* perm[4];      // x position i of the copy = x[perm[i]]
    int xraw_off;            // byte offset of the raw x rows (whole K, row stride 2 K + 16) in the dynamic LDS
    // ---- behind the first weight burst / cold
    int nseg, nsum;
    unsigned max_spins;
    TiledSeg seg[4];
    unsigned long long* gran;   // K-split exchange granules (stream_finish)
    unsigned* epochs;
    unsigned* err;
    PeerEpi peer;            // XM = 3 kernels only: read by the owner workgroups behind their K loop
};
static_assert(offsetof(TiledParams, perm) == 128, "the entry batch of the decode-copy kernel is the first two cache lines of its arguments");

// Per packing: what a lane of one chunk load holds.  The chunk is always 4 k-slots x 16 columns; a lane (k-slot, column) holds WPL consecutive words =
// KPL consecutive k of ONE column, re-encoded at load time (gptq_prepack_decode) so that the packed fp16 magic-number extraction yields the k pairs in
// the order x lies in memory:
//   4-bit  4 words = 32 k; stored nibbles k0 k2 k4 k6 k1 k3 k5 k7 per word
//   8-bit  4 words = 16 k; stored bytes   k0 k2 k1 k3 per word
//   3-bit  3 words = 32 k (one packing unit, re-encoded without straddlers): word j holds the pairs p = 5 j + i (i = 0..4) = (k 2p, k 2p + 1) at bit 3 i of
//          its low / high half; bits 15 and 31 of the three words are the bits of k30 / k31.
template <int BITS> struct TiledFmt;
template <> struct TiledFmt<4> { static constexpr int WPL = 4, KPL = 32, REC = 48, ZB = 1; };
template <> struct TiledFmt<8> { static constexpr int WPL = 4, KPL = 16, REC = 64, ZB = 2; };
template <> struct TiledFmt<3> { static constexpr int WPL = 3, KPL = 32, REC = 48, ZB = 1; };
template <> struct TiledFmt<2> { static constexpr int WPL = 2, KPL = 32, REC = 48, ZB = 1; };      // (round 6) 2 words = 32 k; word w: pair p = (k 16w + 2p, k 16w + 2p + 1) at bit 2p of its halves

// Lab (tools/ab_tiled.sh STAMPS -DGPTQ_TILED_STAMPS -> tools/libgptq_STAMPS.so, read by tools/tail_timeline.py; never in the product library): every wave of four
// workgroups of an unsplit launch keeps s_memtime (shader cycles; a per-XCD counter: only differences on one wave's own clock mean anything) at 0 entry,
// 1 first weight loads issued, 2 staging barrier passed, 3 last weight chunk landed, 4 K loop left, 5 reduction barrier passed, 6 output store issued,
// and s_memrealtime (100 MHz) at entry and exit for the clock; lane 0 writes them with ordinary vector stores to the buffer the lab launch code puts in p.gran.
#ifdef GPTQ_TILED_STAMPS
#define TILED_STAMP(i) (st_[i] = __builtin_amdgcn_s_memtime() | vz_)          /* (| a zero the compiler cannot see: the stamp is a vector value from the start -- kept scalar across divergent code, hipcc of ROCm 7.2 ends in "illegal VGPR to SGPR copy") */
#define TILED_STAMPS_OUT() stamps_out()
#define TILED_HOT_END() return                                                    /* (the stamp stores in front of an s_endpgm in the middle of the kernel: hipcc of ROCm 7.2 fails in the backend) */
#else
#define TILED_HOT_END() __builtin_amdgcn_endpgm()
#define TILED_STAMP(i) ((void)0)
#define TILED_STAMPS_OUT() ((void)0)
#endif

template <int N_> struct WordsOf { typedef unsigned type __attribute__((ext_vector_type(N_))); };

// XM = 1 (ACT): an act-order layer -- the decode copy holds the re-sequenced rows (position i = original k perm[i], groups in sequence); the workgroup DMAs the raw
// x rows (whole K) into the LDS and gathers its slice through perm LDS -> LDS (one more barrier; + M (2 K + 16) bytes of LDS); the rest is the plain kernel.
// (XM = 2 was a GATED form -- the down projection of an MLP forming silu(g) * u while staging its input: correct, and no faster than the elementwise launch it
// removed (20.6 against 20.0 us per Llama-7B MLP: every workgroup repeats the activation); not kept.)
// FL (flags; the kernels' names keep seven arguments -- the ISA tests and the tools find them by their full names): bit 0 = ZM2 (below), bit 1 = AL, the ALIGNED
// form of the K loop: K is a whole number of chunks, so no k-slot is missing, no group index needs a clamp, and every LDS address of a chunk is
// a lane constant set up in front of the loop plus a scalar of the chunk (TiledPlan.aligned).
template <int BITS, int MT, int U, typename T, int MAXW, int XM = 0, int FL = 0>
__global__ void __launch_bounds__(MAXW * 64, MAXW == 16 ? 4 : 2) gemv_tiled_kernel(TiledParams p) {
    constexpr int ZM2 = FL & 1;
    constexpr bool BF_ = std::is_same_v<T, bf16>;
    // Lab (tools/ab_tiled.sh ABLn -DGPTQ_TILED_ABL=n; timing only, the outputs are WRONG by design; never in the product library; fp16 4-bit forms): bit 1 = every
    // kernel takes the aligned form's addressing, 2 = no decode (raw words to the matrix core), 4 = no x reads from the LDS, 8 = no matrix-core steps.
#ifdef GPTQ_TILED_ABL
    constexpr int ABL = GPTQ_TILED_ABL;
#else
    constexpr int ABL = 0;
#endif
    constexpr bool AL = (FL & 2) != 0 || (ABL & 1) != 0;
#ifdef GPTQ_TILED_STAMPS
    unsigned long long st_[9] = {};
    unsigned vz_;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz_));
    st_[7] = __builtin_amdgcn_s_memrealtime() | vz_;
    TILED_STAMP(0);
    auto stamps_out = [&]() {
        st_[8] = __builtin_amdgcn_s_memrealtime() | vz_;
        unsigned long long* const dbg = p.gran;
        const int b = (int)blockIdx.x, nb = (int)gridDim.x;
        const int slot = b == 0 ? 0 : (b == 1 ? 1 : (b == nb / 2 ? 2 : (b == nb - 1 ? 3 : -1)));
        if (dbg != nullptr && p.ksplit == 1 && slot >= 0 && (threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) dbg[(slot * 16 + (int)(threadIdx.x >> 6)) * 16 + i] = st_[i];
        }
    };
#endif
    constexpr bool BF = std::is_same_v<T, bf16>;
    constexpr bool ACT = XM == 1, PEER = XM == 3;          // 3: plain staging + the tensor-parallel epilogue (gemv_tiled_peer.hip)
    // XM = 4 (PAIR, round 5): a [gate | up] layer with the SILU_MUL epilogue (the reference's fused MLP: auto_gptq/nn_modules/fused_llama_mlp.py:131-306).  A
    // workgroup takes strip s of the gate half AND strip s of the up half (N / 32 strips further) behind ONE staged x: the first half of its waves
    // streams the one, the second half the other; act(gate) * up (SiLU or tanh-GELU: p.act) is formed on the fp32 sums behind the cross-wave reduction (no K slices: the planner).
    constexpr bool PAIR = XM == 4;
    // XM = 5 / 6 (MULTI, round 5): FOUR / TWO adjacent strips of a layer per workgroup behind ONE staged x -- the 5..8-row form staged 64 KiB of x per
    // 16-column strip (K = 4096), which the per-CU L2 pull rate (~50 GB/s, profiles/r03_xfetch_lab.log) turned into microseconds on layers of hundreds of
    // strips; the waves split into NSTR groups, one per strip, and the cross-wave sum is per strip (no K slices: the planner).
    constexpr bool MULTI = XM == 5 || XM == 6;
    constexpr int NSTR = PAIR ? 2 : (XM == 5 ? 4 : (XM == 6 ? 2 : 1));            // strips per workgroup
    using F = TiledFmt<BITS>;
    constexpr int WPL = F::WPL, KPL = F::KPL, CKE = 4 * KPL, CHB = 64 * WPL * 4, REC = F::REC, NX = KPL / 8;      // k per chunk, bytes per chunk, x pieces per lane and chunk
    constexpr int LKPL = KPL == 32 ? 5 : 4;
    typedef typename WordsOf<WPL>::type qvec;
    unsigned m_lo, m_hi, m_b, magic;                                              // opaque constants: (q & mask) | magic is ONE v_and_or_b32 (gemv.hip)
    asm("s_mov_b32 %0, 0x000f000f" : "=s"(m_lo));
    asm("s_mov_b32 %0, 0x00f000f0" : "=s"(m_hi));
    asm("s_mov_b32 %0, 0x00ff00ff" : "=s"(m_b));
    asm("v_mov_b32 %0, 0x64006400" : "=v"(magic));
    unsigned m2a, m2b, m2c, m2d, m2e;
    asm("s_mov_b32 %0, 0x00030003" : "=s"(m2a));
    asm("s_mov_b32 %0, 0x000c000c" : "=s"(m2b));
    asm("s_mov_b32 %0, 0x00300030" : "=s"(m2c));
    asm("s_mov_b32 %0, 0x00c000c0" : "=s"(m2d));
    asm("s_mov_b32 %0, 0x03000300" : "=s"(m2e));
    unsigned m3a, m3b, m3c;
    asm("s_mov_b32 %0, 0x00070007" : "=s"(m3a));
    asm("s_mov_b32 %0, 0x00380038" : "=s"(m3b));
    asm("s_mov_b32 %0, 0x01c001c0" : "=s"(m3c));
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                    // scalar: the staging loops below are scalar loops
    const int col = lane & 15, kb = lane >> 4;                                    // lane = kb * 16 + col: lane-linear inside the chunk
    // Everything the head needs: the first 128 bytes of the kernel arguments, in ONE batch of two scalar loads and ONE wait -- issued by hand, so that the words
    // are used where the loads put them.  (Left to itself the compiler loads kernel arguments one dependent step at a time; pinned by an empty asm, as here
    // before, the batch held, and ~25 s_mov copied its words out of the load tuples.)  The words the K loop and the tail need stay in these SGPRs.
    typedef unsigned u32x16 __attribute__((ext_vector_type(16)));
    typedef unsigned long long u64x8 __attribute__((ext_vector_type(8)));
    typedef unsigned long long u64x4 __attribute__((ext_vector_type(4)));
    static_assert(offsetof(TiledParams, x) == 16 && offsetof(TiledParams, M) == 24 && offsetof(TiledParams, chunks) == 32 && offsetof(TiledParams, pair_strips) == 60 &&
                  offsetof(TiledParams, tq) == 64 && offsetof(TiledParams, cst) == 96 && offsetof(TiledParams, perm) == 128 && offsetof(TiledParams, xraw_off) == 160 && offsetof(TiledParams, act) == 12, "the entry batch");
    u32x16 ha;                                                                    // blk_end[3], act, x, M, K, chunks, chunks_per_split, ksplit, gu_shift, groups, xstride, waves, pair_strips
    u64x8 hb;                                                                     // tq[4], cst[4]
    [[maybe_unused]] u64x4 hp = {};                                               // ACT: perm[4]
    [[maybe_unused]] int xraw_off = 0;
    {
        const auto kargs = __builtin_amdgcn_kernarg_segment_ptr();      // (p is the kernel's only parameter: offset 0)
        if constexpr (ACT)
            asm volatile("s_load_dwordx16 %0, %4, 0x0\n\ts_load_dwordx16 %1, %4, 0x40\n\ts_load_dwordx8 %2, %4, 0x80\n\ts_load_dword %3, %4, 0xa0\n\ts_waitcnt lgkmcnt(0)"
                         : "=&s"(ha), "=&s"(hb), "=&s"(hp), "=&s"(xraw_off) : "s"(kargs));
        else
            asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)" : "=&s"(ha), "=&s"(hb) : "s"(kargs));
    }
    const int be0 = (int)ha[0], be1 = (int)ha[1], be2 = (int)ha[2], Mrows = (int)ha[6], K = (int)ha[7], nchunks = (int)ha[8], cps = (int)ha[9], ksplit = (int)ha[10],
              gshift = (int)ha[11], G = (int)ha[12], xstride = (int)ha[13], W = (int)ha[14];
    [[maybe_unused]] const int hstrips = (int)ha[15], act = (int)ha[3];           // PAIR: strips of one half; the activation of the epilogue
    // Two-step staging: a launch deeper than one pass of its workgroup stages in front of the first weight burst only what the first pass reads; the
    // rest of x and of the constants follows BEHIND the staging barrier and is in the LDS by a second barrier in front of the second pass.  The planner's word
    // (TiledPlan.xsteps): 0 = one step -- such a launch runs what it ran before plus two selects in the head and two compares on this word.
#if defined(GPTQ_TILED_NO_ROLL) || defined(GPTQ_TILED_WEIGHTS_FIRST)                   // (lab loops without the second barrier: every launch stages in one step)
    constexpr bool TWO = false;
#else
    constexpr bool TWO = XM == 0 && BITS == 4 && !BF_;
#endif
    [[maybe_unused]] const unsigned xstep1 = TWO ? ha[15] : 0u;
    typedef __attribute__((address_space(1))) const char gchar;                   // (behind the asm the compiler no longer knows that these are global pointers)
    gchar* const xg = (gchar*)(((unsigned long long)ha[5] << 32) | ha[4]);
    // workgroup -> (strip over all layers, K slice); no XCD remap: strips share nothing but x, which every L2 holds.  A launch without K slices (every launch of
    // the Llama decode step) pays one compare: the division and the slice's chunk / k range are a cold block
    int sidx = blockIdx.x, ks = 0, cb = 0, ce = nchunks, kbeg = 0, kend = K;      // (no slices: chunks_per_split = chunks)
    if (__builtin_expect(ksplit != 1, 0)) {
        sidx = (int)blockIdx.x / ksplit; ks = (int)blockIdx.x - sidx * ksplit;
        cb = ks * cps; ce = min(cb + cps, nchunks);                               // this slice's chunks
        kbeg = cb * CKE; kend = min(ce * CKE, K);                                 // ... and its k range: what is staged of x
    }
    // the layer: scalar compares on entry-loaded words, everything of it the head needs chosen by s_cselect (blk_end is cumulative, unused entries INT_MAX: the
    // compares are nested, and a workgroup of the first layer -- every workgroup of a one-layer launch -- leaves behind the first).  In asm on purpose: written
    // as C++ selects, the compiler keeps each compare as a lane mask with several users and selects on the VECTOR unit (v_cndmask_b32 + v_readfirstlane_b32
    // -- or fails with "illegal VGPR to SGPR copy" where the result feeds an "s" operand).
    unsigned long long tqs_ = hb[0], csts_ = hb[4];
    [[maybe_unused]] unsigned long long perm_ = hp[0];
    int sbase = 0, s = 0;
    if constexpr (ACT)
        asm("s_cmp_ge_i32 %[i], %[e0]\n\ts_cbranch_scc0 1f\n\t"
            "s_mov_b64 %[tq], %[tq1]\n\ts_mov_b64 %[cs], %[cs1]\n\ts_mov_b64 %[pm], %[pm1]\n\ts_mov_b32 %[sb], %[e0]\n\ts_mov_b32 %[s], 1\n\t"
            "s_cmp_ge_i32 %[i], %[e1]\n\ts_cselect_b64 %[tq], %[tq2], %[tq]\n\ts_cselect_b64 %[cs], %[cs2], %[cs]\n\ts_cselect_b64 %[pm], %[pm2], %[pm]\n\ts_cselect_b32 %[sb], %[e1], %[sb]\n\ts_cselect_b32 %[s], 2, %[s]\n\t"
            "s_cmp_ge_i32 %[i], %[e2]\n\ts_cselect_b64 %[tq], %[tq3], %[tq]\n\ts_cselect_b64 %[cs], %[cs3], %[cs]\n\ts_cselect_b64 %[pm], %[pm3], %[pm]\n\ts_cselect_b32 %[sb], %[e2], %[sb]\n\ts_cselect_b32 %[s], 3, %[s]\n"
            "1:"
            : [tq] "+&s"(tqs_), [cs] "+&s"(csts_), [pm] "+&s"(perm_), [sb] "+&s"(sbase), [s] "+&s"(s)
            : [i] "s"(sidx), [e0] "s"(be0), [e1] "s"(be1), [e2] "s"(be2), [tq1] "s"(hb[1]), [tq2] "s"(hb[2]), [tq3] "s"(hb[3]), [cs1] "s"(hb[5]), [cs2] "s"(hb[6]), [cs3] "s"(hb[7]),
              [pm1] "s"(hp[1]), [pm2] "s"(hp[2]), [pm3] "s"(hp[3])
            : "scc");
    else
        asm("s_cmp_ge_i32 %[i], %[e0]\n\ts_cbranch_scc0 1f\n\t"
            "s_mov_b64 %[tq], %[tq1]\n\ts_mov_b64 %[cs], %[cs1]\n\ts_mov_b32 %[sb], %[e0]\n\ts_mov_b32 %[s], 1\n\t"
            "s_cmp_ge_i32 %[i], %[e1]\n\ts_cselect_b64 %[tq], %[tq2], %[tq]\n\ts_cselect_b64 %[cs], %[cs2], %[cs]\n\ts_cselect_b32 %[sb], %[e1], %[sb]\n\ts_cselect_b32 %[s], 2, %[s]\n\t"
            "s_cmp_ge_i32 %[i], %[e2]\n\ts_cselect_b64 %[tq], %[tq3], %[tq]\n\ts_cselect_b64 %[cs], %[cs3], %[cs]\n\ts_cselect_b32 %[sb], %[e2], %[sb]\n\ts_cselect_b32 %[s], 3, %[s]\n"
            "1:"
            : [tq] "+&s"(tqs_), [cs] "+&s"(csts_), [sb] "+&s"(sbase), [s] "+&s"(s)
            : [i] "s"(sidx), [e0] "s"(be0), [e1] "s"(be1), [e2] "s"(be2), [tq1] "s"(hb[1]), [tq2] "s"(hb[2]), [tq3] "s"(hb[3]), [cs1] "s"(hb[5]), [cs2] "s"(hb[6]), [cs3] "s"(hb[7])
            : "scc");
    gchar* const tqs = (gchar*)tqs_;
    gchar* const csts = (gchar*)csts_;
    [[maybe_unused]] const int* const permp = (const int*)perm_;                  // ACT: the layer's perm, its words requested in front of the weight loads
    const int strip = sidx - sbase;
    const int Wh = NSTR == 4 ? (W >> 2) : (NSTR == 2 ? (W >> 1) : W);             // waves per strip
    const int sel = NSTR == 1 ? 0 : (scalar_ge(wave, Wh) + (NSTR == 4 ? scalar_ge(wave, 2 * Wh) + scalar_ge(wave, 3 * Wh) : 0));      // which of the workgroup's strips (wave-uniform); PAIR: 0 = gate, 1 = up
    const int wv = NSTR == 1 ? wave : wave - sel * Wh;
    const int strip_w = PAIR ? strip + sel * hstrips : (MULTI ? strip * NSTR + sel : strip);      // the strip this WAVE streams
    // LDS: [x: MT rows of (kend - kbeg) values, row stride + 16 B][constants: G x REC bytes][cross-wave sums]
    char* const xs = smem;                                                        // row stride xstride = chunks_per_split * CKE * 2 + 16 bytes: the 4 rows of a 4-lane group hit different banks
    char* const cs = smem + (size_t)MT * xstride;
    const unsigned crec = (unsigned)G * (unsigned)REC;                            // bytes of one strip's constants
    const size_t cpad = ((size_t)crec + 15) & ~(size_t)15;
    float* const red = (float*)(cs + NSTR * cpad);
    gchar* const tb = tqs + (size_t)(unsigned)strip_w * ((unsigned)nchunks * (unsigned)CHB);      // this wave's strip of weights: one contiguous run
    gchar* const cg = csts + (size_t)(unsigned)(MULTI ? strip * NSTR : strip) * crec;             // this strip's (MULTI: these strips') constants: one contiguous run
    const unsigned t_lane = (unsigned)lane * (WPL * 4u);
    [[maybe_unused]] unsigned tlv = t_lane;                                       // AL: the same offset, as the weight loads' only vector operand (wload)
    // ---- stage x and the constants by LDS DMA: no VGPRs, issued FIRST (loads return in issue order), waited for behind the first weight burst.  Every DMA of a
    // thread takes a scalar base and a 32-bit lane offset; a wave without a piece skips a block on one scalar compare (stage_rows)
    auto stage_all = [&]() __attribute__((always_inline)) {
        const unsigned xs_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)xs, cs_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)cs;
        const int w64 = wave * 64, step = W * 64;
        gchar* xrow[MT];
        unsigned xdst[MT];
        if constexpr (XM == 0 || XM == 3 || XM == 4 || MULTI) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                xrow[m] = xg + (unsigned)((m == 0 ? 0 : min(m, Mrows - 1)) * K + kbeg) * 2u;
                xdst[m] = xs_lds + m * xstride;
            }
#ifdef GPTQ_TILED_STAGE1                                                           // lab (tools/ab_tiled.sh STAGE1; timing only, the outputs are WRONG by design): only what the first pass reads is staged
            stage_rows<MT, false>(xrow, xdst, tid, w64, step, min(kend - kbeg, Wh * U * CKE) >> 3);
#else
            int xpieces = (kend - kbeg) >> 3;
            if constexpr (TWO) xpieces = scalar_sel_nz(xstep1, (int)(xstep1 & 0xffffu), xpieces);      // two steps: the first pass's part of every row
            stage_rows<MT, false>(xrow, xdst, tid, w64, step, xpieces);         // default cache policy: every workgroup reads x
#endif
        } else if constexpr (ACT) {
            // act-order: the RAW rows, whole K (a slice's positions map to any original k), by the same DMA; the gather through perm is LDS -> LDS
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                xrow[m] = xg + (unsigned)((m == 0 ? 0 : min(m, Mrows - 1)) * K) * 2u;
                xdst[m] = xs_lds + (unsigned)xraw_off + m * (K * 2 + 16);
            }
            stage_rows<MT, false>(xrow, xdst, tid, w64, step, K >> 3);
        }
#ifdef GPTQ_TILED_STAGE1                                                           // (the byte count of the first pass's groups; multi-strip forms: not where the strips' records lie)
        const int cpieces = (ACT ? G : min(G, ((min(kend - kbeg, Wh * U * CKE) - 1) >> LKPL >> gshift) + 1)) * (REC >> 4) * (MULTI ? NSTR : 1);
#else
        int cpieces = (int)(crec >> 4) * (MULTI ? NSTR : 1);                      // REC is a multiple of 16 (MULTI: adjacent strips' records are adjacent, cpad = G * REC)
        if constexpr (TWO) cpieces = scalar_sel_nz(xstep1, (int)(xstep1 >> 16), cpieces);          // two steps: the records of the groups the first pass touches
#endif
        if constexpr (PAIR) {                                                     // the up strip's constants behind the gate strip's
            gchar* const crow[2] = {cg, cg + (size_t)(unsigned)hstrips * crec};
            const unsigned cdst[2] = {cs_lds, cs_lds + (unsigned)cpad};
            stage_rows<2, true>(crow, cdst, tid, w64, step, cpieces);
        } else {
            gchar* const crow[1] = {cg};
            const unsigned cdst[1] = {cs_lds};
            stage_rows<1, true>(crow, cdst, tid, w64, step, cpieces);
        }
    };
    // Step 2 of a two-step launch (xstep1 != 0; no K slices: kbeg = 0, kend = K): the rest of every row of x and of the constants, to the places the one-step launch
    // puts them, by the same DMAs over all waves, issued BEHIND the staging barrier -- so behind the first weight burst, and older than every refill: a wave's loads
    // return in issue order, so the wait in front of the wave's LAST first-pass chunk retires its step-2 DMAs, and the earlier chunks of the pass are decoded, and
    // their registers refilled, while step 2 is still on its way.
    // (Measured and not taken, profiles/two_step_staging_ab.log: step 2 by the last quarter of the waves only, so that the others never wait for a DMA -- 1.2 %
    // SLOWER than the one-step launch; step 2 in front of the staging barrier with a counted wait that leaves it in flight -- no gain over the one-step launch.)
    auto stage_rest = [&]() __attribute__((always_inline)) {
        if constexpr (TWO) {
            const unsigned xs_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)xs, cs_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)cs;
            const int w64 = wave * 64, step = W * 64;
            const int xp1 = (int)(xstep1 & 0xffffu), cp1 = (int)(xstep1 >> 16);  // pieces of step 1: per row of x, of the constants
            const int xp2 = (K >> 3) - xp1, cp2 = (int)(crec >> 4) - cp1;         // ... and of step 2
            gchar* xrow[MT];
            unsigned xdst[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                xrow[m] = xg + ((unsigned)((m == 0 ? 0 : min(m, Mrows - 1)) * K) * 2u + (unsigned)xp1 * 16u);
                xdst[m] = xs_lds + m * xstride + (unsigned)xp1 * 16u;
            }
            stage_rows<MT, false>(xrow, xdst, tid, w64, step, xp2);
            gchar* const crow[1] = {cg + (unsigned)cp1 * 16u};
            const unsigned cdst[1] = {cs_lds + (unsigned)cp1 * 16u};
            stage_rows<1, true>(crow, cdst, tid, w64, step, cp2);
        }
    };
#ifndef GPTQ_TILED_WEIGHTS_FIRST
    stage_all();
#endif
    // ACT: one thread = one 16-byte piece of the staged rows: 8 consecutive positions -> 32 contiguous bytes of perm (global, requested HERE, in front of the
    // weight loads), then 8 two-byte LDS reads per row from the raw x the DMA above delivers.  (Gathering x from global instead -- 8 scattered 2-byte
    // loads per piece, by every workgroup -- cost 1.2 - 3 us per launch: profiles/r04_tiled_sweep_act_global_gather.log.)
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    i32x4 pa[2][2] = {};
    const int apieces = ACT ? (kend - kbeg) >> 3 : 0;
    if constexpr (ACT) {
        const int* const pg = permp + kbeg;
        if (tid < apieces) { pa[0][0] = *(const i32x4*)(pg + tid * 8); pa[0][1] = *(const i32x4*)(pg + tid * 8 + 4); }
        if (tid + W * 64 < apieces) { pa[1][0] = *(const i32x4*)(pg + (tid + W * 64) * 8); pa[1][1] = *(const i32x4*)(pg + (tid + W * 64) * 8 + 4); }
    }
    auto x_gather = [&]() {                                                       // behind the barrier that makes the raw rows visible
        const int* const pg = permp + kbeg;
        const char* const xraw = smem + xraw_off;
        for (int pc0 = tid; pc0 < apieces; pc0 += 2 * W * 64) {
            const int pcb = pc0 + W * 64;
            const bool two = pcb < apieces;
            if (pc0 != tid) {                                                     // long K only: further pieces, their perm words loaded here
                pa[0][0] = *(const i32x4*)(pg + pc0 * 8); pa[0][1] = *(const i32x4*)(pg + pc0 * 8 + 4);
                if (two) { pa[1][0] = *(const i32x4*)(pg + pcb * 8); pa[1][1] = *(const i32x4*)(pg + pcb * 8 + 4); }
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const unsigned short* xr = (const unsigned short*)(xraw + (size_t)m * (K * 2 + 16));
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (h == 1 && !two) break;
                    unsigned short v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = xr[pa[h][i >> 2][i & 3]];
                    u32x4 o;
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[i] = (unsigned)v[2 * i] | ((unsigned)v[2 * i + 1] << 16);
                    *(u32x4*)(xs + (size_t)m * xstride + (size_t)(h ? pcb : pc0) * 16) = o;
                }
            }
        }
    };
    // bf16 layers: x is converted IN PLACE in the LDS to fp16 with one power-of-two factor per (row, run of KPL k) -- block floating point -- so that the
    // loop below is the fp16 loop: w - z is a small integer, exact in either type, and turning every fp16 pair into bf16 costs 12 VALU per packed word (the
    // round-3 kernels' 7 - 25 % bf16 gap).  A run is what one lane sums on the matrix core before its fp32 sums meet the scale, so the factor's inverse rides
    // on the scale (xe[run][row]); it puts the run's largest |x| into [2^14, 2^15): nothing overflows (bf16 reaches 3e38, fp16 65504), elements more than
    // 2^-28 below the run's largest lose bits -- below the resolution of the fp32 sum they enter.  Products stay exact (8-bit by 11-bit significands into
    // fp32), as on the bf16 matrix core.  One thread = one 16-byte piece, the NX pieces of a run in adjacent lanes; one more barrier.
    // (Tried instead, same speed at one row and slower at four: one factor per row through an LDS atomic max, and each wave converting its own chunks'
    // x inside the K loop -- profiles/r04_tiled_sweep_bf16_v*.log.)
    // The conversion is done by every workgroup for its whole K slice: at 3 - 4 rows it costs what converting the weights costs, so those keep the bf16
    // matrix core (XC false).
    // Round 5, 4-bit bf16 layers at 1 - 2 rows (XS, instead of XC): neither operand is converted.  (q >> 4 i) & 0x000f000f OR-ed with the bf16 pattern of 128 IS the bf16 pair
    // (128 + w_k, 128 + w_k+1) -- 7 VALU per packed word where the fp16 route takes 13 (+ 12 to turn the pairs into bf16 at 3 - 4 rows) -- raw x goes to the bf16
    // matrix core, and the bias is taken out of the fp32 sum of every run: sum x (128 + w) - (128 + z) sum x = sum x (w - z), with the run sums of x (xe[run][row],
    // fp32) formed ONCE per workgroup behind the staging barrier (a read-only pass: cheaper than the block-floating rewrite).  Products are exact in fp32; the
    // cancellation costs log2(143 / 8) ~ 4 of the fp32 sum's 24 bits, far below bf16's 8; a one-hot row still returns (128 + w) - (128 + z) = w - z exactly.
    // Same-session A/B against the round-4 forms (tools/lab/tiled_noxs.sh, profiles/r05_bf16_vs_f16.log; bf16 behind fp16): 1 row 6 - 13 % -> 2 - 7 %, 2 rows
    // 11 - 27 % -> 6 - 17 %; at 3 - 4 rows the per-workgroup pass over x costs more than converting the weight pairs does (13 - 48 % -> 19 - 75 %): those keep
    // the bf16 matrix core with converted weights.
    // Round 6, 4-bit bf16 layers at 3 - 4 rows, and at 2 rows in launches below 1024 workgroups (ZM): the zero-point goes to the matrix core too.  The B operand is the raw biased pair (bias + w_k, bias + w_k+1)
    // -- bias = 128 as bf16, 1024 as fp16: (q >> 4 i) & 0x000f000f | pattern, 7 VALU per packed word -- and a SECOND accumulator chain multiplies the same x
    // by the constant pair -(bias + z): sum x (bias + w) + sum x (-(bias + z)) = sum x (w - z).  No pass over x per workgroup (XS's run sums), no block-floating
    // rewrite (XC), no conversion of decoded pairs (the 3..4-row bf16 form: 25 VALU per word).  A one-hot row returns (bias + w) - (bias + z) = w - z exactly; a
    // layer whose fields equal their zero-points gives exactly 0 (the two chains are the same instruction sequence on negated operands: their sums are exact
    // negatives); everywhere else the cancellation costs log2(bias / 8) bits of the fp32 run sums (4 for bf16, 7 for fp16: 2^-17 relative, below either type's ulp).
    // Same-session A/B (tools/session_r06_zm.sh, profiles/r06_zm_ab.log; us, bf16 product -> this form | fp16): 4 rows 4096^2 5.96 -> 5.24 | 5.2, 4096 -> 11008
    // 10.1 -> 8.4 | 8.4, 11008 -> 4096 11.1 -> 9.0 | 8.7, q|k|v 10.3 -> 8.8 | 8.7, gate|up 16.1 -> 14.2 | 12.6: bf16 19 - 30 % -> 0 - 3 % (gate|up 13 %) behind fp16.
    // NOT at 1 row, nor at 2 rows in launches of 1024+ workgroups (twice the matrix-core instructions: 11 - 17 % slower than the run-sum form on the 1376-strip gate|up launch) and
    // NOT for fp16 (its 13-VALU exact form is faster: 4096 -> 11008 7.2 -> 7.7, gate|up 12.3 -> 14.3).
#if defined(GPTQ_TILED_ZM)                                                          // lab: 1 = bf16 layers at 1..4 rows, 2 = fp16 layers too (A/B builds: tools/ab_tiled.sh)
    constexpr bool ZM = BITS == 4 && MT <= 4 && (GPTQ_TILED_ZM == 2 || (GPTQ_TILED_ZM == 1 && BF));
#else
    constexpr bool ZM = BITS == 4 && BF && (MT == 4 || (MT == 2 && ZM2 == 1));      // 2 rows: where the planner asks (launches below 1024 workgroups: 4096 -> 11008 8.9 -> 8.4 us,
                                                                                    // 11008 -> 4096 9.3 -> 8.2, q|k|v 9.3 -> 8.8; the 1376-strip gate|up launch 13.3 -> 14.8: stays on the run sums)
#endif
#ifdef GPTQ_TILED_NO_XS                                                            // lab: the round-4 bf16 forms (A/B build: tools/lab/tiled_noxs.sh)
    constexpr bool XS = false;
#else
    constexpr bool XS = BF && BITS == 4 && MT <= 2 && !ZM;
#endif
    constexpr bool XC = BF && MT <= 2 && !XS && !ZM;
    using MM = std::conditional_t<XC, f16, T>;                                    // the matrix core's operand type
    constexpr int ES = MT * 16 + 4;
    float* const xe = red + W * ES;                                               // [runs of the slice][4 rows] inverse factors (bf16 layers only; planned for)
    auto x_to_f16 = [&]() {                                                       // every thread of the workgroup, behind the staging barrier
        const int prow = (kend - kbeg) >> 3, total = prow * MT;                   // pieces per row: a multiple of NX, like the thread stride
        for (int i0 = 0; i0 < total; i0 += W * 64) {                             // uniform trip count: the shuffles below need every lane
            const int idx = i0 + tid;
            const bool ok = idx < total;
            int m = 0, pc = ok ? idx : 0;
            if constexpr (MT > 1) { m = pc / prow; pc -= m * prow; }
            u32x4* const at = (u32x4*)(xs + (size_t)m * xstride + (size_t)pc * 16);
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ok) v = *at;
            unsigned mx = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned a = v[i] & 0x7fff7fffu;
                mx = max(mx, max(a & 0xffffu, a >> 16));
            }
            mx = max(mx, (unsigned)__shfl_xor((int)mx, 1, 64));
            if constexpr (NX == 4) mx = max(mx, (unsigned)__shfl_xor((int)mx, 2, 64));
            const int E = (int)((mx >> 7) & 0xffu);                               // biased exponent of the run's largest |x|
            const int ms = min(max(268 - E, 1), 253);                             // 2^(ms - 127): the largest lands in [2^14, 2^15)
            const float mult = __builtin_bit_cast(float, (unsigned)ms << 23);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float lo = __builtin_bit_cast(float, v[i] << 16) * mult, hi = __builtin_bit_cast(float, v[i] & 0xffff0000u) * mult;
                v[i] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(lo, hi));              // exact unless the result is an fp16 subnormal
            }
            if (ok) {
                *at = v;
                if ((pc & (NX - 1)) == 0) xe[(pc / NX) * 4 + m] = __builtin_bit_cast(float, (unsigned)(254 - ms) << 23);
            }
        }
        __syncthreads();
    };
    auto x_sums = [&]() {                                                         // XS: xe[run][row] = the fp32 sum of the run's x; one thread = one 16-byte piece, the NX pieces of a run in adjacent lanes
        const int prow = (kend - kbeg) >> 3, total = prow * MT;
        for (int i0 = 0; i0 < total; i0 += W * 64) {                             // uniform trip count: the shuffles below need every lane
            const int idx = i0 + tid;
            const bool ok = idx < total;
            int m = 0, pc = ok ? idx : 0;
            if constexpr (MT > 1) { m = pc / prow; pc -= m * prow; }
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ok) v = *(const u32x4*)(xs + (size_t)m * xstride + (size_t)pc * 16);
            float sm = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) sm += __builtin_bit_cast(float, v[i] << 16) + __builtin_bit_cast(float, v[i] & 0xffff0000u);
            sm += __shfl_xor(sm, 1, 64);
            if constexpr (NX == 4) sm += __shfl_xor(sm, 2, 64);
            if (ok && (pc & (NX - 1)) == 0) xe[(pc / NX) * 4 + m] = sm;
        }
        __syncthreads();
    };
    const char* const xl = xs + (size_t)min(lane & 3, MT - 1) * xstride + kb * (KPL * 2);    // A operand: lane i of a 4-lane group carries x row i
    const char* const xl2 = xs + (size_t)min(4 + (lane & 3), MT - 1) * xstride + kb * (KPL * 2);   // MT = 8: rows 4..7, a second matrix-core step per decoded pair
    // AL: 32-bit LDS addresses, lane constants.  The group of (chunk c, k-slot kb) is (4 c + kb) >> gu_shift = (4 c >> gu_shift) + (kb >> gu_shift) for every group
    // size >= KPL (a shift <= 2 divides 4 c; a larger one leaves nothing of kb < 4): a scalar of the chunk plus a constant of the lane.
    typedef __attribute__((address_space(3))) const char lchar;
    [[maybe_unused]] lchar* const cl = (lchar*)cs + ((NSTR > 1 ? (unsigned)sel * (unsigned)cpad : 0u) + (unsigned)(kb >> gshift) * (unsigned)REC);
    [[maybe_unused]] lchar* const sl = cl + col * 2;                              // the lane's scale of group 0
    [[maybe_unused]] lchar* const zl = cl + 32 + col * F::ZB;                     // ... and its zero-point
    [[maybe_unused]] lchar* const xll = (lchar*)xl;
    [[maybe_unused]] lchar* const xll2 = (lchar*)xl2;
    [[maybe_unused]] unsigned xpass = 0u;                                         // steady loop: LDS offset of the pass's first chunk of x (one VALU per PASS; the chunks are immediates)
    [[maybe_unused]] unsigned abl_x = 0u;
    if constexpr ((ABL & 4) != 0) asm("v_mov_b32 %0, 0x3c003c00" : "=v"(abl_x));
    float acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.f;
    const f16x2 k960 = {(f16)960.f, (f16)960.f}, k896 = {(f16)896.f, (f16)896.f}, k1008 = {(f16)1008.f, (f16)1008.f};
    const f16x2 r16 = {(f16)0.0625f, (f16)0.0625f}, r8 = {(f16)0.125f, (f16)0.125f}, r64 = {(f16)0.015625f, (f16)0.015625f};
    const f16x2 k768 = {(f16)768.f, (f16)768.f}, k1020 = {(f16)1020.f, (f16)1020.f}, r4 = {(f16)0.25f, (f16)0.25f}, r256 = {(f16)0.00390625f, (f16)0.00390625f};
    auto bits_of = [&](f16x2 hv) -> unsigned {                                    // the pair as the matrix core takes it: fp16 (also bf16 layers behind x_to_f16), or
        if constexpr (BF && !XC) {                                                // fp16 -> fp32 -> bf16 (exact: small integers)
            const bf16x2 o = {(bf16)(float)hv[0], (bf16)(float)hv[1]};
            return __builtin_bit_cast(unsigned, o);
        } else {
            return __builtin_bit_cast(unsigned, hv);
        }
    };
    // the output this thread writes behind an unsplit launch's cross-wave sum (entry = tid: strip of the workgroup, row, column) and its bias, requested in the
    // first pass -- in flight under the whole K loop, not a global round trip behind the last chunk
    constexpr int E = MT * 16, NE = (MULTI ? NSTR : 1) * E;
    const int n_t = (MULTI ? strip * NSTR + tid / E : strip) * 16 + (tid & 15);
    float bv0 = 0.f, bv1 = 0.f;
    // what the tail and the bias request need of the layer: ONE scalar load indexed by the layer, issued behind the first weight burst (the empty asm in front of
    // it: a memory barrier for the compiler that also makes the index opaque, so the load cannot rise above the weight loads), waited for behind the staging
    // barrier.  From there the words stay in SGPRs (pinned like the entry batch: left to itself the compiler fetches them from the kernel-argument segment
    // again BEHIND the K loop -- a dependent scalar-load round trip in front of the store)
    typedef __attribute__((address_space(1))) T gT;
    int N = 0;
    const void* biasp = nullptr;
    void* outp = nullptr;
    auto seg_request = [&]() __attribute__((always_inline)) {
        int sl = s;
        asm volatile("" : "+s"(sl) : : "memory");
        N = p.seg[sl].N; biasp = p.seg[sl].bias; outp = p.seg[sl].out;
    };
    auto seg_pin = [&]() __attribute__((always_inline)) { asm volatile("" : "+s"(N), "+s"(biasp), "+s"(outp)); };
    bool staged = false;
    auto wload = [&](int c) __attribute__((always_inline)) -> qvec {              // chunk c of this wave's strip, clamped into the slice: [cb, ce)
        if constexpr (AL) {                                                       // the chunk in the scalar base, the lane constant as the only vector operand: no VALU
            // (the base's halves through readfirstlane: left visible, the sum is reassociated into (tb + lane offset) + chunk -- a 64-bit vector add per load)
            const unsigned long long sb0 = (unsigned long long)tb + (unsigned long long)((unsigned)min(c, ce - 1) * (unsigned)CHB);
            const unsigned long long sb = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(sb0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)sb0);      // (of a scalar: folded to nothing)
            asm volatile("" : "+v"(tlv));                                         // (pinned per load, in place: hoisted out of the loop, its zero-extension hides the 32-bit offset from instruction selection)
            return __builtin_nontemporal_load((const __attribute__((address_space(1))) qvec*)((gchar*)sb + tlv));
        } else {
            return __builtin_nontemporal_load((const __attribute__((address_space(1))) qvec*)(tb + ((unsigned)min(c, ce - 1) * (unsigned)CHB + t_lane)));
        }
    };
    auto first_pass = [&]() __attribute__((always_inline)) {                      // (uniform): the staging DMAs are OLDER than the U loads just issued
        TILED_STAMP(1);
        seg_request();
#ifdef GPTQ_TILED_WEIGHTS_FIRST                                                    // lab: the DMAs BEHIND the first weight burst -- the staging barrier then waits for the first chunks too
        stage_all();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(U) : "memory");
#endif
        if constexpr (ACT) {
            __syncthreads();                                                  // the raw rows (every wave's DMAs) are in the LDS
            x_gather();
        }
        __syncthreads();
        if constexpr (TWO) {
            if (__builtin_expect(xstep1 != 0u, 0)) stage_rest();            // two steps: younger than the U weight loads in flight, older than every refill
        }
        if constexpr (XC) x_to_f16();
        if constexpr (XS) x_sums();
        seg_pin();
        if (biasp != nullptr && tid < NE && n_t < (PAIR ? N >> 1 : N)) {
            bv0 = DType<T>::to_f32(((const gT*)biasp)[n_t]);
            if constexpr (PAIR) bv1 = DType<T>::to_f32(((const gT*)biasp)[n_t + (N >> 1)]);
        }
        TILED_STAMP(2);
        staged = true;
    };
    // steady (AL only): chunk j of a pass of the steady loop -- alive by the loop's own condition: no clamp, no select, x at an immediate offset from xpass
    auto chunk = [&](auto steady_c, const int cj, [[maybe_unused]] const int j, const qvec qv) __attribute__((always_inline)) {      // decode chunk cj (dead: >= ce) from its words into acc[]
        constexpr bool STEADY = AL && decltype(steady_c)::value;
        const int cc = STEADY ? cj : min(cj, ce - 1);
        bool live;
        unsigned short sraw;
        unsigned z;
        u32x4 xa[NX];
        u32x4 xb[MT > 4 ? NX : 1];
        if constexpr (AL) {
            live = cj < ce;                                                   // wave-uniform: whole chunks only
            const unsigned go = (unsigned)((cc * 4) >> gshift) * (unsigned)REC;      // scalar
            sraw = *(const __attribute__((address_space(3))) unsigned short*)(sl + go);
            if constexpr (F::ZB == 1) z = *(const __attribute__((address_space(3))) unsigned char*)(zl + go);
            else z = *(const __attribute__((address_space(3))) unsigned short*)(zl + go);
            typedef __attribute__((address_space(3))) const u32x4 lx4;
            const unsigned xo = STEADY ? xpass + (unsigned)j * (unsigned)(CKE * 2) : (unsigned)(cc - cb) * (unsigned)(CKE * 2);
            lchar* const xp = STEADY ? (lchar*)(size_t)xo : xll + xo;
#pragma unroll
            for (int w = 0; w < NX; ++w) xa[w] = *(lx4*)(xp + w * 16u);
            if constexpr (MT > 4) {
                lchar* const xp2 = xp + (xll2 - xll);
#pragma unroll
                for (int w = 0; w < NX; ++w) xb[w] = *(lx4*)(xp2 + w * 16u);
            }
        } else {
            const int k0 = cc * CKE + kb * KPL;                               // first k of this lane's words
            live = (cj < ce) && (k0 < K);                                     // a ragged last chunk: whole k-slots are missing
            const int g = min(k0 >> LKPL >> gshift, G - 1);
            const char* cp = cs + (NSTR > 1 ? (size_t)sel * cpad : (size_t)0) + g * REC;
            sraw = *(const unsigned short*)(cp + col * 2);
            if constexpr (F::ZB == 1) z = *(const unsigned char*)(cp + 32 + col);
            else z = *(const unsigned short*)(cp + 32 + col * 2);
#pragma unroll
            for (int w = 0; w < NX; ++w) xa[w] = *(const u32x4*)(xl + ((unsigned)(cc - cb) * (unsigned)(CKE * 2) + w * 16u));
            if constexpr (MT > 4) {
#pragma unroll
                for (int w = 0; w < NX; ++w) xb[w] = *(const u32x4*)(xl2 + ((unsigned)(cc - cb) * (unsigned)(CKE * 2) + w * 16u));
            }
        }
        if constexpr ((ABL & 4) != 0) {
#pragma unroll
            for (int w = 0; w < NX; ++w) xa[w] = u32x4{abl_x, abl_x, abl_x, abl_x};
        }
        const f16x2 c1 = as_f16x2(z * 0x00010001u + 0xE400E400u);            // -(1024 + z)
        f32x4 accg = {0.f, 0.f, 0.f, 0.f}, accg2 = {0.f, 0.f, 0.f, 0.f};
        auto mm = [&](int pc, int hf, unsigned b0, unsigned b1) __attribute__((always_inline)) {      // 4 k of the lane's column against x piece pc, half hf: rows 0..3 (and 4..7)
            if constexpr ((ABL & 8) != 0) { asm volatile("" ::"v"(b0), "v"(b1), "v"(xa[pc][hf * 2]), "v"(xa[pc][hf * 2 + 1])); return; }
            accg = Mma4<MM>::run(u32x2{xa[pc][hf * 2], xa[pc][hf * 2 + 1]}, u32x2{b0, b1}, accg);
            if constexpr (MT > 4) accg2 = Mma4<MM>::run(u32x2{xb[pc][hf * 2], xb[pc][hf * 2 + 1]}, u32x2{b0, b1}, accg2);
        };
        if constexpr (BITS == 4 && ZM) {
            unsigned mgz;
            asm("v_mov_b32 %0, %1" : "=v"(mgz) : "n"(BF ? 0x43004300 : 0x64006400));     // bias twice: bf16 128 / fp16 1024 (ulp 1 in either)
            const unsigned nz = z * 0x00010001u + (BF ? 0xC300C300u : 0xE400E400u);     // -(bias + z) twice (z <= 16: exact)
            f32x4 accz = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const unsigned qw = qv[w];
                mm(w, 0, (qw & m_lo) | mgz, ((qw >> 4) & m_lo) | mgz);                  // (k0, k1) (k2, k3): stored nibbles 0 | 4, 1 | 5
                mm(w, 1, ((qw >> 8) & m_lo) | mgz, ((qw >> 12) & m_lo) | mgz);          // (k4, k5) (k6, k7)
                accz = Mma4<MM>::run(u32x2{xa[w][0], xa[w][1]}, u32x2{nz, nz}, accz);
                accz = Mma4<MM>::run(u32x2{xa[w][2], xa[w][3]}, u32x2{nz, nz}, accz);
            }
            accg += accz;
        } else if constexpr (BITS == 4 && XS) {
            unsigned magicb;
            asm("v_mov_b32 %0, 0x43004300" : "=v"(magicb));                   // bf16 128.0 twice: its 7 mantissa bits take a 4-bit field with an ulp of 1
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const unsigned qw = qv[w];
                mm(w, 0, (qw & m_lo) | magicb, ((qw >> 4) & m_lo) | magicb);            // (k0, k1) (k2, k3): stored nibbles 0 | 4, 1 | 5
                mm(w, 1, ((qw >> 8) & m_lo) | magicb, ((qw >> 12) & m_lo) | magicb);    // (k4, k5) (k6, k7)
            }
        } else if constexpr (BITS == 4) {
            const f16x2 c2 = c1 + k960;                                       // -(64 + z)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const unsigned qw = qv[w], q8 = qw >> 8;
                if constexpr ((ABL & 2) != 0) { mm(w, 0, qw, qw); mm(w, 1, qw, qw); continue; }
                const f16x2 h0 = as_f16x2((qw & m_lo) | magic) + c1;          // k0,k1  (stored nibbles 0 and 4)
                const f16x2 h1 = as_f16x2((qw & m_hi) | magic) * r16 + c2;    // k2,k3  (1 and 5)
                const f16x2 h2 = as_f16x2((q8 & m_lo) | magic) + c1;          // k4,k5  (2 and 6)
                const f16x2 h3 = as_f16x2((q8 & m_hi) | magic) * r16 + c2;    // k6,k7  (3 and 7)
                mm(w, 0, bits_of(h0), bits_of(h1));
                mm(w, 1, bits_of(h2), bits_of(h3));
            }
        } else if constexpr (BITS == 2) {
            // 16 fields per word: the fp16 mantissa takes the five pairs at bits 0..9 in place (1024 + 4^p w, times 4^-p, minus (1024 / 4^p + z): exact), the
            // three at bits 10..15 come down by a shift first -- 17 VALU per 16 k
            const f16x2 c4 = c1 + k768, c16 = c1 + k960, c64 = c1 + k1008, c256 = c1 + k1020;     // -(256 + z), -(64 + z), -(16 + z), -(4 + z)
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const unsigned t = qv[w], t10 = t >> 10;
                const unsigned p0 = bits_of(as_f16x2((t & m2a) | magic) + c1);
                const unsigned p1 = bits_of(as_f16x2((t & m2b) | magic) * r4 + c4);
                const unsigned p2 = bits_of(as_f16x2((t & m2c) | magic) * r16 + c16);
                const unsigned p3 = bits_of(as_f16x2((t & m2d) | magic) * r64 + c64);
                const unsigned p4 = bits_of(as_f16x2((t & m2e) | magic) * r256 + c256);
                const unsigned p5 = bits_of(as_f16x2((t10 & m2a) | magic) + c1);
                const unsigned p6 = bits_of(as_f16x2((t10 & m2b) | magic) * r4 + c4);
                const unsigned p7 = bits_of(as_f16x2((t10 & m2c) | magic) * r16 + c16);
                mm(2 * w, 0, p0, p1);
                mm(2 * w, 1, p2, p3);
                mm(2 * w + 1, 0, p4, p5);
                mm(2 * w + 1, 1, p6, p7);
            }
        } else if constexpr (BITS == 8) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {                                     // one word = 4 k = one matrix-core step
                const unsigned qw = qv[w], q8 = qw >> 8;
                const f16x2 h0 = as_f16x2((qw & m_b) | magic) + c1;           // k0,k1  (stored bytes 0 and 2)
                const f16x2 h1 = as_f16x2((q8 & m_b) | magic) + c1;           // k2,k3  (1 and 3)
                mm(w >> 1, w & 1, bits_of(h0), bits_of(h1));
            }
        } else {
            const f16x2 c3 = c1 + k896;                                       // -(128 + z): fields at bit 3, times 1/8
            const f16x2 c6 = c1 + k1008;                                      // -(16 + z): fields at bit 6, times 1/64
            unsigned pr[16];                                                  // the 16 k pairs of the unit, in k order
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const unsigned t = qv[w], t6 = t >> 6;
                pr[5 * w + 0] = bits_of(as_f16x2((t & m3a) | magic) + c1);
                pr[5 * w + 1] = bits_of(as_f16x2((t & m3b) | magic) * r8 + c3);
                pr[5 * w + 2] = bits_of(as_f16x2((t & m3c) | magic) * r64 + c6);
                pr[5 * w + 3] = bits_of(as_f16x2((t6 & m3b) | magic) * r8 + c3);
                pr[5 * w + 4] = bits_of(as_f16x2((t6 & m3c) | magic) * r64 + c6);
            }
            const unsigned e = ((qv[0] >> 15) & 0x00010001u) | ((qv[1] >> 14) & 0x00020002u) | ((qv[2] >> 13) & 0x00040004u);   // (k30 | k31 << 16): bits 15 / 31 of the three words
            pr[15] = bits_of(as_f16x2(e | magic) + c1);
#pragma unroll
            for (int i = 0; i < 8; ++i) mm(i >> 1, i & 1, pr[2 * i], pr[2 * i + 1]);
        }
        // the scale is pinned in front of the select on live (an empty asm: the value is read by every lane here).  Left to the compiler, the LDS read of a
        // dead slot's scale is sunk under a branch on live -- s_and_saveexec, ds_read_u16, s_waitcnt lgkmcnt(0), one v_fma_mix -- behind the last matrix-core
        // step of EVERY chunk: an exposed LDS round trip per chunk, and a block boundary the scheduler cannot move the next chunk's reads across
        unsigned sr_ = sraw;
        asm volatile("" : "+v"(sr_));
        const float sc = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)sr_));
        if constexpr (XS) {
            const float* const xv = xe + ((cc - cb) * 4 + kb) * 4;           // the run's sums of x, one per row
            const float zc = (float)(128u + z);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = (STEADY || live) ? fmaf(sc, fmaf(-zc, xv[m], accg[m]), acc[m]) : acc[m];
        } else if constexpr (XC) {
            const float* const xi = xe + ((cc - cb) * 4 + kb) * 4;           // the run's inverse block factors, one per row
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = (STEADY || live) ? fmaf(sc * xi[m], accg[m], acc[m]) : acc[m];
        } else {
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = (STEADY || live) ? fmaf(sc, m < 4 ? accg[m] : accg2[m - 4], acc[m]) : acc[m];   // a select, not a product by 0: a dead slot's x is whatever the LDS holds
        }
    };
    // The K loop: a ROLLING refill.  The wave's first U chunks are requested in front of the staging barrier as before; from then on the load of
    // chunk c0 + j + Wh U goes into q[j] as soon as q[j] has been decoded -- the same registers, no copy -- so U - 1 loads are in flight under every decode
    // (the wait in front of chunk j is vmcnt(U - 1)) and the stream drains only in the wave's LAST pass, which is peeled: it requests nothing.  A wave leaves
    // the loop on its own chunk count (wave-uniform; nothing behind the staging barrier synchronises the waves before the reduction).  Every address is
    // min(c, ce - 1) of the wave's own strip: [cb, ce) as before.  The sched_barriers keep each refill where it is written: free to move, the loads gather at
    // the top of the block, the registers are renamed (copies of registers whose load is in flight: a vmcnt(0) at loop entry) and the counted waits collapse.
    // Same chunks, same sequence, same acc[]: bit-identical to the pass-at-a-time loop (lab: -DGPTQ_TILED_NO_ROLL, tools/ab_tiled.sh).
#ifdef GPTQ_TILED_NO_ROLL
    for (int cbase = cb; cbase < ce; cbase += Wh * U) {
        const int c0 = cbase + wv * U;
        qvec q[U];
#pragma unroll
        for (int j = 0; j < U; ++j) q[j] = wload(c0 + j);
        if (!staged) first_pass();
#ifdef GPTQ_TILED_STAMPS
        if (cbase + Wh * U >= ce) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TILED_STAMP(3); }      // the last pass's chunks have landed
#endif
#pragma unroll
        for (int j = 0; j < U; ++j) chunk(std::false_type{}, c0 + j, j, q[j]);
    }
#else
    if (cb < ce) {                                                                // (an empty slice takes no staging barrier; the planner makes none)
        int c0 = cb + wv * U;
        qvec q[U];
#pragma unroll
        for (int j = 0; j < U; ++j) q[j] = wload(c0 + j);
        first_pass();
        if constexpr (AL) { xpass = (unsigned)(size_t)xll + (unsigned)(c0 - cb) * (unsigned)(CKE * 2); asm volatile("" : "+v"(xpass)); }
        int cn = c0 + Wh * U;
        auto steady = [&](const int stop) __attribute__((always_inline)) {
            for (; cn < stop; cn += Wh * U) {                                     // this wave has a live chunk in the next pass
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    chunk(std::true_type{}, c0 + j, j, q[j]);
                    __builtin_amdgcn_sched_barrier(0);
                    q[j] = wload(cn + j);
                    __builtin_amdgcn_sched_barrier(0);
                }
                c0 = cn;
                if constexpr (AL) { xpass += (unsigned)(Wh * U) * (unsigned)(CKE * 2); asm volatile("" : "+v"(xpass)); }
            }
        };
        if constexpr (TWO) {
            // Two steps: the steady loop stops ONCE behind the wave's first pass -- or in front of it, where the wave has no chunk in a second one --
            // for the barrier that makes step 2 visible: straight-line code between two runs of the SAME loop, reached exactly once by every wave whatever its
            // chunk count, never inside the loop block.  The wave's own step-2 DMAs are older than every refill: the wait in front of its last first-pass chunk
            // (at most U - 1 refills, and the bias, are younger) has retired them; vmcnt(U) says so again and changes nothing.  A wave that will not enter the loop
            // has its U first chunks and its DMAs outstanding, the DMAs youngest: vmcnt(0), where the run is set up -- it decodes those chunks next.  A raw s_barrier, not
            // __syncthreads(): the refills stay in flight across it.
            int stop = ce, pend = 0;
            if (__builtin_expect(xstep1 != 0u, 0)) {
                pend = 1; stop = min(cn + 1, ce);
                if (cn >= ce) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        second_run:
            asm volatile("" : "+s"(stop), "+s"(pend));                            // (opaque: one copy of the loop, not one per run)
            steady(stop);
            if (__builtin_expect(pend != 0, 0)) {
                asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(U) : "memory");
                pend = 0; stop = ce;
                goto second_run;
            }
        } else {
            steady(ce);
        }
#ifdef GPTQ_TILED_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TILED_STAMP(3);          // the last pass's chunks have landed
#endif
#pragma unroll
        for (int j = 0; j < U; ++j) chunk(std::false_type{}, c0 + j, j, q[j]);
    }
#endif
    TILED_STAMP(4);
    // ---- k-slots (two register swaps: a lane owns one column), waves (LDS), then write / publish ---------------------------------------------
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = kslot_sum_swap(acc[m]);
    if (__builtin_expect(!staged, 0)) {                                           // (an empty slice never took the staging barrier; the planner makes none)
        seg_request();
        seg_pin();
        __syncthreads();
    }
    gT* const outg = (gT*)outp;
    if (lane < 16) {
#pragma unroll
        for (int m = 0; m < MT; ++m) red[wave * ES + m * 16 + lane] = acc[m];
    }
    __syncthreads();
    TILED_STAMP(5);
    // Behind this barrier an unsplit launch is straight-line code: the threads that own an output read its W partials in one LDS round trip (wave count known
    // at compile time in each arm: tree_sum / seq_sum, the association of the loops they replace), add the bias that has been in a register since the first
    // pass, and store through pointers held in SGPRs since entry -- no kernel-argument load, no shuffle, no second barrier.  Other wave counts (a forced
    // geometry, a very short K) keep the run-time loops.
    if constexpr (PAIR) {
        // entry e = (row m, column c): gate = the sum over the first half of the waves, up = over the second half (fixed order), the activation on the fp32 sum --
        // the arithmetic of the fused GEMV epilogue of rounds 1-3 (gemv.hip) and, up to the one rounding it saves, of silu_mul_kernel (utils.hip)
        const int NH = N >> 1;
        if (tid < E) {
            const int m = tid >> 4;
            const float* const r = red + tid;
            float s0 = 0.f, s1 = 0.f;
            if (Wh == 4) { s0 = seq_sum<4, ES>(r); s1 = seq_sum<4, ES>(r + 4 * ES); }
            else if (MAXW == 16 && Wh == 8) { s0 = seq_sum<8, ES>(r); s1 = seq_sum<8, ES>(r + 8 * ES); }
            else if (Wh == 2) { s0 = seq_sum<2, ES>(r); s1 = seq_sum<2, ES>(r + 2 * ES); }
            else for (int w = 0; w < Wh; ++w) { s0 += r[w * ES]; s1 += r[(Wh + w) * ES]; }
            if (m < Mrows && n_t < NH) {
                if (biasp != nullptr) { s0 += bv0; s1 += bv1; }
                if (__builtin_expect(is_plain_act(act), 0)) {
                    // split mode (an ungated layer, RELU / GELU / GELU_TANH): the two strips are columns n and n + N/2 of ONE [M, N] output -- the same sums,
                    // the same bias registers, two stores with the row stride N in place of the product
                    outg[(size_t)m * N + n_t] = DType<T>::from_f32(plain_act(s0, act));
                    outg[(size_t)m * N + n_t + NH] = DType<T>::from_f32(plain_act(s1, act));
                } else {
                    const float g = gated_act(s0, act);
                    outg[(size_t)m * NH + n_t] = DType<T>::from_f32(g * s1);
                }
            }
        }
        TILED_STAMP(6);
        TILED_STAMPS_OUT();
        return;
    }
    if constexpr (MULTI) {
        // per strip: the sum over its group of waves (fixed order), bias, one rounding
        const bool lean = (NE <= W * 64) & ((((MAXW == 16 ? 0x114u : 0x14u) >> (Wh & 31)) & 1u) != 0u);      // 2, 4 or 8 waves per strip, a thread per output
        if (__builtin_expect(lean, 1)) {
            if (tid < NE) {
                const int s4 = tid / E, r = tid & (E - 1), m = r >> 4;
                float t;
                constexpr int WHOT = (XM == 6 && MT <= 2) ? 2 : 4;                // the planner's: 4 waves x 2 strips at 1 - 2 rows (K <= 7168), else 4 waves per strip
                if (__builtin_expect(Wh == WHOT, 1)) t = seq_sum<WHOT, ES>(red + s4 * WHOT * ES + r);
                else if (Wh == 6 - WHOT) t = seq_sum<6 - WHOT, ES>(red + s4 * (6 - WHOT) * ES + r);
                else if constexpr (MAXW == 16) t = seq_sum<8, ES>(red + s4 * 8 * ES + r);
                else t = 0.f;                                                     // (not reached)
                if (m < Mrows && n_t < N) {
                    if (biasp != nullptr) t += bv0;
                    outg[(size_t)m * N + n_t] = DType<T>::from_f32(t);
                }
            }
            TILED_STAMP(6);
            TILED_STAMPS_OUT();
            TILED_HOT_END();
        }
        for (int e = tid; e < NSTR * MT * 16; e += W * 64) {
            const int s4 = e / (MT * 16), r = e - s4 * (MT * 16), m = r >> 4, c = r & 15, n = (strip * NSTR + s4) * 16 + c;
            float t = 0.f;
            for (int w = 0; w < Wh; ++w) t += red[(s4 * Wh + w) * ES + r];
            if (m < Mrows && n < N) {
                if (biasp) t += DType<T>::to_f32(((const T*)biasp)[n]);
                ((T*)outp)[(size_t)m * N + n] = DType<T>::from_f32(t);
            }
        }
        return;
    }
    if constexpr (!PEER) {
        // launches without K slices (every launch of the Llama decode step): the hot tail ends here; K slices (granules, epochs, bounded polling) and the other
        // wave counts are the cold block behind it -- one uniform branch on words loaded at entry
        const bool lean = (ksplit == 1) & ((((MAXW == 16 ? 0x10110u : 0x110u) >> (W & 31)) & 1u) != 0u);      // 4, 8 or 16 waves: one scalar test
        if (__builtin_expect(lean, 1)) {
            if (tid < E) {
                const int m = tid >> 4;
                const float* const r = red + tid;
                float t;
                constexpr int WHOT = MAXW == 16 ? 16 : 4;                         // the planner's usual geometry of this compilation first: 16 waves x 2 chunks (up to 256
                if (__builtin_expect(W == WHOT, 1)) t = tree_sum<WHOT, ES>(r);    // workgroups), 4 waves x 4 chunks (more than 512)
                else if (MAXW == 8 || W == 8) t = tree_sum<8, ES>(r);
                else t = tree_sum<4, ES>(r);
                if (m < Mrows && n_t < N) {
                    if (biasp != nullptr) t += bv0;
                    outg[(size_t)m * N + n_t] = DType<T>::from_f32(t);
                }
            }
            TILED_STAMP(6);
            TILED_STAMPS_OUT();
            TILED_HOT_END();                                            // the hot s_endpgm: not a jump over the cold block to a shared return
        }
    }
    T* const stage = PEER ? (T*)xs : nullptr;                                      // the staged x is dead behind the barrier above
    const TiledSeg sg{biasp, outp, N, ksplit != 1 ? p.seg[s].col0 : 0};              // (col0: K slices only -- a kernel-argument load in the cold block)
    stream_finish<16, MT, T, TiledParams, TiledSeg>(p, sg, strip, sidx, ks, N, red, stage);
    if constexpr (PEER) if (ks == 0) {                                            // uniform: the strip's owner
        const int pworld = p.peer.world;
        __syncthreads();
        const unsigned e = __hip_atomic_load(p.peer.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;      // this gather's epoch (peer.hip)
        if (tid < pworld * MT * 2) {                                              // (peer, row, half of the strip's 32 bytes)
            const int r = tid / (MT * 2), m = (tid >> 1) % MT, q = tid & 1;
            if (m < Mrows) {
                const u32x4 v = *(const u32x4*)((const char*)stage + m * 32 + q * 16);
                char* const dst = p.peer.xbuf[e & 1u][r] + (size_t)m * p.peer.row_bytes + p.peer.col_off_bytes + (size_t)strip * 32 + q * 16;
                // a system-scope WRITE-THROUGH store (sc0 sc1): the payload goes to its home, not into this XCD's L2.  NOT a release fence per
                // workgroup: at system (and agent) scope that is an L2 write-back, and hundreds of strips doing one each cost 20 - 240 us per launch
                // (profiles/r04_tp2_same_device_fused_scatter_v1 / v2*.json).
                asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
            }
        }
        // No ticket, no flag here: the rank's arrival flag is raised by its COLLECT launch, which starts behind this kernel in stream order (every store
        // above has been acknowledged by then).  A ticket drawn by every strip -- 256 .. 896 fetch-adds on one word -- measured 8 - 70 us per launch.
    }
}

// ONE compilation per (BITS, MT, U, T, XM) (round 6: there were two -- workgroups of up to 16 and of up to 8 waves -- that differed by a register or two, every
// form fits 128 VGPRs): the launch bound is the one the planner's geometry of that depth uses -- 2 chunks in flight: 16-wave workgroups (<= 320 workgroups:
// one per CU); 4 chunks in flight: 4- or 8-wave workgroups, except the four-strip form (XM = 5: 16 waves = 4 strips x 4 waves).  A forced (waves, depth)
// outside its compilation is refused by plan_tiled.
template <int U, int XM> constexpr int tiled_maxw() { return (U == 2 || XM == 5) ? 16 : 8; }
int tiled_max_waves(int u, int nstr);                                             // the same rule for the planner (gemv_tiled.hip)
// The forms that have an aligned twin (FL = 2): 4-bit layers at one row, plain and two-strip, and the two-strip form at two rows -- what the
// library's kernel budget (tests/test_kernel_resources.py) leaves room for; tiled_has_aligned() is the same rule for the planner.
template <int BITS, int MT, int U, int XM> constexpr bool tiled_aligned_form() { return BITS == 4 && ((XM == 0 && MT == 1) || (XM == 6 && MT <= 2 && U == 4)); }
bool tiled_has_aligned(int bits, int mt, int u, int nstr);
template <int BITS, int MT, int U, typename T, int XM>
static hipError_t launch_tiled_one(const TiledPlan& pl, const TiledParams& p, hipStream_t st) {
    constexpr int MAXW = tiled_maxw<U, XM>();
    if (pl.waves > MAXW) return hipErrorInvalidValue;
    if constexpr (tiled_aligned_form<BITS, MT, U, XM>()) {
        if (pl.aligned) {
            hipLaunchKernelGGL((gemv_tiled_kernel<BITS, MT, U, T, MAXW, XM, 2>), dim3(pl.strips_total * pl.ksplit), dim3(pl.waves * 64), pl.lds_bytes, st, p);
            return hipGetLastError();
        }
    } else if (pl.aligned) {
        return hipErrorInvalidValue;
    }
    if constexpr (BITS == 4 && MT == 2 && std::is_same_v<T, bf16> && (XM == 0 || XM == 1)) {      // plain and act-order forms
        if (pl.zm2) {
            hipLaunchKernelGGL((gemv_tiled_kernel<BITS, MT, U, T, MAXW, XM, 1>), dim3(pl.strips_total * pl.ksplit), dim3(pl.waves * 64), pl.lds_bytes, st, p);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((gemv_tiled_kernel<BITS, MT, U, T, MAXW, XM>), dim3(pl.strips_total * pl.ksplit), dim3(pl.waves * 64), pl.lds_bytes, st, p);
    return hipGetLastError();
}
template <int BITS, int MT, typename T, int XM>
static hipError_t launch_tiled_u(const TiledPlan& pl, const TiledParams& p, hipStream_t st) {
    switch (pl.u) {
        // (the four-strip form with 2 chunks in flight: 4-bit layers only -- no plan but a doubly forced one asks for it, and the 3- / 8-bit ones paid for the aligned twins)
        case 2: if constexpr (!(XM == 6 && MT <= 2) && !(XM == 5 && BITS != 4)) return launch_tiled_one<BITS, MT, 2, T, XM>(pl, p, st); else return hipErrorInvalidValue;
        case 4: return launch_tiled_one<BITS, MT, 4, T, XM>(pl, p, st);
        default: return hipErrorInvalidValue;
    }
}
template <int BITS, typename T, int XM>
static hipError_t launch_tiled_mt(const TiledPlan& pl, const TiledParams& p, hipStream_t st) {
    // multi-strip workgroups: the 3..4-row and 5..8-row forms; round 6: two strips per workgroup also at 1 - 2 rows of 4-bit layers (the planner's own geometry only:
    // 8 waves x 4 chunks) -- the 1376-strip gate|up launch 11.8 -> 11.5 us (profiles/r06_multi_low_ab.log)
    constexpr bool LOW_OK = XM != 5 && (XM != 6 || BITS == 4);
    if constexpr (!LOW_OK) {
        if (pl.mt != 4 && pl.mt != 8) return hipErrorInvalidValue;
    }
    switch (pl.mt) {
        case 1: if constexpr (LOW_OK) return launch_tiled_u<BITS, 1, T, XM>(pl, p, st); else return hipErrorInvalidValue;
        case 2: if constexpr (LOW_OK) return launch_tiled_u<BITS, 2, T, XM>(pl, p, st); else return hipErrorInvalidValue;
        case 4: return launch_tiled_u<BITS, 4, T, XM>(pl, p, st);
        case 8: if constexpr (XM != 3 && XM != 4 && BITS != 2) return launch_tiled_u<BITS, 8, T, XM>(pl, p, st); else return hipErrorInvalidValue;      // 5..8 rows: plain, act-order and multi-strip forms
        default: return hipErrorInvalidValue;
    }
}
template <typename T, int XM>
static hipError_t launch_tiled_bits(const TiledPlan& pl, const TiledParams& p, hipStream_t st) {
    switch (pl.bits) {
        case 4: return launch_tiled_mt<4, T, XM>(pl, p, st);
        case 8: return launch_tiled_mt<8, T, XM>(pl, p, st);
        case 3: return launch_tiled_mt<3, T, XM>(pl, p, st);
        case 2:                                                                   // 2 bits (round 6): plain and act-order forms, up to 4 rows
            if constexpr (XM == 0 || XM == 1) { if (pl.mt <= 4) return launch_tiled_mt<2, T, XM>(pl, p, st); }
            return hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
}

// grants > 64 KiB of dynamic LDS to every instantiation of one x mode (long K at 4 rows of x: the staged activations can pass the default)
template <int XM>
static hipError_t grant_tiled_lds() {
    hipError_t e = hipSuccess;
    auto grant = [&](auto kern) { hipError_t r = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); if (e == hipSuccess) e = r; };
    auto grant_mt = [&](auto mt) {
        constexpr int MT = decltype(mt)::value;
        auto grant_u = [&](auto bu, auto uu) {
            constexpr int B = decltype(bu)::value, U = decltype(uu)::value;
            constexpr int MAXW = tiled_maxw<U, XM>();
            if constexpr (!(XM == 5 && B != 4 && U == 2)) { grant(gemv_tiled_kernel<B, MT, U, f16, MAXW, XM>); grant(gemv_tiled_kernel<B, MT, U, bf16, MAXW, XM>); }      // (else: not compiled -- launch_tiled_u)
            if constexpr (tiled_aligned_form<B, MT, U, XM>()) { grant(gemv_tiled_kernel<B, MT, U, f16, MAXW, XM, 2>); grant(gemv_tiled_kernel<B, MT, U, bf16, MAXW, XM, 2>); }
            if constexpr (B == 4 && MT == 2 && (XM == 0 || XM == 1)) grant(gemv_tiled_kernel<B, MT, U, bf16, MAXW, XM, 1>);
        };
        using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>; using I4 = std::integral_constant<int, 4>; using I8 = std::integral_constant<int, 8>;
        grant_u(I4{}, I2{}); grant_u(I4{}, I4{});
        grant_u(I8{}, I2{}); grant_u(I8{}, I4{}); grant_u(I3{}, I2{}); grant_u(I3{}, I4{});
        if constexpr ((XM == 0 || XM == 1) && MT <= 4) { grant_u(I2{}, I2{}); grant_u(I2{}, I4{}); }
    };
    if constexpr (XM != 5 && XM != 6) { grant_mt(std::integral_constant<int, 1>{}); grant_mt(std::integral_constant<int, 2>{}); }
    if constexpr (XM == 6) {                                                      // the 1 - 2-row two-strip form (4 bits, 8 waves x 4 chunks)
        grant(gemv_tiled_kernel<4, 1, 4, f16, 8, 6>); grant(gemv_tiled_kernel<4, 1, 4, bf16, 8, 6>);
        grant(gemv_tiled_kernel<4, 2, 4, f16, 8, 6>); grant(gemv_tiled_kernel<4, 2, 4, bf16, 8, 6>);
        grant(gemv_tiled_kernel<4, 1, 4, f16, 8, 6, 2>); grant(gemv_tiled_kernel<4, 1, 4, bf16, 8, 6, 2>);      // their aligned twins
        grant(gemv_tiled_kernel<4, 2, 4, f16, 8, 6, 2>); grant(gemv_tiled_kernel<4, 2, 4, bf16, 8, 6, 2>);
    }
    grant_mt(std::integral_constant<int, 4>{});
    if constexpr (XM != 3 && XM != 4) grant_mt(std::integral_constant<int, 8>{});
    return e;
}

}  // namespace gptq
