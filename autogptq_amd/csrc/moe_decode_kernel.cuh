// moe_decode_kernel.cuh -- the body of the two decode launches of a routed mixture-of-experts layer, moe_decode_body<T, BITS, PAIR, SHARED>:
//   SHARED = false  moe_decode.hip's moe_decode_kernel<T, BITS, PAIR>, the routed experts alone (every `sh` below is a constant false: the code of the
//                   kernels as they were before the shared form existed); at BITS 3 and 2 (GPTQ_MOE_LOW_BIT_DECODE) the same compilation runs as
//                   forms 10..17 of moe_shared.hip's kernel -- the library's kernel count is guarded, so those widths are forms, not kernels
//   SHARED = true   moe_shared.hip: the always-on shared expert of a Qwen-MoE block served by the same two launches
//
// A SEGMENT is one streamed strip (pair: one strip of W1 next to the same strip of W3) against one staged activation row.  The routed kernels run one
// segment per assignment; the shared form adds
//   pair  workgroups past the routed rows of the grid (blockIdx.y >= T topk): per token ceil(I_s / I) rows of I / 16 workgroups, strip =
//         (row within the token) (I / 16) + blockIdx.x, workgroups with strip >= I_s / 16 leave before any barrier.  Their pointers come from the launch
//         arguments, their K is H as well; groups / gshift / LDS offsets are those of the shared layers.  Strip 0 also writes the gate scalar s_t.
//   down  one more segment behind the token's topk routed ones: hs[t] against strip s of the shared W2, weighted by s_t, into the same register.
// The two kinds of segment may want different wave counts (K = I against K = I_s): the workgroup has the larger count, a segment distributes its chunks
// over ITS OWN count W (so the routed segments sum in the order of the routed launch, bit for bit), and a wave >= W sees clamped chunks only and adds
// nothing (W < block waves implies W U >= chunks: one pass, every chunk of such a wave is past the end).  The cross-wave slab sits behind BOTH layouts.
#pragma once
#include "gemv_tiled_kernel.cuh"     // TiledFmt<BITS>, WordsOf, and through gemv_shared.cuh: Mma4, kslot_sum_swap; common.cuh: lds_dma16_nt

namespace gptq {
namespace moedec {

constexpr int U = 4;                            // chunks per wave in flight
constexpr int ES = 16 + 4;                      // floats per wave in the cross-wave slab (padded by 16 B)
constexpr int MAX_WAVES_PAIR = 8, MAX_WAVES_DOWN = 16;       // sized down from the chunk count of a strip: waves_for()
constexpr int MAX_LDS = 160 * 1024;

struct Entry {                                  // one (projection, expert) of the device table: [3 projections][E], 32 bytes
    const unsigned* tq;                         // qweight_tiled
    const void* cst;                            // qconst_tiled
    const int* perm;                            // NULL: sequential groups
    const void* reserved;
};

struct Args {
    const Entry* table;                         // pair: W1 entries (W3: + E); down: W2 entries
    const long long* idx;                       // [T][topk]
    const float* w;                             // [T][topk] (down)
    const void* a;                              // pair: x [T][K]; down: h [T topk][K]
    void* out;                                  // pair: h [T topk][N]; down: out [T][N]
    int* pos;                                   // pair: [T topk]
    int E, topk, K, N, chunks, groups, gshift, waves;
    int off_xs0, off_xs1, off_cs, cpad;         // LDS layout (bytes): raw row at 0, gathered rows, constants (pair: two records runs cpad apart); sums behind them
};

struct Shared {                                 // the shared expert's segment (SHARED form only)
    int form, pad;                              // moe_shared.hip: which compilation of the body the one shared kernel runs
    Entry e0, e1;                               // pair: the shared gate and up layers; down: e0 = the shared W2
    const void* gate_w;                         // pair: [H] layer dtype or NULL (s = 1)
    float* s;                                   // [T]: pair writes (strip 0), down reads
    const void* a;                              // pair: x [T][K]; down: hs [T][K]
    void* out;                                  // pair: hs [T][N]
    int rows, per_tok, strips;                  // pair: T topk (the routed rows of the grid), grid rows per token, I_s / 16
    int K, N, chunks, groups, gshift, waves;    // this segment's own (waves: the count its chunks are distributed over)
    int off_xs0, off_xs1, off_cs, cpad;
    int block_waves, off_red;                   // waves of the workgroup; the cross-wave slab, behind the routed and the shared layout
};

// The table entry of an expert: every lane loads the same 32 bytes; readfirstlane makes the pointers scalars for the compiler (uniform branches, SGPR bases).
typedef unsigned u32x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ Entry load_entry(const Entry* p) {
    const u32x8 v = *(const u32x8*)p;
    u32x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = __builtin_amdgcn_readfirstlane(v[i]);
    return __builtin_bit_cast(Entry, o);
}

// The gate scalar of a shared expert, s = sigmoid(T(x . w_g)), by ONE wave (every lane returns it): lane l takes the 16-byte pieces l, l + 64, .. of the
// row in ascending order (fmaf, ascending element), then a butterfly -- the order of the router kernel's rows form, a function of H alone.  One rounding
// to the layer dtype, the sigmoid in fp32.  xrow: LDS or global, 16-byte aligned; H % 8 == 0.
template <typename T, typename XP>
__device__ __forceinline__ float shared_gate_scalar(XP xrow, const void* w, int H, int lane) {
    typedef __attribute__((address_space(1))) const u32x4 gu32x4;
    gu32x4* const wrow = (gu32x4*)w;
    float a = 0.f;
    for (int pc = lane; pc < (H >> 3); pc += 64) {
        const u32x4 xv = xrow[pc], wv = wrow[pc];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float xf = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(xv[c >> 1] >> (16 * (c & 1)))));
            const float wf = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(wv[c >> 1] >> (16 * (c & 1)))));
            a = fmaf(xf, wf, a);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
    const float l = DType<T>::to_f32(DType<T>::from_f32(a));
    return 1.f / (1.f + __expf(-l));
}

template <typename T, int BITS, bool PAIR, bool SHARED>
__device__ __forceinline__ void moe_decode_body(const Args& p, const Shared& sp) {
    constexpr bool BF = std::is_same_v<T, bf16>;
    using F = TiledFmt<BITS>;
    constexpr int WPL = F::WPL, KPL = F::KPL, CKE = 4 * KPL, CHB = 64 * WPL * 4, REC = F::REC, NX = KPL / 8;
    constexpr int LKPL = KPL == 32 ? 5 : 4;
    typedef typename WordsOf<WPL>::type qvec;
    unsigned m_lo, m_hi, m_b, magic;                                              // opaque constants: (q & mask) | magic is ONE v_and_or_b32
    asm("s_mov_b32 %0, 0x000f000f" : "=s"(m_lo));
    asm("s_mov_b32 %0, 0x00f000f0" : "=s"(m_hi));
    asm("s_mov_b32 %0, 0x00ff00ff" : "=s"(m_b));
    asm("v_mov_b32 %0, 0x64006400" : "=v"(magic));
    [[maybe_unused]] unsigned m2a, m2b, m2c, m2d, m2e, m3a, m3b, m3c;            // the 2- and 3-bit forms' field masks (unused ones leave no instruction)
    if constexpr (BITS == 2) {
        asm("s_mov_b32 %0, 0x00030003" : "=s"(m2a));
        asm("s_mov_b32 %0, 0x000c000c" : "=s"(m2b));
        asm("s_mov_b32 %0, 0x00300030" : "=s"(m2c));
        asm("s_mov_b32 %0, 0x00c000c0" : "=s"(m2d));
        asm("s_mov_b32 %0, 0x03000300" : "=s"(m2e));
    }
    if constexpr (BITS == 3) {
        asm("s_mov_b32 %0, 0x00070007" : "=s"(m3a));
        asm("s_mov_b32 %0, 0x00380038" : "=s"(m3b));
        asm("s_mov_b32 %0, 0x01c001c0" : "=s"(m3c));
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, kb = lane >> 4;
    const int E = p.E, topk = p.topk;
    const int WB = SHARED ? sp.block_waves : p.waves;                                 // waves of the workgroup: staging and gathers are spread over all of them
    // pair, shared form: the workgroups past the routed rows serve (token, strip of I_s)
    const bool shared_wg = SHARED && PAIR && (int)blockIdx.y >= sp.rows;          // uniform
    int strip = blockIdx.x, stok = 0;
    if constexpr (SHARED && PAIR) {
        if (shared_wg) {
            const int y = (int)blockIdx.y - sp.rows;
            stok = y / sp.per_tok;
            strip = (y - stok * sp.per_tok) * (int)gridDim.x + (int)blockIdx.x;
            if (strip >= sp.strips) return;                                       // before any barrier
        }
    }
    char* const xraw = smem;
    const unsigned t_lane = (unsigned)lane * (WPL * 4u);
    const f16x2 k960 = {(f16)960.f, (f16)960.f};
    const f16x2 r16 = {(f16)0.0625f, (f16)0.0625f};
    [[maybe_unused]] const f16x2 k768 = {(f16)768.f, (f16)768.f}, k896 = {(f16)896.f, (f16)896.f}, k1008 = {(f16)1008.f, (f16)1008.f}, k1020 = {(f16)1020.f, (f16)1020.f};
    [[maybe_unused]] const f16x2 r4 = {(f16)0.25f, (f16)0.25f}, r8 = {(f16)0.125f, (f16)0.125f}, r64 = {(f16)0.015625f, (f16)0.015625f}, r256 = {(f16)0.00390625f, (f16)0.00390625f};
    auto bits_of = [&](f16x2 hv) -> unsigned {                                    // the pair as the matrix core takes it (bf16: fp16 -> fp32 -> bf16, exact: small integers)
        if constexpr (BF) {
            const bf16x2 o = {(bf16)(float)hv[0], (bf16)(float)hv[1]};
            return __builtin_bit_cast(unsigned, o);
        } else {
            return __builtin_bit_cast(unsigned, hv);
        }
    };

    const int first = PAIR ? (int)blockIdx.y : (int)blockIdx.y * topk;            // pair: the assignment; down: the token's first assignment
    const int count = PAIR ? 1 : topk + (SHARED ? 1 : 0);                         // down, shared form: the shared expert's segment behind the routed ones
    float total = 0.f;                                                            // down: thread c < 16 -- sum_j w[t, j] * (h_r . W2_e)[16 s + c] (+ s_t * (hs_t . W2_s)[16 s + c])
    for (int jj = 0; jj < count; ++jj) {
        const bool sh = SHARED && (PAIR ? shared_wg : jj == topk);                // uniform: this segment is the shared expert's
        // the segment's own geometry (without SHARED: the launch's, loop-invariant)
        const int W = sh ? sp.waves : p.waves, K = sh ? sp.K : p.K, N = sh ? sp.N : p.N, G = sh ? sp.groups : p.groups;
        const int nchunks = sh ? sp.chunks : p.chunks, gshift = sh ? sp.gshift : p.gshift;
        const int off_xs0 = sh ? sp.off_xs0 : p.off_xs0, off_xs1 = sh ? sp.off_xs1 : p.off_xs1, off_cs = sh ? sp.off_cs : p.off_cs, cpad = sh ? sp.cpad : p.cpad;
        const int Wh = PAIR ? (W >> 1) : W;                                       // waves per streamed strip
        const int sel = PAIR ? (wave >= Wh ? 1 : 0) : 0;                          // pair: 0 = gate (W1), 1 = up (W3)
        const int wv = wave - sel * Wh;
        char* const xs0 = smem + off_xs0;
        char* const xs1 = smem + off_xs1;
        char* const cs = smem + off_cs + sel * cpad;
        float* const red = (float*)(smem + (SHARED ? sp.off_red : off_cs + (PAIR ? 2 : 1) * cpad));
        const int r = sh ? 0 : first + jj;
        int e = 0;
        float wr = 0.f;
        if (!sh) {
            const long long ev = p.idx[r];
            wr = p.w[r];
            e = __builtin_amdgcn_readfirstlane((ev >= 0 && ev < (long long)E) ? (int)ev : -1);
            if constexpr (PAIR) {
                if (strip == 0 && tid == 0) p.pos[r] = e >= 0 ? r : -1;
            }
        }
        if constexpr (SHARED && !PAIR) {
            if (sh) wr = sp.s[blockIdx.y];
        }
        if (e < 0) continue;                                                      // uniform: a dropped assignment
        const Entry e0 = sh ? sp.e0 : load_entry(p.table + e);
        const unsigned* tq0 = e0.tq;
        const char* cst0 = (const char*)e0.cst;
        const int* perm0 = e0.perm;
        const unsigned* tq1 = tq0;
        const char* cst1 = cst0;
        const int* perm1 = perm0;
        if constexpr (PAIR) {
            const Entry e1 = sh ? sp.e1 : load_entry(p.table + E + e);
            tq1 = e1.tq;
            cst1 = (const char*)e1.cst;
            perm1 = e1.perm;
        }
        const bool same = perm0 == perm1;                                         // (down: always)
        const int* const pm = sel ? perm1 : perm0;                                // this wave's projection
        typedef __attribute__((address_space(1))) const char gchar;               // (rebuilt from readfirstlane words the pointers are generic for the compiler: say that they are global,
        typedef __attribute__((address_space(1))) const int gint;                 //  or the weight stream becomes flat loads that also count as LDS traffic)
        typedef __attribute__((address_space(1))) const qvec gqvec;
        gchar* const tb = (gchar*)(sel ? tq1 : tq0) + (size_t)strip * nchunks * CHB;      // this wave's strip of weights: one contiguous run
        gint* const pmg = (gint*)pm;
        const char* const arow = sh ? (const char*)sp.a + (size_t)(PAIR ? stok : (int)blockIdx.y) * K * 2
                                    : (const char*)p.a + (size_t)(PAIR ? r / topk : r) * K * 2;
        // ---- stage the raw activation row and the constants by LDS DMA, issued FIRST (loads return in issue order), waited for behind the first weight burst
        {
            const unsigned x_lds = lds_addr_of(xraw), c_lds = lds_addr_of(smem + off_cs);
            const int pieces = K >> 3;                                            // 16-byte pieces of the row
            for (int pc0 = wave * 64; pc0 < pieces; pc0 += WB * 64)               // wave-uniform trip count
                if (pc0 + lane < pieces) lds_dma16(arow + (size_t)(pc0 + lane) * 16, x_lds + pc0 * 16);
            const int cpieces = (G * REC) >> 4;                                   // REC is a multiple of 16
            const char* const cg0 = cst0 + (size_t)strip * G * REC;
            for (int pc0 = wave * 64; pc0 < cpieces; pc0 += WB * 64)
                if (pc0 + lane < cpieces) lds_dma16_nt(cg0 + (size_t)(pc0 + lane) * 16, __builtin_amdgcn_readfirstlane(c_lds + pc0 * 16));
            if constexpr (PAIR) {
                const char* const cg1 = cst1 + (size_t)strip * G * REC;
                for (int pc0 = wave * 64; pc0 < cpieces; pc0 += WB * 64)
                    if (pc0 + lane < cpieces) lds_dma16_nt(cg1 + (size_t)(pc0 + lane) * 16, __builtin_amdgcn_readfirstlane(c_lds + (unsigned)cpad + pc0 * 16));
            }
        }
        const char* const xw = pm ? ((same || !sel) ? xs0 : xs1) : xraw;          // the row this wave multiplies: gathered through its perm, or raw
        const char* const xl = xw + kb * (KPL * 2);
        float acc = 0.f;
        bool staged = false;
        for (int cbase = 0; cbase < nchunks; cbase += Wh * U) {
            const int c0 = cbase + wv * U;
            qvec q[U];
#pragma unroll
            // INVARIANT of the staging wait below: exactly U separate vector loads (run-time clamped addresses: not merged, not hoisted) and nothing else that
            // counts on vmcnt between the asm-hidden DMAs above and the s_waitcnt vmcnt(U) -- then "at most U outstanding" means every DMA has landed
            for (int j = 0; j < U; ++j) q[j] = __builtin_nontemporal_load((gqvec*)(tb + ((unsigned)min(c0 + j, nchunks - 1) * (unsigned)CHB + t_lane)));
            if (!staged) {                                                        // first pass only (uniform): the staging DMAs are OLDER than the U loads just issued
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(U) : "memory");
                __syncthreads();                                                  // the raw row and the constants (every wave's DMAs) are in the LDS
                if (perm0 != nullptr || perm1 != nullptr) {                       // uniform over the workgroup
                    if (pm != nullptr) {
                        // act-order: one thread = one 16-byte piece = 8 consecutive positions of the copy = 32 contiguous bytes of perm; LDS -> LDS.
                        // Equal pointers: ONE gather by all waves; else each half gathers through its own projection's perm into its own buffer.
                        const int gt = same ? tid : tid - sel * Wh * 64, gn = same ? WB * 64 : Wh * 64;
                        char* const dst = (same || !sel) ? xs0 : xs1;
                        const unsigned short* const xr = (const unsigned short*)xraw;
                        typedef int i32x4 __attribute__((ext_vector_type(4)));
                        for (int pc = gt; pc < (K >> 3); pc += gn) {
                            typedef __attribute__((address_space(1))) const i32x4 gi32x4;
                            const i32x4 pa = *(gi32x4*)(pmg + pc * 8), pb = *(gi32x4*)(pmg + pc * 8 + 4);
                            u32x4 o;
                            o[0] = (unsigned)xr[pa[0]] | ((unsigned)xr[pa[1]] << 16);
                            o[1] = (unsigned)xr[pa[2]] | ((unsigned)xr[pa[3]] << 16);
                            o[2] = (unsigned)xr[pb[0]] | ((unsigned)xr[pb[1]] << 16);
                            o[3] = (unsigned)xr[pb[2]] | ((unsigned)xr[pb[3]] << 16);
                            *(u32x4*)(dst + (size_t)pc * 16) = o;
                        }
                    }
                    __syncthreads();
                }
                staged = true;
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const int cc = min(c0 + j, nchunks - 1);
                const int k0 = cc * CKE + kb * KPL;                               // first k of this lane's words
                const bool live = (c0 + j < nchunks) && (k0 < K);                 // a ragged last chunk: whole k-slots are missing
                const int g = min(k0 >> LKPL >> gshift, G - 1);
                const char* cp = cs + g * REC;
                const unsigned short sraw = *(const unsigned short*)(cp + col * 2);
                unsigned z;
                if constexpr (F::ZB == 1) z = *(const unsigned char*)(cp + 32 + col);
                else z = *(const unsigned short*)(cp + 32 + col * 2);
                u32x4 xa[NX];
#pragma unroll
                for (int w = 0; w < NX; ++w) xa[w] = *(const u32x4*)(xl + ((unsigned)cc * (unsigned)(CKE * 2) + w * 16u));      // (a dead k-slot reads whatever the LDS holds behind the row: discarded below)
                const f16x2 c1 = as_f16x2(z * 0x00010001u + 0xE400E400u);        // -(1024 + z)
                const qvec qv = q[j];
                f32x4 accg = {0.f, 0.f, 0.f, 0.f};
                auto mm = [&](int pc, int hf, unsigned b0, unsigned b1) __attribute__((always_inline)) {      // 4 k of the lane's column against x piece pc, half hf
                    accg = Mma4<T>::run(u32x2{xa[pc][hf * 2], xa[pc][hf * 2 + 1]}, u32x2{b0, b1}, accg);
                };
                if constexpr (BITS == 4) {
                    const f16x2 c2 = c1 + k960;                                   // -(64 + z)
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const unsigned qw = qv[w], q8 = qw >> 8;
                        const f16x2 h0 = as_f16x2((qw & m_lo) | magic) + c1;      // k0,k1  (stored nibbles 0 and 4)
                        const f16x2 h1 = as_f16x2((qw & m_hi) | magic) * r16 + c2;      // k2,k3  (1 and 5)
                        const f16x2 h2 = as_f16x2((q8 & m_lo) | magic) + c1;      // k4,k5  (2 and 6)
                        const f16x2 h3 = as_f16x2((q8 & m_hi) | magic) * r16 + c2;      // k6,k7  (3 and 7)
                        mm(w, 0, bits_of(h0), bits_of(h1));
                        mm(w, 1, bits_of(h2), bits_of(h3));
                    }
                } else if constexpr (BITS == 8) {
#pragma unroll
                    for (int w = 0; w < 4; ++w) {                                 // one word = 4 k = one matrix-core step
                        const unsigned qw = qv[w], q8 = qw >> 8;
                        const f16x2 h0 = as_f16x2((qw & m_b) | magic) + c1;       // k0,k1  (stored bytes 0 and 2)
                        const f16x2 h1 = as_f16x2((q8 & m_b) | magic) + c1;       // k2,k3  (1 and 3)
                        mm(w >> 1, w & 1, bits_of(h0), bits_of(h1));
                    }
                } else if constexpr (BITS == 2) {
                    // the dense decode kernel's 2-bit branch (gemv_tiled_kernel.cuh): the five pairs at bits 0..9 in place (1024 + 4^p w, times 4^-p, minus
                    // (1024 / 4^p + z): exact), the three at bits 10..15 behind a shift
                    const f16x2 c4 = c1 + k768, c16 = c1 + k960, c64 = c1 + k1008, c256 = c1 + k1020;      // -(256 + z), -(64 + z), -(16 + z), -(4 + z)
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
                } else {
                    // 3 bits, the dense decode kernel's branch: word j holds the pairs 5 j + i at bit 3 i of its halves, no field straddles a word; the
                    // pairs are consumed as they are produced (two at a time, in k order), pair 15 = bits 15 / 31 of the three words
                    static_assert(BITS == 3, "moe_decode_body: 2, 3, 4 or 8 bits");
                    const f16x2 c3 = c1 + k896;                                   // -(128 + z): fields at bit 3, times 1/8
                    const f16x2 c6 = c1 + k1008;                                  // -(16 + z): fields at bit 6, times 1/64
                    auto field = [&](int pi) __attribute__((always_inline)) -> unsigned {      // pair pi of the unit (compile-time pi)
                        if (pi == 15) {
                            const unsigned e15 = ((qv[0] >> 15) & 0x00010001u) | ((qv[1] >> 14) & 0x00020002u) | ((qv[2] >> 13) & 0x00040004u);
                            return bits_of(as_f16x2(e15 | magic) + c1);
                        }
                        const unsigned t = qv[pi / 5], t6 = t >> 6;
                        switch (pi % 5) {
                            case 0: return bits_of(as_f16x2((t & m3a) | magic) + c1);
                            case 1: return bits_of(as_f16x2((t & m3b) | magic) * r8 + c3);
                            case 2: return bits_of(as_f16x2((t & m3c) | magic) * r64 + c6);
                            case 3: return bits_of(as_f16x2((t6 & m3b) | magic) * r8 + c3);
                            default: return bits_of(as_f16x2((t6 & m3c) | magic) * r64 + c6);
                        }
                    };
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const unsigned b0 = field(2 * i), b1 = field(2 * i + 1);
                        mm(i >> 1, i & 1, b0, b1);
                    }
                }
                const float sc = DType<T>::to_f32(__builtin_bit_cast(T, sraw));
                acc = live ? fmaf(sc, accg[0], acc) : acc;                        // a select, not a product by 0
            }
        }
        // ---- k-slots (two register swaps: a lane owns one column), waves (LDS, wave order)
        acc = kslot_sum_swap(acc);
        if (lane < 16) red[wave * ES + lane] = acc;
        __syncthreads();
        if constexpr (PAIR) {
            if (tid < 16) {
                float s0 = 0.f, s1 = 0.f;
                for (int w = 0; w < Wh; ++w) { s0 += red[w * ES + tid]; s1 += red[(Wh + w) * ES + tid]; }
                const float gv = s0 / (1.f + __expf(-s0));
                T* const orow = sh ? (T*)sp.out + (size_t)stok * N : (T*)p.out + (size_t)r * N;
                orow[strip * 16 + tid] = DType<T>::from_f32(gv * s1);
            }
            if constexpr (SHARED) {
                // the gate scalar of the token, by wave 0 of the shared workgroup of strip 0: x_t is staged here already, and nothing reads s_t before launch 2
                if (sh && strip == 0 && wave == 0) {
                    float sv = 1.f;
                    if (sp.gate_w) sv = shared_gate_scalar<T>((const u32x4*)xraw, sp.gate_w, K, lane);
                    if (lane == 0) sp.s[stok] = sv;
                }
            }
        } else {
            if (tid < 16) {
                float s0 = 0.f;
                for (int w = 0; w < W; ++w) s0 += red[w * ES + tid];
                total += wr * s0;
            }
            // the next assignment's DMAs overwrite the row and the constants: every wave is past its K loop here (the barrier above); the sums are
            // written again only behind the next staging barrier, which thread c reaches after it has read them.  (Shared form: the slab lies behind
            // both layouts, so the DMAs of a segment with the other layout cannot reach it either.)
        }
    }
    if constexpr (!PAIR) {
        if (tid < 16) ((T*)p.out)[(size_t)blockIdx.y * p.N + strip * 16 + tid] = DType<T>::from_f32(total);
    }
}


// waves that stream one strip: one per U chunks of the strip, so that no wave runs the K loop on clamped chunks only (I = 1408 at 4 bits is 11 chunks: 3 waves)
static inline int waves_for(int K, int bits, bool pair) {
    const int cke = bits == 8 ? 64 : 128, chunks = (K + cke - 1) / cke, per = (chunks + U - 1) / U;
    return pair ? 2 * std::min(MAX_WAVES_PAIR / 2, per) : std::min(MAX_WAVES_DOWN, per);
}

struct Lds { int off_xs0, off_xs1, off_cs, cpad, bytes; };
static inline Lds lds_layout(int K, int groups, int bits, bool act, bool pair, int waves) {
    Lds l;
    const int cke = bits == 8 ? 64 : 128;
    const int row = (K + cke - 1) / cke * cke * 2 + 16;          // whole chunks: the dead k-slots of a ragged last chunk read inside the row's own padding
    l.off_xs0 = row;
    l.off_xs1 = act && pair ? 2 * row : row;
    l.off_cs = !act ? row : (pair ? 3 * row : 2 * row);
    l.cpad = (groups * (bits == 8 ? 64 : 48) + 15) & ~15;
    l.bytes = l.off_cs + (pair ? 2 : 1) * l.cpad + waves * ES * 4;
    return l;
}

static inline int kpl_of(int bits) { return bits == 8 ? 16 : 32; }
// the geometry of one layer's segment as the kernel takes it
template <typename A>
static inline void fill_geometry(A& a, const gptq_layer_t& L, bool act, bool pair, int waves) {
    const int cke = 4 * kpl_of(L.bits);
    a.K = L.K; a.N = L.N;
    a.chunks = (L.K + cke - 1) / cke;
    a.groups = (L.K + L.group_size - 1) / L.group_size;
    a.gshift = L.group_size >= L.K ? 26 : __builtin_ctz((unsigned)(L.group_size / kpl_of(L.bits)));      // one group: every k maps to group 0
    a.waves = waves;
    const Lds l = lds_layout(L.K, a.groups, L.bits, act, pair, waves);
    a.off_xs0 = l.off_xs0; a.off_xs1 = l.off_xs1; a.off_cs = l.off_cs; a.cpad = l.cpad;
}

// moe_shared.hip: one launch of the routed experts alone at 2 or 3 bits -- moe_decode_body<T, BITS, PAIR, false> as a form of moe_shared_kernel (the
// library's kernel count is guarded: a form, not a kernel), on a.waves waves; grid, arguments and LDS bytes as moe_decode_kernel takes them
hipError_t launch_low_bit_form(bool pair, int dtype, int bits, const Args& a, dim3 grid, int lds, hipStream_t st);

static inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }      // the workspace's rounding
static inline bool any_perm(const gptq_layer_t* const* Ls, int E) {
    for (int e = 0; e < E; ++e)
        if (Ls[e]->perm) return true;
    return false;
}

}  // namespace moedec
}  // namespace gptq
