// moe_decode.hip -- routed mixture-of-experts layers at decode row counts (gptq_moe_decode_forward): 1..4 tokens on the experts' DECODE COPY.
//
// What one call computes (T <= 4 tokens, topk assignments r = (t, j) each, expert e = topk_idx[t, j]; indices outside [0, E) are dropped):
//   g = x_t . W1_e,  u = x_t . W3_e          fp32
//   h_r = T(silu(g) * u)                     silu and the product on the fp32 sums, one rounding
//   out[t] = T(sum_j w[t, j] * (h_r . W2_e)) fp32, ascending j, one rounding; a token without a valid expert gets 0
// ARITHMETIC CONTRACT: that of the dense decode-copy kernel (gemv_tiled_kernel.cuh), NOT the grouped path's "every W bit-exact to gptq_dequant":
// w - z is exact in the layer dtype, every product x (w - z) is exact in fp32, a lane sums the KPL consecutive k of its column on the matrix core
// (v_mfma_f32_4x4x4_16b) in fp32, and the group's scale multiplies that fp32 sum (fmaf into the lane's accumulator).  W is never rounded to the layer dtype.
// Two launches, no routing launch, no host round trip (capturable): the expert of an assignment is read from topk_idx by the workgroup that serves it.
//   1. moe_decode_kernel<T, BITS, true>   grid (I / 16, T topk): a workgroup = one assignment x one 16-column strip of I.  It reads e (uniform), the two
//      entries of the device table (ONE dependent load each: decode-copy pointers and perm of W1_e / W3_e), stages the raw x_t and the two strips' constants
//      in the LDS by DMA, then the first half of its waves streams strip s of W1_e and the second half strip s of W3_e.  Act-order experts: each half gathers
//      x through its own projection's perm LDS -> LDS (one gather by all waves when the two pointers are equal).  Waves meet in the LDS, thread c < 16 adds
//      the halves' partials in wave order and stores h[r][16 s + c].  Workgroups of strip 0 also write pos[r] (r, or -1 for a dropped assignment).
//   2. moe_decode_kernel<T, BITS, false>  grid (H / 16, T): a workgroup = one token x one 16-column strip of H.  It walks the token's assignments in
//      ascending j: stages h_r (gathered through W2_e's perm for act-order experts), all waves stream strip s of W2_e, cross-wave sum in wave order, and
//      thread c keeps total += w[t, j] * sum in a register; one rounding at the store.  (The alternative -- a workgroup per (assignment, strip) into fp32
//      rows plus moe_combine_kernel, three launches -- computes the same bits; it is not built: DESIGN 4.8.)
// No K slices, no atomics: every output is one thread's sum in a fixed order, so results are bit-reproducible and the row of token t does not depend on the
// other tokens of the call.
// Layout read: gptq_layer_t.qweight_tiled / qconst_tiled (include/gptq_mi355x.h): a strip is one contiguous run, a chunk (4 k-slots x 16 columns) one wave
// load, lane (kb, col) holds KPL consecutive k of one column.
#include <string.h>

#include <algorithm>

#include "gemv_tiled_kernel.cuh"     // TiledFmt<BITS>, WordsOf, and through gemv_shared.cuh: Mma4, kslot_sum_swap, dma16_nt

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

// The table entry of an expert: every lane loads the same 32 bytes; readfirstlane makes the pointers scalars for the compiler (uniform branches, SGPR bases).
typedef unsigned u32x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ Entry load_entry(const Entry* p) {
    const u32x8 v = *(const u32x8*)p;
    u32x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = __builtin_amdgcn_readfirstlane(v[i]);
    return __builtin_bit_cast(Entry, o);
}

template <typename T, int BITS, bool PAIR>
__global__ void __launch_bounds__(1024) moe_decode_kernel(Args p) {
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
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, kb = lane >> 4;
    const int W = p.waves, K = p.K, N = p.N, G = p.groups, nchunks = p.chunks, gshift = p.gshift, E = p.E, topk = p.topk;
    const int strip = blockIdx.x;
    const int Wh = PAIR ? (W >> 1) : W;                                           // waves per streamed strip
    const int sel = PAIR ? (wave >= Wh ? 1 : 0) : 0;                              // pair: 0 = gate (W1), 1 = up (W3)
    const int wv = wave - sel * Wh;
    char* const xraw = smem;
    char* const xs0 = smem + p.off_xs0;
    char* const xs1 = smem + p.off_xs1;
    char* const cs = smem + p.off_cs + sel * p.cpad;
    float* const red = (float*)(smem + p.off_cs + (PAIR ? 2 : 1) * p.cpad);
    const unsigned t_lane = (unsigned)lane * (WPL * 4u);
    const f16x2 k960 = {(f16)960.f, (f16)960.f};
    const f16x2 r16 = {(f16)0.0625f, (f16)0.0625f};
    auto bits_of = [&](f16x2 hv) -> unsigned {                                    // the pair as the matrix core takes it (bf16: fp16 -> fp32 -> bf16, exact: small integers)
        if constexpr (BF) {
            const bf16x2 o = {(bf16)(float)hv[0], (bf16)(float)hv[1]};
            return __builtin_bit_cast(unsigned, o);
        } else {
            return __builtin_bit_cast(unsigned, hv);
        }
    };

    const int first = PAIR ? (int)blockIdx.y : (int)blockIdx.y * topk;            // pair: the assignment; down: the token's first assignment
    const int count = PAIR ? 1 : topk;
    float total = 0.f;                                                            // down: thread c < 16 -- sum_j w[t, j] * (h_r . W2_e)[16 s + c]
    for (int jj = 0; jj < count; ++jj) {
        const int r = first + jj;
        const long long ev = p.idx[r];
        const float wr = p.w[r];
        const int e = __builtin_amdgcn_readfirstlane((ev >= 0 && ev < (long long)E) ? (int)ev : -1);
        if constexpr (PAIR) {
            if (strip == 0 && tid == 0) p.pos[r] = e >= 0 ? r : -1;
        }
        if (e < 0) continue;                                                      // uniform: a dropped assignment
        const Entry e0 = load_entry(p.table + e);
        const unsigned* tq0 = e0.tq;
        const char* cst0 = (const char*)e0.cst;
        const int* perm0 = e0.perm;
        const unsigned* tq1 = tq0;
        const char* cst1 = cst0;
        const int* perm1 = perm0;
        if constexpr (PAIR) {
            const Entry e1 = load_entry(p.table + E + e);
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
        const char* const arow = (const char*)p.a + (size_t)(PAIR ? r / topk : r) * K * 2;
        // ---- stage the raw activation row and the constants by LDS DMA, issued FIRST (loads return in issue order), waited for behind the first weight burst
        {
            const unsigned x_lds = lds_addr_of(xraw), c_lds = lds_addr_of(smem + p.off_cs);
            const int pieces = K >> 3;                                            // 16-byte pieces of the row
            for (int pc0 = wave * 64; pc0 < pieces; pc0 += W * 64)                // wave-uniform trip count
                if (pc0 + lane < pieces) lds_dma16(arow + (size_t)(pc0 + lane) * 16, x_lds + pc0 * 16);
            const int cpieces = (G * REC) >> 4;                                   // REC is a multiple of 16
            const char* const cg0 = cst0 + (size_t)strip * G * REC;
            for (int pc0 = wave * 64; pc0 < cpieces; pc0 += W * 64)
                if (pc0 + lane < cpieces) dma16_nt(cg0 + (size_t)(pc0 + lane) * 16, __builtin_amdgcn_readfirstlane(c_lds + pc0 * 16));
            if constexpr (PAIR) {
                const char* const cg1 = cst1 + (size_t)strip * G * REC;
                for (int pc0 = wave * 64; pc0 < cpieces; pc0 += W * 64)
                    if (pc0 + lane < cpieces) dma16_nt(cg1 + (size_t)(pc0 + lane) * 16, __builtin_amdgcn_readfirstlane(c_lds + (unsigned)p.cpad + pc0 * 16));
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
                        const int gt = same ? tid : tid - sel * Wh * 64, gn = same ? W * 64 : Wh * 64;
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
                } else {
#pragma unroll
                    for (int w = 0; w < 4; ++w) {                                 // one word = 4 k = one matrix-core step
                        const unsigned qw = qv[w], q8 = qw >> 8;
                        const f16x2 h0 = as_f16x2((qw & m_b) | magic) + c1;       // k0,k1  (stored bytes 0 and 2)
                        const f16x2 h1 = as_f16x2((q8 & m_b) | magic) + c1;       // k2,k3  (1 and 3)
                        mm(w >> 1, w & 1, bits_of(h0), bits_of(h1));
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
                ((T*)p.out)[(size_t)r * N + strip * 16 + tid] = DType<T>::from_f32(gv * s1);
            }
        } else {
            if (tid < 16) {
                float s0 = 0.f;
                for (int w = 0; w < W; ++w) s0 += red[w * ES + tid];
                total += wr * s0;
            }
            // the next assignment's DMAs overwrite the row and the constants: every wave is past its K loop here (the barrier above); the sums are
            // written again only behind the next staging barrier, which thread c reaches after it has read them
        }
    }
    if constexpr (!PAIR) {
        if (tid < 16) ((T*)p.out)[(size_t)blockIdx.y * N + strip * 16 + tid] = DType<T>::from_f32(total);
    }
}

template <typename T, int BITS, bool PAIR>
static hipError_t launch_one(const Args& a, dim3 grid, int lds, hipStream_t st) {
    hipLaunchKernelGGL((moe_decode_kernel<T, BITS, PAIR>), grid, dim3(a.waves * 64), lds, st, a);
    return hipGetLastError();
}
template <bool PAIR>
static hipError_t launch_any(int dtype, int bits, const Args& a, dim3 grid, int lds, hipStream_t st) {
    if (dtype == GPTQ_F16) return bits == 4 ? launch_one<f16, 4, PAIR>(a, grid, lds, st) : launch_one<f16, 8, PAIR>(a, grid, lds, st);
    return bits == 4 ? launch_one<bf16, 4, PAIR>(a, grid, lds, st) : launch_one<bf16, 8, PAIR>(a, grid, lds, st);
}

// waves that stream one strip: one per U chunks of the strip, so that no wave runs the K loop on clamped chunks only (I = 1408 at 4 bits is 11 chunks: 3 waves)
static int waves_for(int K, int bits, bool pair) {
    const int cke = bits == 8 ? 64 : 128, chunks = (K + cke - 1) / cke, per = (chunks + U - 1) / U;
    return pair ? 2 * std::min(MAX_WAVES_PAIR / 2, per) : std::min(MAX_WAVES_DOWN, per);
}

struct Lds { int off_xs0, off_xs1, off_cs, cpad, bytes; };
static Lds lds_layout(int K, int groups, int bits, bool act, bool pair, int waves) {
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

}  // namespace moedec

static size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }
static int kpl_of(int bits) { return bits == 8 ? 16 : 32; }
static bool any_perm(const gptq_layer_t* const* Ls, int E) {
    for (int e = 0; e < E; ++e)
        if (Ls[e]->perm) return true;
    return false;
}

MoeDecodePlan plan_moe_decode(const gptq_moe_t& m, int T, int topk) {
    MoeDecodePlan pl{};
    const gptq_layer_t& G = *m.gate[0];
    const gptq_layer_t& D = *m.down[0];
    const int H = G.K, I = G.N;
    const bool act_pair = any_perm(m.gate, m.E) || any_perm(m.up, m.E), act_down = any_perm(m.down, m.E);
    pl.waves_pair = moedec::waves_for(H, G.bits, true);
    pl.waves_down = moedec::waves_for(I, D.bits, false);
    pl.lds_pair = moedec::lds_layout(H, (H + G.group_size - 1) / G.group_size, G.bits, act_pair, true, pl.waves_pair).bytes;
    pl.lds_down = moedec::lds_layout(I, (I + D.group_size - 1) / D.group_size, D.bits, act_down, false, pl.waves_down).bytes;
    pl.ok = pl.lds_pair <= moedec::MAX_LDS && pl.lds_down <= moedec::MAX_LDS;
    pl.wg_pair = T * topk * (I / 16);
    pl.wg_down = T * (H / 16);
    const size_t R = (size_t)T * topk;
    size_t o = GPTQ_WORKSPACE_HEADER_BYTES;                      // the header of a shared workspace belongs to the other entry points: left as it is
    pl.off_h = o; o += a256(R * I * dtype_size(G.dtype));
    pl.off_pos = o; o += a256(4 * R);
    pl.bytes = o;
    return pl;
}

hipError_t launch_moe_decode(const gptq_moe_t& m, const void* table, const MoeDecodePlan& pl, const void* x, const int64_t* idx, const float* w, int T, int topk,
                             void* out, char* ws, hipStream_t st) {
    const gptq_layer_t& G = *m.gate[0];
    const gptq_layer_t& D = *m.down[0];
    const int E = m.E, H = G.K, I = G.N;
    auto fill = [&](moedec::Args& a, const gptq_layer_t& L, bool act, bool pair, int waves) {
        const int cke = 4 * kpl_of(L.bits);
        a.E = E; a.topk = topk; a.K = L.K; a.N = L.N;
        a.chunks = (L.K + cke - 1) / cke;
        a.groups = (L.K + L.group_size - 1) / L.group_size;
        a.gshift = L.group_size >= L.K ? 26 : __builtin_ctz((unsigned)(L.group_size / kpl_of(L.bits)));      // one group: every k maps to group 0
        a.waves = waves;
        const moedec::Lds l = moedec::lds_layout(L.K, a.groups, L.bits, act, pair, waves);
        a.off_xs0 = l.off_xs0; a.off_xs1 = l.off_xs1; a.off_cs = l.off_cs; a.cpad = l.cpad;
    };
    moedec::Args g{};
    g.table = (const moedec::Entry*)table;
    g.idx = (const long long*)idx; g.w = w; g.a = x; g.out = ws + pl.off_h; g.pos = (int*)(ws + pl.off_pos);
    fill(g, G, any_perm(m.gate, E) || any_perm(m.up, E), true, pl.waves_pair);
    hipError_t e = moedec::launch_any<true>(G.dtype, G.bits, g, dim3(I / 16, T * topk), pl.lds_pair, st);
    if (e != hipSuccess) return e;
    moedec::Args d{};
    d.table = (const moedec::Entry*)table + 2 * (size_t)E;
    d.idx = g.idx; d.w = w; d.a = ws + pl.off_h; d.out = out; d.pos = nullptr;
    fill(d, D, any_perm(m.down, E), false, pl.waves_down);
    return moedec::launch_any<false>(D.dtype, D.bits, d, dim3(H / 16, T), pl.lds_down, st);
}

size_t moe_decode_table_entry_bytes() { return sizeof(moedec::Entry); }

void moe_decode_table_entry(const gptq_layer_t& L, void* dst) {
    moedec::Entry p;
    p.tq = L.qweight_tiled;
    p.cst = L.qconst_tiled;
    p.perm = L.qweight_seq ? L.perm : nullptr;
    p.reserved = nullptr;
    memcpy(dst, &p, sizeof(p));
}

// grants > 64 KiB of dynamic LDS (long K of act-order experts: the raw and the gathered row next to the constants)
hipError_t init_moe_decode_device() {
    hipError_t e = hipSuccess;
    auto grant = [&](auto kern) { hipError_t r = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, moedec::MAX_LDS); if (e == hipSuccess) e = r; };
    grant(moedec::moe_decode_kernel<f16, 4, true>); grant(moedec::moe_decode_kernel<f16, 4, false>);
    grant(moedec::moe_decode_kernel<f16, 8, true>); grant(moedec::moe_decode_kernel<f16, 8, false>);
    grant(moedec::moe_decode_kernel<bf16, 4, true>); grant(moedec::moe_decode_kernel<bf16, 4, false>);
    grant(moedec::moe_decode_kernel<bf16, 8, true>); grant(moedec::moe_decode_kernel<bf16, 8, false>);
    return e;
}

}  // namespace gptq
