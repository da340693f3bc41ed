// grad_input_copy.hip -- the input gradient on the DECODE COPY: dX[M, K] (+)= dY[M, N] . W^T from qweight_tiled / qconst_tiled alone (gptq_grad_input_ex with
// GPTQ_GRAD_ON_COPY; opt-in).  The contract is grad_input.hip's: every weight is T(s * float(q - z)), bit-exact to gptq_dequant; products and sums in fp32 on the
// matrix core; one rounding at the store (accumulate: the old dX is added in fp32 first); no atomics, no workspace, a fixed summation order.  The checkpoint rows
// (qweight, qzeros, scales, g_idx) are never read, so a layer whose rows have left the device needs no rebuild pass in front of its backward.
//
// The copy holds, per strip of 16 columns and chunk of 128 k, one contiguous KiB in which lane (k-slot g = lane >> 4, column r = lane & 15) owns 16 bytes: 32
// consecutive k of ONE column n.  The reduction of this product runs over n, so the matrix core wants 8 consecutive n at one k: the kernel transposes through LDS.
//   work     a workgroup of 4 waves owns BM rows x 128 k (one chunk of the copy) of dX and walks N in stages of 4 strips (64 n); BM = 128, or 64 where 128-row
//            tiles give fewer than 256 workgroups (runtime-uniform).  The workgroup-id remap is grad_input.hip's: the k tiles of a row block share an XCD.
//   weights  per stage wave w loads the strip-chunk of strip 4 stage + w: ONE 16-byte load per lane; scale and zero-point from the (strip, group) record as the
//            rows kernel reads them (scale at 2 r, zero-point at 32 + r; group per chunk, per half or per k-slot by group mode -- stage-invariant per lane).
//            Deq1<T>::frag (mma_dequant.cuh, the packed magic-number decode) turns each of the lane's 4 words into 8 consecutive k of its column, in memory order.
//   image    each frag is ONE 16-byte LDS write into an [n][k] image: 64 rows (n) of 256 bytes (128 k).  The B fragments of v_mfma_f32_16x16x32 -- lane
//            (column k = lane & 15, g = lane >> 4) wants n = 8 g .. 8 g + 7 at its k -- come out of it with ds_read_b64_tr_b16, two per fragment: a 16-lane
//            group reads 4 rows (n) x 16 columns (k), lane 4 q + pp gives the address of row q, columns 4 pp .. 4 pp + 3, and lane i receives column i
//            (adapter_grad.hip uses the same mapping).  The first read takes n = 8 g + 0 .. 3, the second 8 g + 4 .. 7: the order ds_read_b128 gives dY.
//   swizzle  16-byte slot c (0 .. 15) of image row n lies at slot c ^ f(n & 15), f(v) = (v0 << 1) | (v1 << 2) | (v3 << 3) | v2 (a permutation of v's bits).
//            Write: the 16 lanes of a ds_write_b128 group hold 16 rows at one slot -> 16 different slots, all 64 banks.  Transposing read: a half-wave (g = 0, 1)
//            reads rows 8 g + q (+ 4), 32 bytes (an aligned slot pair) each: f >> 1 differs over those 8 rows -> 8 different pairs, all 64 banks.  Both free of
//            conflicts by the bank model the rest of the library uses (mma_dequant.cuh: swz); not measured with counters.
//   dY       [BM][64 n] copied to LDS as it lies (16-byte loads, swz() rows of 128 bytes), A fragments by ds_read_b128.  Rows past M repeat the last row (not
//            stored); a last stage with fewer than 4 strips clamps its strip index and zero-fills its dY columns.
//   pipeline two stage buffers (2 x (BM x 128 + 64 x 256) bytes = 64 KiB at BM = 128); the next stage's raw words (weights, constants, dY) are loaded into
//            registers before this stage's MFMAs and written to the other buffer behind them; one barrier per stage.
//   epilogue fp32 accumulators through LDS (the same 64 KiB) to rows.  Plain layers: 16-byte stores of 8 consecutive k.  Act-order layers: the copy is made of the
//            re-sequenced rows, so column k' of the tile is dX[:, perm[k']] (gptq_permute_columns: x_seq[:, i] = x[:, perm[i]]): each thread loads its 8 perm
//            entries once and stores 2-byte elements to the scattered columns (accumulate: the old value from the same address first).  No g_idx lookups,
//            no pre- or post-pass.
// BM, the group mode, act-order and accumulate are launch-uniform: one kernel per dtype.  So is the GROUPED form (moe_grad_copy.cuh, included behind the dense
// body): the down and the up stage of the routed layer's backward on the experts' copies, behind the mode word of the kernel's second argument.
//
// 2, 3 AND 8 BITS (GPTQ_GRAD_COPY_ANY_BITS; opt-in).  The width is a launch-uniform word too (Args::bits / Grouped::bits, the 4-bit bodies first in the code);
// only the weight FRONT-END (Front<T, BITS> below: the lane's raw loads and its image writes) differs, everything above is shared.  Every decoder returns 8
// consecutive k of the lane's column in memory order, so each frag is still ONE 16-byte write at slot (k of the frag) / 8 of row n, swizzled by the same f:
// the 16 lanes of a write group hold 16 rows at ONE logical slot whatever the slot is, so the write argument above holds for every width, and the reads are
// the 4-bit reads.
//   3 bits   a strip-chunk is 768 B; the lane's 3 words (32 k) in ONE 12-byte load; Deq1_3::frag(w, ks), ks = 0 .. 3 -> slot 4 g + ks.
//   2 bits   a strip-chunk is 512 B; the lane's 2 words (32 k) in ONE 8-byte load; the copy puts pair p = (k 16 w + 2 p, + 1) at bit 2 p of the halves of
//            word w, so Deq1_2::frag(word[ks >> 1] >> 8 (ks & 1)) is k = 8 ks .. 8 ks + 7 in memory order (as moe_rows.hip reads it) -> slot 4 g + ks:
//            no relabelling of dX columns is left to absorb.
//   8 bits   a chunk of the copy is 64 k (a lane owns 16 k), the tile two chunks: TWO 16-byte loads per lane, at k-slot 16 g of chunk 2 kt and of chunk
//            2 kt + 1; two Deq1_8::frag(q0, q1) per load -> slots 8 h + 2 g, 8 h + 2 g + 1 (h: the chunk).  The lane's two runs lie 64 k apart: it holds
//            two (scale, zero-point) pairs (group kt >> gshift | 2 kt + h | 4 kt + 2 h + (g >> 1)); the record is 64 B, the zero-point 2 bytes at 32 + 2 r
//            (gemm_rows_kernel.cuh).  A last tile with one chunk inside K reads that chunk twice (clamped index); its second half is never stored.
#include "common.cuh"
#include "mma_dequant.cuh"
#include "launch.h"

namespace gptq {
namespace gcopy {

constexpr int THREADS = 256;                // 4 waves: a strip each while dequantising; 2 (rows) x 2 (k halves of 64) on the matrix core
constexpr int BK = 128;                     // k per workgroup: one chunk of the copy
constexpr int BN = 64;                      // n per stage: 4 strips
constexpr int B_ROW = 256;                  // bytes of a weight image row: 128 k of one n
constexpr int B_BYTES = BN * B_ROW;
constexpr int LDS_BYTES = 65536;            // 2 x (BM x 128 + B_BYTES) at BM = 128 = the fp32 epilogue tile [128][128]

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

struct Args {
    const char* qw;              // qweight_tiled
    const char* qc;              // qconst_tiled
    const int* perm;             // act-order: original k of re-sequenced position i, else NULL
    const void* dy;
    void* dx;
    int M, K, N, strips, chunks, groups, gshift, gm, bm, nkt, accumulate;      // chunks: of the copy (128 k; 8 bits: 64 k); nkt: 128-k tiles
    int bits;
};

// image slot swizzle: a permutation of the row's low four bits whose upper three differ over rows {0..3, 8..11} and over {4..7, 12..15}
__device__ __forceinline__ int fswz(int v) { return ((v & 3) << 1) | (v & 8) | ((v >> 2) & 1); }

// The weight front-end of one lane: what it loads per stage (Raw) and how it writes the [n][k] image.  The lane's groups are the same in every stage.
struct W3 { unsigned x, y, z; };             // 12 bytes, 4-byte aligned: one global_load_dwordx3 that touches nothing behind them
template <typename T, int BITS>
struct Front {
    static constexpr int NH = BITS == 8 ? 2 : 1;                                  // chunks of the copy per tile = loads per lane and stage
    static constexpr unsigned LB = BITS == 3 ? 12u : (BITS == 2 ? 8u : 16u);      // a lane's bytes of a strip-chunk
    static constexpr unsigned WCH = 64u * LB, REC = BITS == 8 ? 64u : 48u;       // a strip-chunk of the copy, a constant record
    struct Raw {
        u32x4 q[NH];             // the lane's words (3 bits: x y z, 2 bits: x y)
        unsigned cs[NH], cz[NH]; // scale bits and zero-point of each run
    };
    const char* wsrc[NH];
    const char* qc;
    unsigned coff[NH], zoff[NH];
    size_t strip_w, strip_c;
    int wrow, wf, g;

    // chunks, groups, gshift, gm: the copy's (chunks of 128 k, at 8 bits of 64 k); kt: the 128-k tile
    __device__ __forceinline__ void init(const char* qw, const char* qc_, int chunks, int groups, int gshift, int gm, int kt, int lane, int wave) {
        const int r = lane & 15;
        g = lane >> 4;
        qc = qc_;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            int grp;
            if constexpr (BITS == 8) grp = gm == 0 ? (kt >> gshift) : (gm == 1 ? 2 * kt + h : 4 * kt + 2 * h + (g >> 1));
            else grp = gm == 0 ? (kt >> gshift) : (gm == 1 ? 2 * kt + (g >> 1) : 4 * kt + g);
            grp = min(grp, groups - 1);                    // (one group; the k-slots past K of a last, partial chunk)
            coff[h] = (unsigned)grp * REC + 2u * (unsigned)r;
            zoff[h] = (unsigned)grp * REC + 32u + (BITS == 8 ? 2u : 1u) * (unsigned)r;
            const int c = BITS == 8 ? min(2 * kt + h, chunks - 1) : kt;      // (8 bits, a last tile with one chunk inside K: that chunk again, never stored)
            wsrc[h] = qw + (size_t)c * WCH + (size_t)lane * LB;
        }
        strip_w = (size_t)chunks * WCH, strip_c = (size_t)groups * REC;
        wrow = (16 * wave + r) * B_ROW, wf = fswz(r);      // image row 16 wave + r
    }
    __device__ __forceinline__ void fetch(Raw& s, int strip) const {
        const char* rec = qc + (size_t)strip * strip_c;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const char* src = wsrc[h] + (size_t)strip * strip_w;
            if constexpr (BITS == 3) {
                const W3 w = *(const W3*)src;
                s.q[h] = u32x4{w.x, w.y, w.z, 0u};
            } else if constexpr (BITS == 2) {
                const u32x2 w = *(const u32x2*)src;
                s.q[h] = u32x4{w.x, w.y, 0u, 0u};
            } else {
                s.q[h] = *(const u32x4*)src;
            }
            s.cs[h] = *(const unsigned short*)(rec + coff[h]);
            if constexpr (BITS == 8) s.cz[h] = *(const unsigned short*)(rec + zoff[h]);
            else s.cz[h] = *(const unsigned char*)(rec + zoff[h]);
        }
    }
    // the lane's four writes: 8 consecutive k each, slot (k / 8) of its row
    __device__ __forceinline__ void store(const Raw& s, char* Bs) const {
        char* row = Bs + wrow;
        if constexpr (BITS == 4) {
            Deq1<T> dq;
            dq.setup(s.cs[0], s.cz[0]);
#pragma unroll
            for (int w = 0; w < 4; ++w) *(u32x4*)(row + (((4 * g + w) ^ wf) << 4)) = dq.frag(s.q[0][w]);
        } else if constexpr (BITS == 3) {
            Deq1_3<T> dq;
            dq.setup(s.cs[0], s.cz[0]);
            const u32x3 w3 = {s.q[0].x, s.q[0].y, s.q[0].z};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) *(u32x4*)(row + (((4 * g + ks) ^ wf) << 4)) = dq.frag(w3, ks);
        } else if constexpr (BITS == 2) {
            Deq1_2<T> dq;
            dq.setup(s.cs[0], s.cz[0]);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) *(u32x4*)(row + (((4 * g + ks) ^ wf) << 4)) = dq.frag(s.q[0][ks >> 1] >> (8 * (ks & 1)));
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                Deq1_8<T> dq;
                dq.setup(s.cs[h], s.cz[h]);
                *(u32x4*)(row + (((8 * h + 2 * g) ^ wf) << 4)) = dq.frag(s.q[h].x, s.q[h].y);
                *(u32x4*)(row + (((8 * h + 2 * g + 1) ^ wf) << 4)) = dq.frag(s.q[h].z, s.q[h].w);
            }
        }
    }
};

// B fragment: n = 8 g .. 8 g + 7 (rows at, at + 4 rows) at the lane's k, transposed out of the image
__device__ __forceinline__ u32x4 tr_fragment(const char* lo_at, const char* hi_at) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lo_at);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)hi_at);
    const u32x2 l = __builtin_bit_cast(u32x2, lo), h = __builtin_bit_cast(u32x2, hi);
    return u32x4{l.x, l.y, h.x, h.y};
}

template <typename T, int RB, int BITS>
__device__ __forceinline__ void run(const Args& p, char* smem, int m0, int kt) {
    constexpr int BM = RB * 32;
    constexpr int NA = BM * 8 / THREADS;                  // dY slots per thread
    constexpr int BUF = BM * 128 + B_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wk = wave & 1;
    const int M = p.M, K = p.K, N = p.N, k0 = kt * BK;
    const T* __restrict__ dy = (const T*)p.dy;

    typedef Front<T, BITS> F;
    F fr;
    fr.init(p.qw, p.qc, p.chunks, p.groups, p.gshift, p.gm, kt, lane, wave);
    // the raw words one thread loads for a stage
    struct Stage {
        u32x4 a[NA];             // dY: 16-byte slots of the A image
        typename F::Raw w;       // the lane's weights and their constants
    };

    auto fetch = [&](Stage& s, int it) {
        const int n0 = it * BN;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int c = tid + THREADS * i, row = c >> 3, sl = c & 7;
            const int m = min(m0 + row, M - 1);            // rows past M repeat the last one (their outputs are not stored)
            s.a[i] = n0 + sl * 8 < N ? *(const u32x4*)(dy + (size_t)m * N + n0 + sl * 8) : u32x4{0, 0, 0, 0};
        }
        fr.fetch(s.w, min(4 * it + wave, p.strips - 1));   // past the last strip: a strip again, against zero dY columns
    };

    // image offsets: the lane's writes (Front::store: row 16 wave + r) ...
    auto store = [&](const Stage& s, char* buf) {
        char* As = buf;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int c = tid + THREADS * i;
            *(u32x4*)(As + swz(c >> 3, c & 7)) = s.a[i];
        }
        fr.store(s.w, buf + BM * 128);
    };
    // ... and its transposing reads: row 8 g + q (second read: + 4), the 8 bytes at k = 64 wk + 16 j + 4 pp -> slot 8 wk + 2 j + (pp >> 1), half pp & 1.
    // 2 j touches bits 1, 2 of the slot alone, so block j is the j = 0 address ^ 32 j; the second row flips bit 0 of f
    const int q = r >> 2, pp = r & 3;
    const int rf = fswz(8 * (g & 1) + q);
    const int rd_lo = (8 * g + q) * B_ROW + (((8 * wk + (pp >> 1)) ^ rf) << 4) + 8 * (pp & 1);
    const int rd_hi = (8 * g + q + 4) * B_ROW + (((8 * wk + (pp >> 1)) ^ rf ^ 1) << 4) + 8 * (pp & 1);

    f32x4 acc[RB][4];
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int stages = (N + BN - 1) / BN;
    Stage st;
    fetch(st, 0);
    store(st, smem);
    __syncthreads();
    const int arow = wm * (BM / 2) + r;
    for (int it = 0; it < stages; ++it) {
        const bool more = it + 1 < stages;
        if (more) fetch(st, it + 1);
        const char* As = smem + (it & 1) * BUF;
        const char* Bs = As + BM * 128;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u32x4 a[RB], b[4];
#pragma unroll
            for (int i = 0; i < RB; ++i) a[i] = *(const u32x4*)(As + swz(arow + 16 * i, 4 * s + g));
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = tr_fragment(Bs + s * 32 * B_ROW + (rd_lo ^ (32 * j)), Bs + s * 32 * B_ROW + (rd_hi ^ (32 * j)));
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = Mma16<T>::run(a[i], b[j], acc[i][j]);
        }
        if (more) store(st, smem + ((it + 1) & 1) * BUF);
        __syncthreads();
    }

    // epilogue: [BM][128] fp32 through LDS (column ^ 16 on odd rows, as grad_input.hip)
    float* E = (float*)smem;
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = wm * (BM / 2) + 16 * i + 4 * g + e, col = wk * 64 + 16 * j + r;
                E[row * BK + (col ^ ((row & 1) << 4))] = acc[i][j][e];
            }
    __syncthreads();
    T* __restrict__ dx = (T*)p.dx;
    const int c8 = (tid & 15) * 8, k = k0 + c8;           // the thread's 8 columns: the same in every item (THREADS % 16 == 0)
    if (k >= K) return;                                    // (K % 32 == 0: 8 columns are inside or outside as a whole; no barrier follows)
    int pk[8];
    if (p.perm) {
        const u32x4 p0 = *(const u32x4*)(p.perm + k), p1 = *(const u32x4*)(p.perm + k + 4);
        pk[0] = p0.x; pk[1] = p0.y; pk[2] = p0.z; pk[3] = p0.w; pk[4] = p1.x; pk[5] = p1.y; pk[6] = p1.z; pk[7] = p1.w;
    }
#pragma unroll
    for (int i = 0; i < BM * 16 / THREADS; ++i) {
        const int row = (tid + THREADS * i) >> 4;
        const int m = m0 + row;
        if (m >= M) continue;
        const float* e = E + row * BK + (c8 ^ ((row & 1) << 4));
        const f32x4 lo = *(const f32x4*)e, hi = *(const f32x4*)(e + 4);
        float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        T* orow = dx + (size_t)m * K;
        if (p.perm) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                T* o = orow + pk[c];
                if (p.accumulate) v[c] += DType<T>::to_f32(*o);
                *o = DType<T>::from_f32(v[c]);
            }
        } else {
            T* out = orow + k;
            if (p.accumulate) {
                float old[8];
                unpack8<T>(*(const u32x4*)out, old);
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] += old[c];
            }
            const u32x2 w0 = pack4<T>(f32x4{v[0], v[1], v[2], v[3]}), w1 = pack4<T>(f32x4{v[4], v[5], v[6], v[7]});
            *(u32x4*)out = u32x4{w0.x, w0.y, w1.x, w1.y};
        }
    }
}

template <typename T, int BITS>
__device__ __forceinline__ void run_dense(const Args& p, char* smem) {
    const int b = xcd_remap(blockIdx.x, gridDim.x);        // consecutive k tiles of one row block on one XCD: they share dY in its L2
    const int kt = b % p.nkt, mt = b / p.nkt;
    if (p.bm == 128) run<T, 4, BITS>(p, smem, mt * 128, kt);
    else run<T, 2, BITS>(p, smem, mt * 64, kt);
}

}  // namespace gcopy
}  // namespace gptq

#include "moe_grad_copy.cuh"

namespace gptq {
namespace gcopy {

template <typename T>
__global__ void __launch_bounds__(THREADS, 2) grad_copy_kernel(Args p, Grouped q) {
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    if (__builtin_expect(q.mode == GR_DENSE, 1)) {         // (launch-uniform; the dense bodies first in the code, the 4-bit ones first among them)
        if (__builtin_expect(p.bits == 4, 1)) run_dense<T, 4>(p, smem);
        else if (p.bits == 3) run_dense<T, 3>(p, smem);
        else if (p.bits == 2) run_dense<T, 2>(p, smem);
        else run_dense<T, 8>(p, smem);
        return;
    }
    if (__builtin_expect(q.bits == 4, 1)) run_grouped<T, 4>(q, smem);
    else if (q.bits == 3) run_grouped<T, 3>(q, smem);
    else if (q.bits == 2) run_grouped<T, 2>(q, smem);
    else run_grouped<T, 8>(q, smem);
}

}  // namespace gcopy

// The one place the qualification rule lives: gptq_describe_grad_input_plan prints it, gptq_grad_input_ex launches by it.  Pure host arithmetic.
// GPTQ_GRAD_ON_COPY alone takes 4-bit layers; | GPTQ_GRAD_COPY_ANY_BITS also 2, 3 and 8 bits.  (A 2-bit layer's copy has ONE layout, whether or not
// tiled_cols carries GPTQ_COPY_ROWS_INT2 / _WIDE -- those bits choose forward kernels; copy_cols() masks them.)
GradCopyPlan plan_grad_copy(const gptq_layer_t& L, int M, int flags) {
    GradCopyPlan pl{};
    auto no = [&](const char* why) { pl.why = why; return pl; };
    if (!(flags & GPTQ_GRAD_ON_COPY)) return no("flag_off");
    const bool any = (flags & GPTQ_GRAD_COPY_ANY_BITS) != 0;
    if (L.bits != 4 && !(any && (L.bits == 2 || L.bits == 3 || L.bits == 8))) return no("bits");
    if (L.dtype != GPTQ_F16 && L.dtype != GPTQ_BF16) return no("dtype");
    // (an act-order layer's copy is made of its re-sequenced rows: without perm the kernel cannot name its output columns)
    if (!L.qweight_tiled || !L.qconst_tiled || copy_cols(L) != GPTQ_STRIP_COLS || (L.g_idx && !L.perm) || L.K % 32 || L.N % GPTQ_STRIP_COLS) return no("no_copy");
    const int gs = L.group_size;
    if (gs == 32) pl.gm = 2;
    else if (gs == 64) pl.gm = 1;
    else if (gs >= L.K) pl.gshift = 31;
    else if (gs > 0 && gs % 128 == 0 && ((gs / 128) & (gs / 128 - 1)) == 0) {
        while ((128 << pl.gshift) < gs) ++pl.gshift;
    } else return no("group_size");
    pl.bits = L.bits;
    pl.groups = gs >= L.K ? 1 : (L.K + gs - 1) / gs;
    pl.chunks = (L.K + 127) / 128;
    pl.stages = (L.N + gcopy::BN - 1) / gcopy::BN;
    pl.act = L.g_idx != nullptr;
    // 128-row tiles where they still give 256 workgroups (a full round at one per CU), else 64 rows: grad_input.hip's rule
    pl.bm = ((long)(M + 127) / 128) * pl.chunks >= 256 ? 128 : 64;
    pl.blocks = (long)pl.chunks * ((M + pl.bm - 1) / pl.bm);
    pl.ok = M > 0 && pl.blocks <= 0x7fffffffL;
    if (!pl.ok) pl.why = "no_copy";
    return pl;
}

hipError_t launch_grad_copy(const gptq_layer_t& L, const GradCopyPlan& pl, const void* dy, void* dx, int M, int accumulate, hipStream_t st) {
    if (!pl.ok) return hipErrorInvalidValue;
    gcopy::Args p;
    p.qw = (const char*)L.qweight_tiled;
    p.qc = (const char*)L.qconst_tiled;
    p.perm = pl.act ? L.perm : nullptr;
    p.dy = dy;
    p.dx = dx;
    p.M = M, p.K = L.K, p.N = L.N, p.strips = L.N / GPTQ_STRIP_COLS, p.groups = pl.groups, p.gshift = pl.gshift, p.gm = pl.gm;
    p.chunks = pl.bits == 8 ? (L.K + 63) / 64 : pl.chunks;      // (the 8-bit copy's chunks are 64 k deep)
    p.bm = pl.bm, p.nkt = pl.chunks, p.accumulate = accumulate ? 1 : 0, p.bits = pl.bits;
    const dim3 grid((unsigned)pl.blocks), block(gcopy::THREADS);
    gcopy::Grouped q{};                                    // GR_DENSE
    if (L.dtype == GPTQ_F16) hipLaunchKernelGGL(gcopy::grad_copy_kernel<f16>, grid, block, 0, st, p, q);
    else hipLaunchKernelGGL(gcopy::grad_copy_kernel<bf16>, grid, block, 0, st, p, q);
    return hipGetLastError();
}

// The grouped form's qualification: every layer of the three projections by the dense rule above (ONE width -- mixed widths are declined as a whole --, fp16 /
// bf16, a 16-column copy, the group sizes), its copies 16-byte aligned.  W1 and W3 share one up-stage launch where every expert's gate and up name the same
// output columns: both plain, or one perm pointer.
MoeGradCopyPlan plan_moe_grad_copy(const gptq_moe_t& m, int flags) {
    MoeGradCopyPlan pl{};
    pl.up_launches = 1;
    pl.bits = m.gate[0]->bits;
    const gptq_layer_t* const* proj[3] = {m.gate, m.up, m.down};
    auto cols = [](const gptq_layer_t& L) { return L.qweight_seq ? L.perm : nullptr; };      // as the decode table's entry names them
    for (int ps = 0; ps < 3; ++ps)
        for (int e = 0; e < m.E; ++e) {
            const gptq_layer_t& L = *proj[ps][e];
            const GradCopyPlan lp = plan_grad_copy(L, gcopy::GBM, flags);
            if (!lp.ok) { pl.why = lp.why; return pl; }
            if (L.bits != pl.bits) { pl.why = "bits"; return pl; }
            if (((uintptr_t)L.qweight_tiled | (uintptr_t)L.qconst_tiled) & 15) { pl.why = "no_copy"; return pl; }
            pl.act = pl.act || lp.act;
            if (e == 0 && ps == 0) pl.gm1 = lp.gm, pl.gshift1 = lp.gshift, pl.groups1 = lp.groups;
            if (e == 0 && ps == 2) pl.gm2 = lp.gm, pl.gshift2 = lp.gshift, pl.groups2 = lp.groups;
        }
    for (int e = 0; e < m.E; ++e)
        if (cols(*m.gate[e]) != cols(*m.up[e])) pl.up_launches = 2;
    pl.ok = true;
    return pl;
}

// The down stage and the up stage (one launch, or W1 then W3 in stream order) of launch_moe_grad on the decode table.
hipError_t launch_moe_grad_copy_stages(const gptq_moe_t& m, const MoeGradCopyPlan& cp, const void* decode_table, const MoeGradPlan& pl, const void* dout,
                                       const float* w, int topk, bool want_dx, bool want_dw, char* ws, hipStream_t st) {
    if (!cp.ok || !decode_table) return hipErrorInvalidValue;
    const gptq_layer_t& G = *m.gate[0];
    gcopy::Args none{};
    gcopy::Grouped q{};
    q.E = m.E; q.topk = topk; q.H = G.K; q.I = G.N;
    q.bits = cp.bits;
    q.table = (const moerows::Entry*)decode_table;
    q.dout = dout; q.w = w;
    q.row_assign = (const int*)(ws + pl.off_rows); q.tile_count = (const int*)(ws + pl.off_tile_count); q.tiles = (const int4*)(ws + pl.off_tiles);
    q.g = ws + pl.off_g; q.u = ws + pl.off_u;
    q.dwp = want_dw ? (float*)(ws + pl.off_dwp) : nullptr;
    q.dxr = (float*)(ws + pl.off_dxr);
    q.gm1 = cp.gm1; q.gshift1 = cp.gshift1; q.groups1 = cp.groups1;
    q.gm2 = cp.gm2; q.gshift2 = cp.gshift2; q.groups2 = cp.groups2;
    auto stage = [&](int mode, int nkt) -> hipError_t {
        const long blocks = (long)pl.tiles * nkt;
        if (blocks <= 0) return hipSuccess;
        if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
        q.mode = mode; q.nkt = nkt;
        if (G.dtype == GPTQ_F16) hipLaunchKernelGGL(gcopy::grad_copy_kernel<f16>, dim3((unsigned)blocks), dim3(gcopy::THREADS), 0, st, none, q);
        else hipLaunchKernelGGL(gcopy::grad_copy_kernel<bf16>, dim3((unsigned)blocks), dim3(gcopy::THREADS), 0, st, none, q);
        return hipGetLastError();
    };
    hipError_t e = stage(gcopy::GR_DOWN, pl.nblk_i);
    if (e != hipSuccess || !want_dx) return e;
    if (cp.up_launches == 1) return stage(gcopy::GR_UP, pl.nblk_h);
    if ((e = stage(gcopy::GR_UP1, pl.nblk_h)) != hipSuccess) return e;
    return stage(gcopy::GR_UP3, pl.nblk_h);
}

}  // namespace gptq
