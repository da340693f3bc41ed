// moe_grad_copy.cuh -- the GROUPED form of grad_copy_kernel (grad_input_copy.hip includes this behind its dense body): the two transposed stages of the
// routed layer's backward (gptq_moe_backward_ex with GPTQ_GRAD_ON_COPY; moe_grad.hip has the formulas and the other three launches) from the experts'
// qweight_tiled / qconst_tiled alone.  A launch-uniform mode of the dense kernel -- no kernel of its own: the data movement is the dense body's at RB = 2
// (one 16-byte weight load per lane, Deq1<T>::frag, four 16-byte writes into the swizzled [n][k] image, B fragments by ds_read_b64_tr_b16, A rows copied
// as they lie and read by ds_read_b128, two stage buffers, one barrier per stage); only what routing forces differs:
//   work     a workgroup owns one routing tile (<= 64 rows of one expert, moe_route_kernel with bm = 64) x one chunk of the copy (128 output columns);
//            moe_grad.hip's remap (the column blocks of a tile share an XCD) and its early return for tiles past the routing kernel's count.  16-row
//            blocks the tile does not have skip their MFMAs.
//   weights  {qweight_tiled, qconst_tiled, perm} of (projection, expert) from the DECODE table (moe_entry.cuh).  H and I are multiples of 64: every stage
//            has its 4 strips; a partial last chunk (I = 192) decodes its padding k-slots against the last group and never stores them.
//   A rows   a pointer per row: dOut through row_assign / topk (down stage), dg then du (up stage); a row past the tile reads as zero.
//   down     moe_grad_kernel's epilogue.  Act-order W2: column k' of the tile is element perm2[k'] of the row -- G, U are read and dg, du written as
//            2-byte elements there (the thread that reads an element writes it); the dw partial sums the block's columns in ascending k'.
//   up       fp32 rows into DXR; act-order experts scatter through perm.  W1 and W3 run into one set of accumulators only where they name the same
//            output columns (GR_UP).  Otherwise two launches in stream order: GR_UP1 stores W1's rows, GR_UP3 LOADS its accumulators from DXR (through
//            W3's perm) before it walks W3 and stores them back -- the fp32 sums continue exactly where W1's ended, so every element sums its reduction
//            axis in the order of the one-launch form (and of moe_grad_kernel), and no two workgroups touch one element within a launch.
// 2 x (64 x 128 + 64 x 256) = 48 KiB of the kernel's 64; the fp32 epilogue tile [64][128] reuses them.
// 2, 3 and 8 bits (Grouped::bits, launch-uniform; GPTQ_GRAD_COPY_ANY_BITS): the dense body's front-ends (grad_input_copy.hip Front<T, BITS>), nothing else.
#pragma once
#include "moe_entry.cuh"

namespace gptq {
namespace gcopy {

enum { GR_DENSE = 0, GR_DOWN = 1, GR_UP = 2, GR_UP1 = 3, GR_UP3 = 4 };

struct Grouped {
    int mode;                                // GR_DENSE: the dense layer of Args, nothing below is read
    int bits;                                // the experts' width (one for gate, up and down)
    int E, topk, H, I, nkt;                  // nkt: 128-column blocks (chunks of the copy) of this stage's output
    const moerows::Entry* table;             // the decode table [3][E]: W1, W3, W2
    const void* dout;                        // [T][H]
    const float* w;                          // [T * topk]
    const int* row_assign;
    const int* tile_count;
    const int4* tiles;
    void* g;                                 // [R][I] T: G in, dg out (down stage); dg in (up stage)
    void* u;                                 // [R][I] T: U in, du out; du in
    float* dwp;                              // [R][nkt] or NULL
    float* dxr;                              // [R][H]
    int gm1, gshift1, groups1;               // the gate / up copies: group mode, chunk -> group shift, groups (over H)
    int gm2, gshift2, groups2;               // the down copies (over I)
};

constexpr int GBM = 64;                      // tile height (the routing kernel's bm): RB = 2
constexpr int GBUF = GBM * 128 + B_BYTES;    // one stage buffer: A image + weight image

// One copy as dX = A . W^T sees it: K output columns in `chunks` chunks, N reduction elements (N / 16 strips).
struct Copy {
    const char* qw;
    const char* qc;
    int N, chunks, groups, gshift, gm;       // chunks: of the copy (128 k; 8 bits: 64 k)
};

// acc += A[64][N] . W^T[N][128 kt .. 128 kt + 127]: a0 / a1 are rows (tid >> 3) and (tid >> 3) + 32 of A (NULL: a row the tile does not have), rb the
// number of 16-row blocks the tile has.  Ends behind a barrier: the LDS is free again.
template <typename T, int BITS>
__device__ __forceinline__ void walk(const Copy& p, const T* a0, const T* a1, int rb, char* smem, int kt, f32x4 (&acc)[2][4]) {
    const T* const arow[2] = {a0, a1};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wk = wave & 1;

    typedef Front<T, BITS> F;
    F fr;
    fr.init(p.qw, p.qc, p.chunks, p.groups, p.gshift, p.gm, kt, lane, wave);
    struct GStage {                          // the raw words one thread loads for a stage
        u32x4 a[2];                          // A: slot tid & 7 of rows tid >> 3 and (tid >> 3) + 32
        typename F::Raw w;                   // the lane's weights and their constants
    };

    auto fetch = [&](GStage& s, int it) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            s.a[i] = arow[i] ? *(const u32x4*)((const char*)(arow[i] + it * BN) + (tid & 7) * 16) : u32x4{0, 0, 0, 0};
        fr.fetch(s.w, 4 * it + wave);                     // (N % 64 == 0: the stage has its 4 strips)
    };
    auto store = [&](const GStage& s, char* buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *(u32x4*)(buf + swz((tid >> 3) + 32 * i, tid & 7)) = s.a[i];
        fr.store(s.w, buf + GBM * 128);
    };
    // the transposing reads: grad_input_copy.hip's run() derives the addresses
    const int q = r >> 2, pp = r & 3;
    const int rf = fswz(8 * (g & 1) + q);
    const int rd_lo = (8 * g + q) * B_ROW + (((8 * wk + (pp >> 1)) ^ rf) << 4) + 8 * (pp & 1);
    const int rd_hi = (8 * g + q + 4) * B_ROW + (((8 * wk + (pp >> 1)) ^ rf ^ 1) << 4) + 8 * (pp & 1);

    const int stages = p.N / BN;
    GStage st;
    fetch(st, 0);
    store(st, smem);
    __syncthreads();
    const int arow_l = wm * (GBM / 2) + r;
    for (int it = 0; it < stages; ++it) {
        const bool more = it + 1 < stages;
        if (more) fetch(st, it + 1);
        const char* As = smem + (it & 1) * GBUF;
        const char* Bs = As + GBM * 128;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u32x4 a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *(const u32x4*)(As + swz(arow_l + 16 * i, 4 * s + g));
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = tr_fragment(Bs + s * 32 * B_ROW + (rd_lo ^ (32 * j)), Bs + s * 32 * B_ROW + (rd_hi ^ (32 * j)));
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (2 * wm + i >= rb) continue;           // a 16-row block the tile does not have (uniform over the wave)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = Mma16<T>::run(a[i], b[j], acc[i][j]);
            }
        }
        if (more) store(st, smem + ((it + 1) & 1) * GBUF);
        __syncthreads();
    }
}

template <typename T>
__device__ __forceinline__ float elem16(const T* p) { return DType<T>::to_f32(*p); }

// The down stage's scalar epilogue gives moe_grad_kernel's bits, and that kernel's source leaves two things to the compiler: which products are fused
// into their add, and whether T(a * b) is one instruction (v_fma_mixlo_f16) or two (multiply to fp32, convert).  On an MI355X the two forms of T(a * b)
// do not always agree in the last bit, so the choices its object code makes -- the same in all eight item bodies of both types -- are written out here:
//   h_r[c]   fp16, columns 0 and 1 of a lane: v_fma_mixlo_f16; every other column, and bf16: multiply, convert
//   dg, du   multiply, convert
//   dw       columns 0 and 1 fused into the running sum, columns 2 .. 7 rounded before their add
// a * b rounded to fp32 (the empty asm keeps the product and a conversion that follows it two instructions)
__device__ __forceinline__ float prod(float a, float b) {
    float x = a * b;
    asm("" : "+v"(x));
    return x;
}
template <typename T>
__device__ __forceinline__ float h_mix(float silu, float u) { return DType<T>::to_f32(DType<T>::from_f32(prod(silu, u))); }
template <>
__device__ __forceinline__ float h_mix<f16>(float silu, float u) {
    unsigned d = 0;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "+v"(d) : "v"(silu), "v"(u));
    return DType<f16>::to_f32(__builtin_bit_cast(f16, (unsigned short)d));
}

template <typename T, int BITS>
__device__ __forceinline__ void run_grouped(const Grouped& p, char* smem) {
    const int b = xcd_remap(blockIdx.x, gridDim.x);        // consecutive column blocks of one tile on one XCD: they share the A rows in its L2
    const int kt = b % p.nkt, tile = b / p.nkt;
    if (tile >= *p.tile_count) return;
    const int4 tl = p.tiles[tile];
    const int e = tl.x, row0 = tl.y, rows = tl.z;
    const int rb = (rows + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wk = wave & 1;
    const int k0 = kt * BK;
    const int H = p.H, I = p.I;
    const bool up = p.mode != GR_DOWN;
    const int KO = up ? H : I;                             // this stage's output columns

    // the passes of this launch over the decode table's projections: W2 | W1, W3 | W1 | W3
    const int first = p.mode == GR_DOWN ? 2 : (p.mode == GR_UP3 ? 1 : 0);
    const int last = p.mode == GR_UP ? 1 : first;
    const int* perm = nullptr;                             // the output columns' perm: the last pass's (GR_UP: W1's and W3's are one)

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ps = first; ps <= last; ++ps) {
        const moerows::Entry en = moerows::load_entry(p.table + (size_t)ps * p.E + e);
        perm = en.perm;
        Copy W;
        W.qw = (const char*)en.tq; W.qc = (const char*)en.cst;
        constexpr int CK = BITS == 8 ? 64 : 128;          // k of a chunk of the copy
        if (up) { W.N = I; W.chunks = (H + CK - 1) / CK; W.groups = p.groups1; W.gshift = p.gshift1; W.gm = p.gm1; }
        else { W.N = H; W.chunks = (I + CK - 1) / CK; W.groups = p.groups2; W.gshift = p.gshift2; W.gm = p.gm2; }
        if (p.mode == GR_UP3) {
            // the sums continue where the W1 launch ended: its fp32 rows, in the accumulators' own layout, through THIS projection's columns
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + wk * 64 + 16 * j + r;
                if (k >= H) continue;
                const int col = perm ? perm[k] : k;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int row = wm * (GBM / 2) + 16 * i + 4 * g + c;
                        if (row < rows) acc[i][j][c] = p.dxr[(size_t)(row0 + row) * H + col];
                    }
            }
        }
        const T* arow[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rr = (tid >> 3) + 32 * i;
            if (rr >= rows) arow[i] = nullptr;
            else if (up) arow[i] = (const T*)(ps ? p.u : p.g) + (size_t)(row0 + rr) * I;
            else arow[i] = (const T*)p.dout + (size_t)(p.row_assign[row0 + rr] / p.topk) * H;
        }
        walk<T, BITS>(W, arow[0], arow[1], rb, smem, kt, acc);
    }

    // epilogue: [64][128] fp32 through LDS (column ^ 16 on odd rows, as the dense body)
    float* E = (float*)smem;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int row = wm * (GBM / 2) + 16 * i + 4 * g + c, col = wk * 64 + 16 * j + r;
                E[row * BK + (col ^ ((row & 1) << 4))] = acc[i][j][c];
            }
    __syncthreads();
    const int c8 = (tid & 15) * 8, k = k0 + c8;            // the thread's 8 columns: the same in every item; inside or outside KO as a whole (KO % 64 == 0)
    const bool inside = k < KO;
    int pk[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) pk[c] = k + c;
    if (perm && inside) {
        const u32x4 p0 = *(const u32x4*)(perm + k), p1 = *(const u32x4*)(perm + k + 4);
        pk[0] = p0.x; pk[1] = p0.y; pk[2] = p0.z; pk[3] = p0.w; pk[4] = p1.x; pk[5] = p1.y; pk[6] = p1.z; pk[7] = p1.w;
    }
#pragma unroll
    for (int i = 0; i < GBM * 16 / THREADS; ++i) {
        const int row = (tid + THREADS * i) >> 4;          // the 16 lanes of a row are consecutive lanes of one wave
        const bool live = row < rows && inside;
        float v[8];
        {
            const float* ep = E + row * BK + (c8 ^ ((row & 1) << 4));
            const f32x4 lo = *(const f32x4*)ep, hi = *(const f32x4*)(ep + 4);
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        }
        if (up) {
            if (live) {
                float* orow = p.dxr + (size_t)(row0 + row) * H;
                if (perm) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) orow[pk[c]] = v[c];
                } else {
                    *(f32x4*)(orow + k) = f32x4{v[0], v[1], v[2], v[3]};
                    *(f32x4*)(orow + k + 4) = f32x4{v[4], v[5], v[6], v[7]};
                }
            }
            continue;
        }
        float part = 0.f;
        if (live) {
            T* grow = (T*)p.g + (size_t)(row0 + row) * I;
            T* urow = (T*)p.u + (size_t)(row0 + row) * I;
            const float wt = p.w[p.row_assign[row0 + row]];
            float gv[8], uv[8], dg[8], du[8];
            if (perm) {
#pragma unroll
                for (int c = 0; c < 8; ++c) gv[c] = elem16<T>(grow + pk[c]), uv[c] = elem16<T>(urow + pk[c]);
            } else {
                unpack8<T>(*(const u32x4*)(grow + k), gv);
                unpack8<T>(*(const u32x4*)(urow + k), uv);
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float den = 1.f + __expf(-gv[c]);
                const float sg = 1.f / den, silu = gv[c] / den;
                // h_r as the forward's epilogue forms and rounds it; the forms of moe_grad_kernel's object code (above)
                if (c < 2) {
                    part = __builtin_fmaf(v[c], h_mix<T>(silu, uv[c]), part);
                } else {
                    part += prod(v[c], DType<T>::to_f32(DType<T>::from_f32(prod(silu, uv[c]))));
                }
                const float wd = wt * v[c];
                dg[c] = prod(wd * uv[c], sg * __builtin_fmaf(gv[c], 1.f - sg, 1.f));
                du[c] = prod(wd, silu);
            }
            if (perm) {
#pragma unroll
                for (int c = 0; c < 8; ++c) grow[pk[c]] = DType<T>::from_f32(dg[c]), urow[pk[c]] = DType<T>::from_f32(du[c]);
            } else {
                const u32x2 g0 = pack4<T>(f32x4{dg[0], dg[1], dg[2], dg[3]}), g1 = pack4<T>(f32x4{dg[4], dg[5], dg[6], dg[7]});
                const u32x2 u0 = pack4<T>(f32x4{du[0], du[1], du[2], du[3]}), u1 = pack4<T>(f32x4{du[4], du[5], du[6], du[7]});
                *(u32x4*)(grow + k) = u32x4{g0.x, g0.y, g1.x, g1.y};
                *(u32x4*)(urow + k) = u32x4{u0.x, u0.y, u1.x, u1.y};
            }
        }
        if (p.dwp) {                                       // (uniform) the row's 128 columns: 8 per lane in ascending order, then a fixed tree over its 16 lanes
            part += __shfl_xor(part, 8);
            part += __shfl_xor(part, 4);
            part += __shfl_xor(part, 2);
            part += __shfl_xor(part, 1);
            if ((tid & 15) == 0 && row < rows) p.dwp[(size_t)(row0 + row) * p.nkt + kt] = part;
        }
    }
}

}  // namespace gcopy
}  // namespace gptq
