// adapter_rows.hip -- per-row adapter banks beside a quantized linear (gptq_adapter_route, gptq_adapter_rows_apply): every row of a batch carries the slot
// of ITS adapter, or none.  A bank holds `slots` adapters of one layer: A [slots][r][K], B [slots][N][r] in the layer dtype T, scales [slots] fp32.
//   row m with a = ids[m] in [0, slots):
//     u_m[j]    = T(sum_k x[m, k] * A[a][j, k])                                          fp32 products and sums, one rounding
//     out[m, n] = T(float(out[m, n]) + scales[a] * sum_j float(u_m[j]) * float(B[a][n, j]))   in place on the base output
//   any other id leaves out[m] untouched, bit for bit.
// Three launches, no host round trip (capturable: ids is read on the device only):
//   1. moe_route_kernel (moe.hip; idx = ids, topk = 1, E = slots, bm = 16): rows sorted by slot, pos[m], row_assign[sorted row] -> m and a table of tiles
//      (slot, first sorted row, rows <= 16) with its count.  One routing serves every layer of a model step.
//   2. adapter_rows_down_kernel<T>: a workgroup = one tile x one 16-wide block of A rows of the tile's slot x the whole K; its 8 waves take the 32-wide
//      k-steps round robin and meet once in LDS, summed in wave order (lora.hip's matrix-core regime).  u is [M][r] in SORTED-row order.
//   3. adapter_rows_up_kernel<T>: B rows of the tile's slot are the MFMA's A operand, the tile's u rows its B operand; a lane's four accumulators are four
//      consecutive n of one output row: an 8-byte read-modify-write of out[row_assign[first + row]].  Every out row belongs to at most one tile: no race.
// The grid's x is a bound computed from (M, slots) alone -- M / 16 + min(slots, M) tiles -- and workgroups past the count the routing wrote return at
// once.  Lane rows past the tile repeat its last row (results discarded), so the loops have no branch on the row count.  A row's dot products never mix
// with another row's: its bits depend on x[m], its slot and the bank alone.  Up to GPTQ_LORA_MAX banks that share x and the routing (q|k|v, gate|up) go
// through ONE launch per direction: the pointer sets travel by value and are addressed with constant indices only (as lora::locate does), so they
// stay in scalar registers.  No atomics, no workgroup waits on another, fixed summation order, one instantiation per kernel and dtype (4 in all).
#include <algorithm>

#include "common.cuh"
#include "mma_dequant.cuh"
#include "launch.h"

namespace gptq {
namespace adapters {

constexpr int DOWN_THREADS = 512;           // 8 waves split K
constexpr int DOWN_WAVES = DOWN_THREADS / 64;
constexpr int UP_THREADS = 256;             // 4 waves x 64 columns
constexpr int UP_COLS = 256;
constexpr int TILE_ROWS = GPTQ_ADAPTER_TILE_ROWS;

struct Set {
    const void* A;                          // [slots][r][K]
    const void* B;                          // [slots][N][r]
    const float* scales;                    // [slots]
    void* u;                                // [M][r], sorted-row order
    void* out;                              // [M][N]
    int N, r;
};
struct Args {
    Set s[GPTQ_LORA_MAX];
    const void* x;
    const int* tile_count;
    const int4* tiles;                      // (slot, first sorted row, rows, 0)
    const int* row_assign;                  // sorted row -> m
    int n, K;
};

__host__ __device__ inline int down_units(int r) { return (r + 15) / 16; }
__host__ __device__ inline int up_units(int N) { return (N + UP_COLS - 1) / UP_COLS; }

// the bank that owns unit `b` of the concatenated grid, and b relative to it (constant indices only: the sets stay in scalar registers)
template <bool UP>
__device__ __forceinline__ Set locate(const Args& p, int& b) {
    Set s = p.s[0];
    int start = 0;
    const int g = b;
#pragma unroll
    for (int i = 1; i < GPTQ_LORA_MAX; ++i) {
        start += UP ? up_units(p.s[i - 1].N) : down_units(p.s[i - 1].r);
        if (i < p.n && g >= start) {
            s = p.s[i];
            b = g - start;
        }
    }
    return s;
}

template <typename T>
__global__ void __launch_bounds__(DOWN_THREADS) adapter_rows_down_kernel(Args p) {
    __shared__ float red[DOWN_WAVES * 256];
    if ((int)blockIdx.x >= *p.tile_count) return;
    const int4 tile = p.tiles[blockIdx.x];
    const int slot = tile.x, first = tile.y, rows = tile.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K;
    int b = blockIdx.y;
    const Set s = locate<false>(p, b);
    const T* __restrict__ x = (const T*)p.x;
    const T* __restrict__ A = (const T*)s.A + (size_t)slot * s.r * K;
    T* __restrict__ u = (T*)s.u;

    const int j0 = b * 16;
    const int row = lane & 15, kq = lane >> 4;
    const int m = p.row_assign[first + min(row, rows - 1)];      // rows past the tile repeat its last row
    const bool aok = j0 + row < s.r;
    const char* xp = (const char*)(x + (size_t)m * K) + kq * 16;
    const char* ap = (const char*)(A + (size_t)(aok ? j0 + row : 0) * K) + kq * 16;
    const u32x4 zero = u32x4{0, 0, 0, 0};
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int steps = K / 32;                                   // 64 bytes of a row per step
    for (int st = wave; st < steps; st += 4 * DOWN_WAVES) {
        u32x4 xa[4], aa[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = st + i * DOWN_WAVES;
            const bool in = t < steps;
            xa[i] = in ? *(const u32x4*)(xp + (size_t)t * 64) : zero;
            aa[i] = in && aok ? *(const u32x4*)(ap + (size_t)t * 64) : zero;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = Mma16<T>::run(xa[i], aa[i], acc);
    }
    // accumulator: column (l & 15) is j, rows 4 (l >> 4) + reg are the tile's rows
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) red[wave * 256 + (4 * kq + reg) * 16 + row] = acc[reg];
    __syncthreads();
    if (tid < 256) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < DOWN_WAVES; ++w) v += red[w * 256 + tid];
        const int tr = tid >> 4, j = j0 + (tid & 15);
        if (tr < rows && j < s.r) u[(size_t)(first + tr) * s.r + j] = DType<T>::from_f32(v);
    }
}

template <typename T>
__global__ void __launch_bounds__(UP_THREADS) adapter_rows_up_kernel(Args p) {
    if ((int)blockIdx.x >= *p.tile_count) return;
    const int4 tile = p.tiles[blockIdx.x];
    const int slot = tile.x, first = tile.y, rows = tile.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.y;
    const Set s = locate<true>(p, b);
    const int N = s.N, r = s.r;
    const int n0 = b * UP_COLS + wave * 64;
    if (n0 >= N) return;
    const T* __restrict__ B = (const T*)s.B + (size_t)slot * N * r;
    const T* __restrict__ u = (const T*)s.u;
    T* __restrict__ out = (T*)s.out;
    const float scale = s.scales[slot];                         // uniform over the workgroup: one scalar load

    const int row = lane & 15, kq = lane >> 4;
    const bool mok = row < rows;
    const int sr = first + (mok ? row : rows - 1);
    const int m = p.row_assign[sr];
    const u32x4 zero = u32x4{0, 0, 0, 0};
    const bool two = r > 32;                                    // the second k-step of the matrix core (j = 32..63)
    const int ja = 8 * kq, jb = 32 + 8 * kq;
    const T* up = u + (size_t)sr * r;
    const u32x4 u0 = mok && ja < r ? *(const u32x4*)(up + ja) : zero;
    const u32x4 u1 = mok && jb < r ? *(const u32x4*)(up + jb) : zero;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int nn = n0 + nb * 16;                            // N % 16 == 0: a block is inside or outside as a whole
        const bool nok = nn < N;
        const T* bp = B + (size_t)(nok ? nn + row : 0) * r;
        const u32x4 b0 = nok && ja < r ? *(const u32x4*)(bp + ja) : zero;
        const u32x4 b1 = nok && jb < r ? *(const u32x4*)(bp + jb) : zero;
        f32x4 acc = Mma16<T>::run(b0, u0, f32x4{0.f, 0.f, 0.f, 0.f});
        if (two) acc = Mma16<T>::run(b1, u1, acc);
        // accumulator: column (l & 15) is the tile's row, rows 4 (l >> 4) + reg are four consecutive n
        if (nok && mok) {
            T* o = out + (size_t)m * N + nn + 4 * kq;
            const u32x2 old = *(const u32x2*)o;
            const unsigned ow[2] = {old.x, old.y};
            unsigned short h[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float prev = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(ow[c >> 1] >> (16 * (c & 1)))));
                h[c] = __builtin_bit_cast(unsigned short, DType<T>::from_f32(prev + scale * acc[c]));
            }
            *(u32x2*)o = u32x2{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
        }
    }
}

static Args make_args(const gptq_adapter_bank_t* const* Bs, int n, const void* x, void* const* u, void* const* outs, const AdapterRoutePlan& rp,
                      const char* route) {
    Args p;
    for (int i = 0; i < GPTQ_LORA_MAX; ++i) {
        Set& s = p.s[i];
        if (i < n) {
            s.A = Bs[i]->A;
            s.B = Bs[i]->B;
            s.scales = Bs[i]->scales;
            s.u = u[i];
            s.out = outs[i];
            s.N = Bs[i]->N;
            s.r = Bs[i]->r;
        } else {
            s.A = s.B = nullptr;
            s.scales = nullptr;
            s.u = s.out = nullptr;
            s.N = s.r = 0;
        }
    }
    p.x = x;
    p.tile_count = (const int*)(route + rp.off_tile_count);
    p.tiles = (const int4*)(route + rp.off_tiles);
    p.row_assign = (const int*)(route + rp.off_rows);
    p.n = n;
    p.K = Bs[0]->K;
    return p;
}

}  // namespace adapters

AdapterRoutePlan plan_adapter_route(int M, int slots) {
    AdapterRoutePlan rp;
    rp.tiles = (long)M / adapters::TILE_ROWS + std::min((long)slots, (long)M);
    rp.bytes = append_route_layout(rp, 0, slots, rp.tiles, M);
    return rp;
}

AdapterRowsPlan plan_adapter_rows(const gptq_adapter_bank_t* const* Bs, int n, int M) {
    AdapterRowsPlan pl;
    pl.tiles = plan_adapter_route(M, Bs[0]->slots).tiles;
    long du = 0, uu = 0;
    for (int i = 0; i < n; ++i) {
        du += adapters::down_units(Bs[i]->r);
        uu += adapters::up_units(Bs[i]->N);
    }
    pl.units_down = du;
    pl.units_up = uu;
    pl.wg_down = du * pl.tiles;
    pl.wg_up = uu * pl.tiles;
    return pl;
}

hipError_t launch_adapter_route(const int64_t* ids, int M, int slots, char* route, hipStream_t st) {
    const AdapterRoutePlan rp = plan_adapter_route(M, slots);
    return launch_moe_route(ids, M, 1, slots, adapters::TILE_ROWS, (int*)(route + rp.off_offsets), (int*)(route + rp.off_tile_count), route + rp.off_tiles,
                            (int*)(route + rp.off_pos), (int*)(route + rp.off_rows), st);
}

hipError_t launch_adapter_rows(const gptq_adapter_bank_t* const* Bs, int n, const void* x, void* const* u, void* const* outs, const void* route, int M,
                               hipStream_t st) {
    const AdapterRowsPlan pl = plan_adapter_rows(Bs, n, M);
    if (pl.tiles > 0x7fffffffL || pl.units_down > 65535 || pl.units_up > 65535) return hipErrorInvalidValue;
    const AdapterRoutePlan rp = plan_adapter_route(M, Bs[0]->slots);
    const adapters::Args p = adapters::make_args(Bs, n, x, u, outs, rp, (const char*)route);
    const dim3 gd((unsigned)pl.tiles, (unsigned)pl.units_down), gu((unsigned)pl.tiles, (unsigned)pl.units_up);
    if (Bs[0]->dtype == GPTQ_F16) {
        hipLaunchKernelGGL(adapters::adapter_rows_down_kernel<f16>, gd, dim3(adapters::DOWN_THREADS), 0, st, p);
        hipLaunchKernelGGL(adapters::adapter_rows_up_kernel<f16>, gu, dim3(adapters::UP_THREADS), 0, st, p);
    } else if (Bs[0]->dtype == GPTQ_BF16) {
        hipLaunchKernelGGL(adapters::adapter_rows_down_kernel<bf16>, gd, dim3(adapters::DOWN_THREADS), 0, st, p);
        hipLaunchKernelGGL(adapters::adapter_rows_up_kernel<bf16>, gu, dim3(adapters::UP_THREADS), 0, st, p);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gptq
