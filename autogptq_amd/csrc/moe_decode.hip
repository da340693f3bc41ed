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
// The body of both launches lives in moe_decode_kernel.cuh (moe_decode_body<T, BITS, PAIR, SHARED>): these kernels are its SHARED = false form, and
// moe_shared.hip compiles the SHARED = true form (the shared expert of a Qwen-MoE block in the same two launches) into a kernel of its own.  2- and 3-bit
// experts (GPTQ_MOE_LOW_BIT_DECODE): the same two launches with the same grids, arguments and LDS bytes, on the 2- / 3-bit forms of that kernel.
// No K slices, no atomics: every output is one thread's sum in a fixed order, so results are bit-reproducible and the row of token t does not depend on the
// other tokens of the call.
// Layout read: gptq_layer_t.qweight_tiled / qconst_tiled (include/gptq_mi355x.h): a strip is one contiguous run, a chunk (4 k-slots x 16 columns) one wave
// load, lane (kb, col) holds KPL consecutive k of one column.
#include <string.h>

#include <algorithm>

#include "moe_decode_kernel.cuh"     // the body of both launches, Args, Entry, waves_for, lds_layout: shared with moe_shared.hip

namespace gptq {
namespace moedec {

template <typename T, int BITS, bool PAIR>
__global__ void __launch_bounds__(1024) moe_decode_kernel(Args p) {
    moe_decode_body<T, BITS, PAIR, false>(p, Shared{});
}

template <typename T, int BITS, bool PAIR>
static hipError_t launch_one(const Args& a, dim3 grid, int lds, hipStream_t st) {
    hipLaunchKernelGGL((moe_decode_kernel<T, BITS, PAIR>), grid, dim3(a.waves * 64), lds, st, a);
    return hipGetLastError();
}
template <bool PAIR>
static hipError_t launch_any(int dtype, int bits, const Args& a, dim3 grid, int lds, hipStream_t st) {
    if (bits == 2 || bits == 3) return launch_low_bit_form(PAIR, dtype, bits, a, grid, lds, st);      // (GPTQ_MOE_LOW_BIT_DECODE) forms of moe_shared.hip's kernel, not kernels of this file
    if (dtype == GPTQ_F16) return bits == 4 ? launch_one<f16, 4, PAIR>(a, grid, lds, st) : launch_one<f16, 8, PAIR>(a, grid, lds, st);
    return bits == 4 ? launch_one<bf16, 4, PAIR>(a, grid, lds, st) : launch_one<bf16, 8, PAIR>(a, grid, lds, st);
}

}  // namespace moedec

using moedec::a256;
using moedec::any_perm;

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
        a.E = E; a.topk = topk;
        moedec::fill_geometry(a, L, act, pair, waves);
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
