// moe_shared.hip -- the shared expert of a Qwen-MoE block next to its routed experts:
//   out[t] = T(sum_j w[t, j] * (h_(t,j) . W2_e)  +  s_t * (hs_t . W2_s)),   hs_t = T(silu(x_t . W1_s) * (x_t . W3_s)),   s_t = sigmoid(T(x_t . w_g))
// (transformers' Qwen2MoeSparseMoeBlock.forward: experts(x, idx, w) + sigmoid(shared_expert_gate(x)) * shared_expert(x)).
//
// 1..4 tokens (gptq_moe_shared_decode_forward): the two launches of moe_decode.hip in their SHARED form (moe_decode_body<T, BITS, PAIR, true>,
// moe_decode_kernel.cuh) -- the shared expert is one more always-on assignment with its own width I_s.
//   1. the pair form   grid (I / 16, T topk + T ceil(I_s / I)): the routed workgroups as they are, then per token ceil(I_s / I)
//      grid rows whose workgroups take the strips (row) (I / 16) + blockIdx.x of I_s (those past I_s / 16 leave at once).  The three shared layers need no
//      device table: their pointers are launch arguments.  The shared workgroup of strip 0 also writes s_t from the raw row it has staged.
//   2. the down form   grid (H / 16, T): after the token's topk routed assignments the workgroup stages hs_t, streams strip s of the
//      shared W2 with all waves and adds s_t * sum to the same register; one rounding.  The workgroup has the larger of the two wave counts (K = I against
//      K = I_s); each segment distributes its chunks over its own count, so the routed part sums exactly as gptq_moe_decode_forward does.
// Any token count (gptq_moe_shared_combine): combine_rows<T>, out[t] = T(float(out[t]) + s_t * float(ys[t])) in place on the routed output,
// one workgroup per token, every wave computes s_t itself (no LDS, no barrier), 16-byte loads and stores.
// No atomics, no K slices; s_t is summed in an order that depends on H alone (shared_gate_scalar), the same in both kernels.
#include <algorithm>

#include "launch.h"
#include "moe_decode_kernel.cuh"

namespace gptq {
namespace moedec {

constexpr int COMBINE_THREADS = 256;

template <typename T>
__device__ __forceinline__ void combine_rows(const void* x, const void* gate_w, const void* ys, void* out, int H) {      // 256 threads: one token
    typedef __attribute__((address_space(1))) const u32x4 gu32x4;
    typedef __attribute__((address_space(1))) u32x4 gu32x4w;
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t row = (size_t)blockIdx.x * H * sizeof(T);
    float s = 1.f;
    if (gate_w) s = shared_gate_scalar<T>((gu32x4*)((const char*)x + row), gate_w, H, lane);      // every wave: the same bits
    gu32x4* const yr = (gu32x4*)((const char*)ys + row);
    gu32x4w* const orow = (gu32x4w*)((char*)out + row);
    for (int pc = tid; pc < (H >> 3); pc += COMBINE_THREADS) {
        const u32x4 ov = orow[pc], yv = yr[pc];
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned wd = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float of = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(ov[i] >> (16 * h))));
                const float yf = DType<T>::to_f32(__builtin_bit_cast(T, (unsigned short)(yv[i] >> (16 * h))));
                wd |= (unsigned)__builtin_bit_cast(unsigned short, DType<T>::from_f32(fmaf(s, yf, of))) << (16 * h);
            }
            r[i] = wd;
        }
        orow[pc] = r;
    }
}

// ONE kernel for everything the shared expert adds: the library's instantiation count is guarded (tests/test_kernel_resources.py) and has room for one, and
// the routed kernels of moe_decode.hip stay the code they were.  `form` is launch-uniform, so a workgroup runs exactly one of the compilations below; the
// kernel's register count is the largest of theirs (the 4-bit down form's), which keeps 16-wave workgroups at 4 waves per SIMD.
//   form 0..7  moe_decode_body<T, BITS, PAIR, true>: 4 (T = bf16) + 2 (BITS = 8) + 1 (PAIR)
//   form 8, 9  the combine tail for fp16 / bf16: x = sp.a, gate_w = sp.gate_w, ys = p.a, out = p.out, H = sp.K
//   form 10..17  the ROUTED experts alone at 3 and 2 bits (gptq_moe_decode_forward with GPTQ_MOE_LOW_BIT_DECODE): moe_decode_body<T, BITS, PAIR, false>,
//              10 + 4 (T = bf16) + 2 (BITS = 2) + 1 (PAIR) -- the SHARED = false compilation reads nothing of sp but form and runs on p.waves.
//              The kernel keeps its 63 VGPRs with them.  Their cases stand in front of the others: of the two orders measured, the one that left forms
//              0..9 closer to their times before (profiles/moe_lowbit_decode_ab.log).
constexpr int FORM_COMBINE = 8, FORM_LOW_BIT = 10;
__global__ void __launch_bounds__(1024) moe_shared_kernel(Args p, Shared sp) {
    switch (sp.form) {
        case FORM_LOW_BIT + 0: moe_decode_body<f16, 3, false, false>(p, sp); break;
        case FORM_LOW_BIT + 1: moe_decode_body<f16, 3, true, false>(p, sp); break;
        case FORM_LOW_BIT + 2: moe_decode_body<f16, 2, false, false>(p, sp); break;
        case FORM_LOW_BIT + 3: moe_decode_body<f16, 2, true, false>(p, sp); break;
        case FORM_LOW_BIT + 4: moe_decode_body<bf16, 3, false, false>(p, sp); break;
        case FORM_LOW_BIT + 5: moe_decode_body<bf16, 3, true, false>(p, sp); break;
        case FORM_LOW_BIT + 6: moe_decode_body<bf16, 2, false, false>(p, sp); break;
        case FORM_LOW_BIT + 7: moe_decode_body<bf16, 2, true, false>(p, sp); break;
        case 0: moe_decode_body<f16, 4, false, true>(p, sp); break;
        case 1: moe_decode_body<f16, 4, true, true>(p, sp); break;
        case 2: moe_decode_body<f16, 8, false, true>(p, sp); break;
        case 3: moe_decode_body<f16, 8, true, true>(p, sp); break;
        case 4: moe_decode_body<bf16, 4, false, true>(p, sp); break;
        case 5: moe_decode_body<bf16, 4, true, true>(p, sp); break;
        case 6: moe_decode_body<bf16, 8, false, true>(p, sp); break;
        case 7: moe_decode_body<bf16, 8, true, true>(p, sp); break;
        case FORM_COMBINE: combine_rows<f16>(sp.a, sp.gate_w, p.a, p.out, sp.K); break;
        default: combine_rows<bf16>(sp.a, sp.gate_w, p.a, p.out, sp.K); break;
    }
}

static hipError_t launch_form(bool pair, int dtype, int bits, const Args& a, Shared s, dim3 grid, int lds, hipStream_t st) {
    s.form = (dtype == GPTQ_BF16 ? 4 : 0) + (bits == 8 ? 2 : 0) + (pair ? 1 : 0);
    hipLaunchKernelGGL(moe_shared_kernel, grid, dim3(s.block_waves * 64), lds, st, a, s);
    return hipGetLastError();
}

hipError_t launch_low_bit_form(bool pair, int dtype, int bits, const Args& a, dim3 grid, int lds, hipStream_t st) {
    if ((bits != 2 && bits != 3) || (dtype != GPTQ_F16 && dtype != GPTQ_BF16)) return hipErrorInvalidValue;
    Shared s{};
    s.form = FORM_LOW_BIT + (dtype == GPTQ_BF16 ? 4 : 0) + (bits == 2 ? 2 : 0) + (pair ? 1 : 0);
    hipLaunchKernelGGL(moe_shared_kernel, grid, dim3(a.waves * 64), lds, st, a, s);
    return hipGetLastError();
}

static Entry entry_of(const gptq_layer_t& L) {
    Entry e;
    moe_decode_table_entry(L, &e);
    return e;
}

}  // namespace moedec

using moedec::a256;
using moedec::any_perm;
static int groups_of(const gptq_layer_t& L) { return (L.K + L.group_size - 1) / L.group_size; }

// The two LDS layouts of one launch (routed segment, shared segment): the cross-wave slab lies behind both.
struct SharedLds { moedec::Lds r, s; int off_red, bytes; };
static SharedLds shared_lds(const gptq_layer_t& R, bool act_r, int waves_r, const gptq_layer_t& S, bool act_s, int waves_s, bool pair, int block_waves) {
    SharedLds l;
    l.r = moedec::lds_layout(R.K, groups_of(R), R.bits, act_r, pair, waves_r);
    l.s = moedec::lds_layout(S.K, groups_of(S), S.bits, act_s, pair, waves_s);
    l.off_red = std::max(l.r.bytes - waves_r * moedec::ES * 4, l.s.bytes - waves_s * moedec::ES * 4);
    l.bytes = l.off_red + block_waves * moedec::ES * 4;
    return l;
}

MoeSharedPlan plan_moe_shared_decode(const gptq_moe_t& m, const gptq_moe_shared_t& sh, int T, int topk) {
    MoeSharedPlan pl{};
    const MoeDecodePlan base = plan_moe_decode(m, T, topk);
    const gptq_layer_t& G = *m.gate[0];
    const gptq_layer_t& D = *m.down[0];
    const int H = G.K, I = G.N, Is = sh.gate->N;
    pl.act_pair_r = any_perm(m.gate, m.E) || any_perm(m.up, m.E);
    pl.act_down_r = any_perm(m.down, m.E);
    pl.act_pair_s = (sh.gate->qweight_seq && sh.gate->perm) || (sh.up->qweight_seq && sh.up->perm);
    pl.act_down_s = sh.down->qweight_seq && sh.down->perm;
    pl.waves_pair = base.waves_pair;                                    // K = H and the bits are the routed ones: the same count
    pl.waves_down_r = base.waves_down;
    pl.waves_down_s = moedec::waves_for(Is, sh.down->bits, false);
    pl.waves_down = std::max(pl.waves_down_r, pl.waves_down_s);
    const SharedLds lp = shared_lds(G, pl.act_pair_r, pl.waves_pair, *sh.gate, pl.act_pair_s, pl.waves_pair, true, pl.waves_pair);
    const SharedLds ld = shared_lds(D, pl.act_down_r, pl.waves_down_r, *sh.down, pl.act_down_s, pl.waves_down_s, false, pl.waves_down);
    pl.lds_pair = lp.bytes;
    pl.lds_down = ld.bytes;
    pl.ok = base.ok && pl.lds_pair <= moedec::MAX_LDS && pl.lds_down <= moedec::MAX_LDS;
    pl.per_tok = (Is + I - 1) / I;
    pl.wg_pair = T * topk * (I / 16) + T * (Is / 16);
    pl.wg_down = T * (H / 16);
    pl.off_h = base.off_h;
    pl.off_pos = base.off_pos;
    size_t o = base.bytes;
    pl.off_hs = o; o += a256((size_t)T * Is * dtype_size(G.dtype));
    pl.off_s = o; o += a256(4 * (size_t)T);
    pl.bytes = o;
    return pl;
}

hipError_t launch_moe_shared_decode(const gptq_moe_t& m, const gptq_moe_shared_t& sh, const void* table, const MoeSharedPlan& pl, const void* x,
                                    const int64_t* idx, const float* w, int T, int topk, void* out, char* ws, hipStream_t st) {
    const gptq_layer_t& G = *m.gate[0];
    const gptq_layer_t& D = *m.down[0];
    const int E = m.E, H = G.K, I = G.N, Is = sh.gate->N;
    const SharedLds lp = shared_lds(G, pl.act_pair_r, pl.waves_pair, *sh.gate, pl.act_pair_s, pl.waves_pair, true, pl.waves_pair);
    const SharedLds ld = shared_lds(D, pl.act_down_r, pl.waves_down_r, *sh.down, pl.act_down_s, pl.waves_down_s, false, pl.waves_down);
    moedec::Args g{};
    g.table = (const moedec::Entry*)table;
    g.idx = (const long long*)idx; g.w = w; g.a = x; g.out = ws + pl.off_h; g.pos = (int*)(ws + pl.off_pos);
    g.E = E; g.topk = topk;
    moedec::fill_geometry(g, G, pl.act_pair_r, true, pl.waves_pair);
    moedec::Shared sg{};
    sg.e0 = moedec::entry_of(*sh.gate);
    sg.e1 = moedec::entry_of(*sh.up);
    sg.gate_w = sh.gate_w;
    sg.s = (float*)(ws + pl.off_s);
    sg.a = x;
    sg.out = ws + pl.off_hs;
    sg.rows = T * topk; sg.per_tok = pl.per_tok; sg.strips = Is / 16;
    moedec::fill_geometry(sg, *sh.gate, pl.act_pair_s, true, pl.waves_pair);
    sg.block_waves = pl.waves_pair;
    sg.off_red = lp.off_red;
    hipError_t e = moedec::launch_form(true, G.dtype, G.bits, g, sg, dim3(I / 16, T * topk + T * pl.per_tok), pl.lds_pair, st);
    if (e != hipSuccess) return e;
    moedec::Args d{};
    d.table = (const moedec::Entry*)table + 2 * (size_t)E;
    d.idx = g.idx; d.w = w; d.a = ws + pl.off_h; d.out = out; d.pos = nullptr;
    d.E = E; d.topk = topk;
    moedec::fill_geometry(d, D, pl.act_down_r, false, pl.waves_down_r);
    moedec::Shared sd{};
    sd.e0 = moedec::entry_of(*sh.down);
    sd.e1 = sd.e0;
    sd.s = sg.s;
    sd.a = ws + pl.off_hs;
    moedec::fill_geometry(sd, *sh.down, pl.act_down_s, false, pl.waves_down_s);
    sd.block_waves = pl.waves_down;
    sd.off_red = ld.off_red;
    return moedec::launch_form(false, D.dtype, D.bits, d, sd, dim3(H / 16, T), pl.lds_down, st);
}

hipError_t launch_moe_shared_combine(const void* x, const void* gate_w, const void* ys, void* out, int T, int H, int dtype, hipStream_t st) {
    if (dtype != GPTQ_F16 && dtype != GPTQ_BF16) return hipErrorInvalidValue;
    moedec::Args a{};
    moedec::Shared s{};
    a.a = ys; a.out = out;
    s.a = x; s.gate_w = gate_w; s.K = H;
    s.form = moedec::FORM_COMBINE + (dtype == GPTQ_BF16 ? 1 : 0);
    hipLaunchKernelGGL(moedec::moe_shared_kernel, dim3((unsigned)T), dim3(moedec::COMBINE_THREADS), 0, st, a, s);
    return hipGetLastError();
}

// grants > 64 KiB of dynamic LDS, as init_moe_decode_device does for the routed kernels
hipError_t init_moe_shared_device() {
    return hipFuncSetAttribute((const void*)moedec::moe_shared_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, moedec::MAX_LDS);
}

}  // namespace gptq
