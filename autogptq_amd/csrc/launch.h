// launch.h -- host-side declarations shared between the kernel translation units and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/gptq_mi355x.h"

namespace gptq {

// The strip width of the layer's decode copy (0: none) -- tiled_cols without the opt-in flag it may carry; every comparison with GPTQ_STRIP_COLS goes through here.
inline int copy_cols(const gptq_layer_t& L) { return GPTQ_COPY_COLS(L.tiled_cols); }
// ... and the opt-in itself: a 2-bit layer that carries its copy and GPTQ_COPY_ROWS_INT2 (on any other layer the flag means nothing)
inline bool copy_rows_int2(const gptq_layer_t& L) {
    return L.bits == 2 && (L.tiled_cols & GPTQ_COPY_ROWS_INT2) != 0 && copy_cols(L) == GPTQ_STRIP_COLS && L.qweight_tiled != nullptr && L.qconst_tiled != nullptr;
}
// ... with GPTQ_COPY_ROWS_INT2_WIDE: the whole band of the 4-bit twin (a layer whose checkpoint rows are not resident)
inline bool copy_rows_int2_wide(const gptq_layer_t& L) { return copy_rows_int2(L) && (L.tiled_cols & GPTQ_COPY_ROWS_INT2_WIDE) != 0; }

struct GemvPlan {
    int ln, waves, ksplit, strips, mt, mtiles;
    int units_total, units_per_split, chunk_units;
    bool perk, use_seq;
    bool mfma;     // 4-bit fp16 / bf16 register kernel with the k-reduction on v_mfma_f32_4x4x4_16b_f16
    bool mfmag;    // matrix-core kernel for the other packings / bf16 (gemv_mfma_generic_kernel)
    bool magic;    // ... with the packed magic-number field decode (3- / 8-bit fp16)
    bool pair;     // mfma path with the fused SILU_MUL epilogue (gate/up halves walked by the same workgroup)
    bool xperm;    // act-order, 2+ rows of x: x is permuted once by a pre-pass into the workspace front (xperm_bytes) and the plain kernel streams qweight_seq
    size_t xperm_bytes;
    int u;         // direct path: consecutive packed rows per lane and iteration
    size_t lds_bytes, workspace_bytes;
};
GemvPlan plan_gemv(const gptq_layer_t& L, int M, const gptq_tuning_t* tune);
hipError_t launch_gemv(const gptq_layer_t& L, const GemvPlan& pl, const void* x, void* out, int M,
                       void* workspace, hipStream_t st);

// 17 .. 128 rows (gemm_mid.hip: gemm_mid_kernel): 1..4 plain 4-bit layers that read the same x, one launch; weights, x and group constants by LDS DMA.
struct MidPlan {
    bool ok;                 // every layer qualifies and the geometry fits
    bool pays;               // measured preference over the other kernels
    bool xreg;               // experiment: x through registers (ordinary loads + ds_write) instead of LDS DMA
    bool gran;               // K slices combined through tag-validated {fp32, tag} granules (one hop) instead of partial tiles + flags
    int cw;                  // 64-column halves per strip (2: 128-column strips, M <= 64)
    int row_blocks;          // workgroups along M (each owns 16 rt rows of x)
    int bits;                // 4 or 8
    int nseg, rt, waves, stages, ksplit, ksteps_total, ksteps_per_split, strips_total, nsum, lg_gsteps, tab_bytes;
    size_t lds_bytes;
    size_t partial_bytes;    // behind the header (and the permuted x of an act-order layer): [ksplit - 1][M][nsum] fp32 when ksplit > 1
};
MidPlan plan_mid(const gptq_layer_t* const* layers, int n, int M, const gptq_tuning_t* tune);
// qweight_override: the re-sequenced rows of a single act-order layer (x is then the permuted copy), else NULL
hipError_t launch_mid(const gptq_layer_t* const* layers, const MidPlan& pl, const void* x, void* const* outs, int M, void* ws_header, void* partial,
                      const uint32_t* qweight_override, hipStream_t st);
hipError_t init_gemm_mid_device();

// gemm_wide_sk.hip: the same wave tile as a stream-K partition (one persistent workgroup per CU; 128 x 256 tiles, two K parts per workgroup) for launches
// that do not divide into whole rounds of 128 x 512 tiles; weights from the decode copy only
struct WideSkGeom {
    int nbm, nbn, upt, units_total, lg_nwg;
    size_t slot_bytes;        // published accumulators of cut tiles: 256 KiB per workgroup (0 when every range boundary is a tile boundary)
};

// gemm_rows.hip: 5 .. ~256 rows from the decode copy, a workgroup = 16 rb rows x s strips x the whole K, no exchange between workgroups
struct RowsPlan {
    bool ok;
    int rb, s, xbufs, waves, cpw, npm, nsg;
    size_t lds_bytes;
};
bool rows_ok(const gptq_layer_t& L, int M);
bool rows_pays(const gptq_layer_t& L, int M);
RowsPlan plan_rows(const gptq_layer_t& L, int M, const gptq_tuning_t* tune);
hipError_t launch_gemm_rows(const gptq_layer_t& L, const RowsPlan& pl, const void* x, void* out, int M, hipStream_t st);
bool rows_multi_ok(const gptq_layer_t* const* Ls, int n, int M);      // 1 .. 4 layers that read the same x in ONE launch (gptq_forward_multi)
bool rows_multi_pays(const gptq_layer_t* const* Ls, int n, int M);
RowsPlan plan_rows_multi(const gptq_layer_t* const* Ls, int n, int M, const gptq_tuning_t* tune);
hipError_t launch_gemm_rows_multi(const gptq_layer_t* const* Ls, int n, const RowsPlan& pl, const void* x, void* const* outs, int M, hipStream_t st);
hipError_t init_gemm_rows_device();

// gemm_panel.hip: 129 .. ~767 rows from the decode copy, a workgroup = 32 mt rows x 32 nt columns x the whole K (kp waves = K parts), no exchange between workgroups
struct PanelPlan {
    bool ok;
    int mt, nt, kp, nbm, nbn, spw;
    size_t lds_bytes;
};
bool panel_ok(const gptq_layer_t& L, int M);
bool panel_pays(const gptq_layer_t& L, int M);
bool panel_pays_filled(const gptq_layer_t& L, int M);
PanelPlan plan_panel(const gptq_layer_t& L, int M, const gptq_tuning_t* tune);
hipError_t launch_gemm_panel(const gptq_layer_t& L, const PanelPlan& pl, const void* x, void* out, int M, hipStream_t st);
hipError_t init_gemm_panel_device();

// Batched decode (gemm_stream64_kernel): 1..4 plain 4-bit layers that read the same x, 1 <= M <= 64, one launch.
struct Stream64Plan {
    bool ok;                 // every layer qualifies and the geometry fits
    bool pays;               // measured preference over the per-layer kernels (enough workgroups, not a small layer)
    int nseg, mt, waves, u, ksplit, ksteps_total, ksteps_per_split, strips_total, nsum;
    size_t lds_bytes;
    size_t partial_bytes;    // behind the header (and the permuted x of an act-order layer): [ksplit][M][nsum] fp32 when ksplit > 1
};
// The ONE kernel a GemmPlan launches; gemm_kernel_names[] is what gptq_describe_plan prints (GEMM_WIDE reading the decode copy -- wide_tiled -- prints "wide_copy")
enum GemmKernel {
    GEMM_TILED,               // 128 / 64 / 32 x 256 tiles of gemm_kernel (gemm.hip): everything no other kernel takes
    GEMM_F32,                 // fp32 I/O: exact-f32 matrix core kernel (128 x 128 tiles)
    GEMM_PANEL,               // gemm_panel.hip (panelp holds its geometry); act-order layers: x permuted in natural order (xnat)
    GEMM_ROWS,                // gemm_rows.hip (rowsp holds its geometry); act-order layers: x permuted in natural order (xnat)
    GEMM_WIDE_SK,             // stream-K partition of 128 x 256 tiles with the 128 x 128 wave tile (gemm_wide_sk.hip; wskg); implies wide_tiled (+ xnat for act-order layers)
    GEMM_WIDE,                // 128 x 512 tiles, 128 x 128 per wave, accumulators in AGPRs (gemm_wide.hip): large launches
    GEMM_MID,                 // 17 .. 128 rows, 4-bit: gemm_mid_kernel (midp holds its geometry)
    GEMM_STREAM64,            // batched decode 4 < M <= 64, 4-bit: 64-column strips by LDS DMA, in-launch K-split combine (s64p holds its geometry; u = K-steps in flight per wave)
    GEMM_STRIP16,             // 8 < M <= 64, 4-bit: 16-column strips on v_mfma_f32_16x16x32 (mt = row tiles of 16)
    GEMM_SKINNY,              // weight-streaming decomposition for 8 < M <= 128 (64-column strips, waves split K)
};
constexpr const char* gemm_kernel_names[] = {"tiled", "f32_mfma", "panel", "rows", "wide_sk", "wide", "mid", "stream64", "strip16", "skinny64"};
struct GemmPlan {
    bool supported, use_seq;
    GemmKernel kernel;
    PanelPlan panelp; RowsPlan rowsp; WideSkGeom wskg; MidPlan midp; Stream64Plan s64p;      // the geometry of `kernel`, where it has a plan of its own
    bool lowbit;              // GEMM_ROWS / GEMM_PANEL on a flagged 2-bit layer: the dense form of moe_rows_lowbit_kernel / moe_panel_lowbit_kernel (rowsp / panelp: its geometry)
    bool wide_tiled;          // GEMM_WIDE / GEMM_WIDE_SK reading the layer's decode copy, raw x staged by LDS DMA
    bool xnat;                // act-order + wide_tiled: x permuted in natural order (the copy is of the re-sequenced rows)
    bool glds;                // ... and stages it with global_load_lds (DMA) into swizzled, unpadded LDS rows
    bool xslot;               // act-order: the x pre-pass writes k-slot order, the kernel copies x to LDS verbatim
    int waves, variant, u;
    int kg;                   // K groups inside a workgroup (2 = 8 waves, two K halves summed through LDS)
    int mt, bk, bm, bn;       // row tiles per wave, K-step, workgroup tile
    int nbm, nbn, ksplit, ksteps_total, ksteps_per_split;
    int tail, tail_lg;        // tiled kernel, balanced tail: the last `tail` tiles run as 2^tail_lg K slices (one workgroup each, combined inside the launch)
    size_t xperm_bytes;       // permuted-x scratch for act-order layers (front of the workspace)
    size_t workspace_bytes;   // xperm + split-K partial slabs (or the balanced tail's accumulator slabs)
};
GemmPlan plan_gemm(const gptq_layer_t& L, int M, const gptq_tuning_t* tune);
hipError_t launch_gemm(const gptq_layer_t& L, const GemmPlan& pl, const void* x, void* out, int M,
                       void* ws_header, void* workspace, hipStream_t st, bool x_permuted = false);

// Streamed GEMV (gemv_q4_stream_kernel): 1..4 plain 4-bit layers that read the same x, one launch.
constexpr size_t WS_HEADER_BYTES = 65536;      // front of every workspace: arrival tickets of the in-launch K-split combine (kept zero)
constexpr size_t WS_HEADER_EPOCH_OFFSET = 32768; // second half of the header: per-strip launch epochs of the streamed GEMV's one-hop K-split combine (monotonic, never reset)
constexpr size_t WS_HEADER_TAIL_BYTES = 64;    // ... except its last 64 bytes: launch epoch / arrival count / sticky error word of the fused MLP exchange (mlp.hip)
struct StreamPlan {
    bool ok;                 // every layer qualifies and the geometry fits
    int nseg, ln, waves, u, mt, ksplit, units_total, units_per_split, strips_total, nsum;
    size_t lds_bytes;
    size_t partial_bytes;    // behind the header: [ksplit][M][nsum] fp32 when ksplit > 1
};
StreamPlan plan_stream(const gptq_layer_t* const* layers, int n, int M, const gptq_tuning_t* tune);
hipError_t launch_stream(const gptq_layer_t* const* layers, const StreamPlan& pl, const void* x, void* const* outs, int M,
                         void* ws_header, void* ws_body, hipStream_t st);
Stream64Plan plan_stream64(const gptq_layer_t* const* layers, int n, int M, const gptq_tuning_t* tune);
// qweight_override: the re-sequenced rows of a single act-order layer (x is then the permuted copy), else NULL
hipError_t launch_stream64(const gptq_layer_t* const* layers, const Stream64Plan& pl, const void* x, void* const* outs, int M,
                           void* ws_header, void* partial, const uint32_t* qweight_override, hipStream_t st);
// Decode from the load-time decode copy (gemv_tiled.hip: gemv_tiled_kernel): 1..4 plain 3/4/8-bit layers with qweight_tiled / qconst_tiled that read the same x, M <= 4, one launch.
struct TiledPlan {
    bool ok;                 // every layer qualifies and the geometry fits
    int nstr;                // strips per workgroup (1; 2 / 4: gemv_tiled_multi.hip -- adjacent strips of a layer behind one staged x)
    bool pair;               // one [gate | up] layer with the SILU_MUL epilogue: a workgroup per pair of strips, SiLU * mul behind the cross-wave sum
    int nseg, bits, waves, u, mt, ksplit, chunks_total, chunks_per_split, strips_total, nsum, groups, xstride, xraw_off;
    size_t lds_bytes;
    size_t partial_bytes;    // behind the header: [ksplit - 1][M][nsum] granules when ksplit > 1
    bool zm2;                // bf16 4-bit layers at 2 rows, launches below 1024 workgroups: the zero-point on the matrix core (gemv_tiled_kernel<..., FL bit 0>)
    bool aligned;            // 4-bit layers whose K is a whole number of chunks, in the forms that have an aligned twin: the K loop with scalar per-chunk addressing (FL bit 1)
    int xsteps;              // 1 or 2: plain 4-bit fp16 launches without K slices that are deeper than one pass of their workgroup stage x and the constants in two steps
};
bool tiled_layer_ok(const gptq_layer_t& L);
TiledPlan plan_tiled(const gptq_layer_t* const* layers, int n, int M, const gptq_tuning_t* tune);
hipError_t launch_tiled(const gptq_layer_t* const* layers, const TiledPlan& pl, const void* x, void* const* outs, int M, void* ws_header, void* ws_body,
                        hipStream_t st, const gptq_peer_group_t* pg = nullptr);      // pg: tensor-parallel epilogue (outs[0] may be null then)
hipError_t init_gemv_tiled_device();
// the decode copy of a 3/4/8-bit layer (utils.hip): qweight_tiled (chunks of 4 k-slots x 16 columns, column per lane, fields in pair order) and qconst_tiled
size_t tiled_weight_bytes(const gptq_layer_t& L);
size_t tiled_const_bytes(const gptq_layer_t& L);
hipError_t launch_prepack_decode(const uint32_t* qweight, const uint32_t* qzeros, const void* scales, int K, int N, int bits, int group_size, int zero_mode,
                                 uint32_t* tiled_out, void* const_out, hipStream_t st);
hipError_t launch_unprepack_decode(const uint32_t* tiled, int K, int N, int bits, uint32_t* qweight_out, hipStream_t st);      // the exact inverse (weights)
bool stream_preferred(const gptq_layer_t& L, int M);                              // single layer: streamed kernel instead of the register one?
bool multi_preferred(const gptq_layer_t* const* layers, int n, int M);             // several layers sharing x: one streamed launch?
hipError_t launch_silu_mul2(const void* g, const void* u, void* out, size_t total, int dtype, int act, hipStream_t st);
bool silu_mul2_permute_ok(int K, int dtype);            // mlp.hip: SiLU * mul and the x permute of an act-order down projection in one pass
hipError_t launch_silu_mul2_permute(const void* g, const void* u, const int32_t* perm, int M, int K, int dtype, int act, void* out, hipStream_t st);
hipError_t init_mlp_device();
// gemm_wide.hip: 128 x 512 prefill tiles, 128 x 128 per wave with the accumulators in AGPRs (4-bit fp16 / bf16; glds: x in k-slot order, staged by LDS DMA)
bool wide_gemm_ok(const gptq_layer_t& L, int M, bool use_seq, bool xslot_glds);
hipError_t launch_gemm_wide(const gptq_layer_t& L, const uint32_t* qweight, const void* x, void* out, int M, bool glds, hipStream_t st, bool tiled = false);
bool wide_sk_ok(const gptq_layer_t& L, int M);
bool wide_sk_pays(const gptq_layer_t& L, int M);      // the planner's measured preference over the whole-tile kernels
WideSkGeom wide_sk_geom(const gptq_layer_t& L, int M);
hipError_t launch_gemm_wide_sk(const gptq_layer_t& L, const void* x, void* out, int M, void* ws_header, void* slots, hipStream_t st);
hipError_t init_gemm_wide_sk_device();
hipError_t init_gemv_device();
hipError_t init_gemm_device();

hipError_t launch_dequant(const gptq_layer_t& L, void* W_out, hipStream_t st);
// grad_input.hip: dX (+)= dY . W^T on the packed rows (L.qweight, L.g_idx); BM x 128 output tiles (grad_input_bm: BM = 128 or 64)
int grad_input_bm(const gptq_layer_t& L, int M);
hipError_t launch_grad_input(const gptq_layer_t& L, const void* dy, void* dx, int M, int accumulate, hipStream_t st);

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }      // the rounding of every workspace segment
inline bool any_perm_of(const gptq_layer_t* const* Ls, int E) {
    for (int e = 0; e < E; ++e)
        if (Ls[e]->perm) return true;
    return false;
}
// The routing block moe_route_kernel fills, as every plan that launches it lays it out: offsets [E + 1], the tile count, tiles (int4 each), pos [R], row_assign [R].
struct RouteLayout {
    size_t off_offsets, off_tile_count, off_tiles, off_pos, off_rows;
};
inline size_t append_route_layout(RouteLayout& rl, size_t o, size_t E, size_t tiles, size_t R) {      // returns the offset behind the block
    rl.off_offsets = o; o += align256(4 * (E + 1));
    rl.off_tile_count = o; o += 256;
    rl.off_tiles = o; o += align256(16 * tiles);
    rl.off_pos = o; o += align256(4 * R);
    rl.off_rows = o; o += align256(4 * R);
    return o;
}
// moe.hip: routed mixture-of-experts layers (gptq_moe_forward): routing table, grouped W1 / W3 + silu * mul, grouped W2, combine -- four launches
struct MoePlan : RouteLayout {
    int bm, bn, tiles, ksplit, steps_per_split;     // tile height, column block, tile bound, K slices of the down projection and their 32-deep steps
    size_t off_h, off_y, bytes;                     // workspace layout behind the routing block (from GPTQ_WORKSPACE_HEADER_BYTES on)
};
MoePlan plan_moe(int E, int T, int topk, int H, int I, int dtype);
size_t moe_table_entry_bytes();
void moe_table_entry(const gptq_layer_t& L, void* dst);
hipError_t launch_moe(const gptq_moe_t& m, const void* table, const MoePlan& pl, const void* x, const int64_t* idx, const float* w, int T, int topk,
                      void* out, char* ws, hipStream_t st);
// host-side launches of moe_route_kernel / moe_combine_kernel (tiles: int4 (expert, first row, rows, 0) per tile)
hipError_t launch_moe_route(const int64_t* idx, int T, int topk, int E, int bm, int* offsets, int* tile_count, void* tiles, int* pos, int* row_assign,
                            hipStream_t st);
hipError_t launch_moe_combine(const int* pos, const float* w, const float* y, void* out, int T, int topk, int H, int ksplit, int rstride, int dtype,
                              hipStream_t st);
// ... and of the pair-mode grouped GEMM with the recompute epilogue (g -> G_sorted, u -> U_sorted [R][I] in T, no silu * mul): moe_grad.hip's second launch
hipError_t launch_moe_recompute(const gptq_moe_t& m, const void* table, const void* x, const int* row_assign, const int* tile_count, const void* tiles,
                                int tiles_bound, int T, int topk, void* g_out, void* u_out, hipStream_t st);
// moe_grad.hip: the backward of the routed layer (gptq_moe_backward): route, recompute g / u, down stage, up stage, combine -- five launches
struct MoeGradPlan : RouteLayout {
    int tiles, nblk_i, nblk_h;                      // tile bound (64-row tiles), 128-column blocks of I and of H
    size_t off_g, off_u, off_dwp, off_dxr, bytes;   // workspace layout behind the routing block (from GPTQ_WORKSPACE_HEADER_BYTES on)
};
MoeGradPlan plan_moe_grad(int E, int T, int topk, int H, int I, int dtype);
size_t moe_grad_table_entry_bytes();
void moe_grad_table_entry(const gptq_layer_t& L, void* dst);
hipError_t launch_moe_grad(const gptq_moe_t& m, const void* table, const void* grad_table, const MoeGradPlan& pl, const void* x, const int64_t* idx,
                           const float* w, const void* dout, int T, int topk, void* dx, float* dw, char* ws, hipStream_t st);
// moe_decode.hip: the same layer at 1..4 tokens on the experts' decode copy (gptq_moe_decode_forward): gate|up + silu * mul, down + combine -- two launches
struct MoeDecodePlan {
    bool ok;                                        // the staged rows and constants fit the LDS
    int wg_pair, wg_down, waves_pair, waves_down, lds_pair, lds_down;
    size_t off_h, off_pos, bytes;                   // workspace layout (from GPTQ_WORKSPACE_HEADER_BYTES on)
};
MoeDecodePlan plan_moe_decode(const gptq_moe_t& m, int T, int topk);
size_t moe_decode_table_entry_bytes();
void moe_decode_table_entry(const gptq_layer_t& L, void* dst);
hipError_t launch_moe_decode(const gptq_moe_t& m, const void* table, const MoeDecodePlan& pl, const void* x, const int64_t* idx, const float* w, int T, int topk,
                             void* out, char* ws, hipStream_t st);
hipError_t init_moe_decode_device();
// moe_shared.hip: the shared expert of a Qwen-MoE block -- the two decode launches in their shared form (gptq_moe_shared_decode_forward, 1..4 tokens), and
// the any-T tail out += sigmoid(x . w_g) * ys in one launch (gptq_moe_shared_combine)
struct MoeSharedPlan {
    bool ok;                                        // both launches' staged rows and constants fit the LDS
    bool act_pair_r, act_down_r, act_pair_s, act_down_s;      // act-order among the routed / the shared layers of either launch
    int wg_pair, wg_down, waves_pair, waves_down, lds_pair, lds_down;      // workgroups that do work, waves per workgroup, dynamic LDS
    int waves_down_r, waves_down_s, per_tok;        // the wave counts the routed / the shared down segment distributes its chunks over; grid rows per token for I_s
    size_t off_h, off_pos, off_hs, off_s, bytes;    // workspace layout (from GPTQ_WORKSPACE_HEADER_BYTES on): the decode path's, then hs [T, I_s] and s [T] fp32
};
MoeSharedPlan plan_moe_shared_decode(const gptq_moe_t& m, const gptq_moe_shared_t& sh, int T, int topk);
hipError_t launch_moe_shared_decode(const gptq_moe_t& m, const gptq_moe_shared_t& sh, const void* table, const MoeSharedPlan& pl, const void* x,
                                    const int64_t* idx, const float* w, int T, int topk, void* out, char* ws, hipStream_t st);
hipError_t launch_moe_shared_combine(const void* x, const void* gate_w, const void* ys, void* out, int T, int H, int dtype, hipStream_t st);
hipError_t init_moe_shared_device();
// moe_rows.hip: the same layer at 5..64 tokens on the experts' decode copy (gptq_moe_batch_forward): route, gate|up + silu * mul, down, combine -- four
// launches (act-order experts: + one row gather through perm in front of either GEMM)
struct MoeBatchPlan : RouteLayout {
    bool act_pair, act_down;                        // some gate / up (down) expert is act-order: the gather pre-pass runs
    int bm, s, tiles, launches;                     // tile height, strip-chunks per wave and chunk, tile bound
    int waves_pair, waves_down, cpw_pair, cpw_down, lds_pair, lds_down;
    size_t off_h, off_y, off_xg, off_hg, bytes;     // workspace layout behind the routing block (from GPTQ_WORKSPACE_HEADER_BYTES on)
};
bool moe_batch_group_ok(const gptq_layer_t& L);    // a group size the rows family takes
MoeBatchPlan plan_moe_batch(const gptq_moe_t& m, int T, int topk);
hipError_t launch_moe_batch(const gptq_moe_t& m, const void* table, const MoeBatchPlan& pl, const void* x, const int64_t* idx, const float* w, int T, int topk,
                            void* out, char* ws, hipStream_t st);
hipError_t init_moe_batch_device();
// ... and the DENSE form of moe_rows_lowbit_kernel<T, 2> (opt-in: copy_rows_int2): one 2-bit QuantLinear layer on its decode copy, out = T(x W + bias), a workgroup
// = 16 rows x 4 strips x the whole K.  x: the rows as the copy wants them (act-order layers: permuted in natural order by the caller).  RowsPlan: rb = 1, s = 4.
bool dense_rows_int2_ok(const gptq_layer_t& L, int M);
RowsPlan plan_dense_rows_int2(const gptq_layer_t& L, int M);
hipError_t launch_dense_rows_int2(const gptq_layer_t& L, const void* x, void* out, int M, const RowsPlan& pl, hipStream_t st);
// 0: the unflagged plan; GEMM_ROWS / GEMM_PANEL: what the planner, left to itself, gives a flagged 2-bit layer at M rows (gemm.hip; the rule of the 4-bit twin)
int dense_int2_choice(const gptq_layer_t& L, int M);
// ... and its row gather (moe_gather_rows_kernel) for the prefill path: out[plane][r] = in[src(r)] through the perm of expert e(r)'s entry of projection
// `plane` of `table` (entries without a perm: a copy); src(r) = row_assign[r] / topk (topk > 0) or r (topk = 0).  R <= 65535 (a grid dimension).
hipError_t launch_moe_gather_rows(const void* table, int planes, int topk, const int64_t* idx, const int* row_assign, const int* offsets, const void* in,
                                  void* out, int E, int K, int R, hipStream_t st);
// moe_panel.hip: the same layer at any token count on the experts' decode copy (gptq_moe_prefill_forward; Python: 65 tokens and more): route with 64-row
// tiles, x into sorted order, gate|up + silu * mul, down, combine -- five launches (act-order down projections: + the gather of H_sorted through perm).
// 4 and 8 bits: moe_panel_kernel; 2 and 3 bits (GPTQ_MOE_LOW_BIT_PREFILL): moe_panel_lowbit_kernel on the copy's 8- / 12-byte lanes, chunks = K / 128 as at 4 bits
constexpr int GPTQ_MOE_PREFILL_MAX_ROWS = 65535;    // T topk: the gather's grid
struct MoePrefillPlan : RouteLayout {
    bool act_pair, act_down;                        // some gate / up (down) expert is act-order: two planes of x_sorted / the gather of H_sorted
    int bm, tiles, launches;                        // tile height, tile bound
    int nt_pair, nt_down;                           // 32-column blocks of I (of both W1 and W3) / of H per workgroup
    int waves_pair, waves_down, spw_pair, spw_down, lds_pair, lds_down;
    size_t off_xs, off_h, off_y, off_hg, bytes;     // workspace layout behind the routing block (from GPTQ_WORKSPACE_HEADER_BYTES on)
};
bool moe_prefill_group_ok(const gptq_layer_t& L);  // 64 times a power of two, or one group
MoePrefillPlan plan_moe_prefill(const gptq_moe_t& m, int T, int topk);
hipError_t launch_moe_prefill(const gptq_moe_t& m, const void* table, const MoePrefillPlan& pl, const void* x, const int64_t* idx, const float* w, int T, int topk,
                              void* out, char* ws, hipStream_t st);
hipError_t init_moe_prefill_device();
// ... and the DENSE form of moe_panel_lowbit_kernel<T, 2> (opt-in: copy_rows_int2): a workgroup = 64 rows x 128 columns x the whole K.  PanelPlan: mt = 2, nt = 4, kp = 8.
bool dense_panel_int2_ok(const gptq_layer_t& L, int M);
PanelPlan plan_dense_panel_int2(const gptq_layer_t& L, int M);
hipError_t launch_dense_panel_int2(const gptq_layer_t& L, const void* x, void* out, int M, const PanelPlan& pl, hipStream_t st);
// lora.hip: the adapter branch out += scale * (x . A^T) . B^T for up to GPTQ_LORA_MAX adapters that share x: one down launch, one up launch
constexpr int GPTQ_LORA_GEMV_ROWS = 8;              // up to here the VALU forms, above the matrix-core forms
struct LoraPlan {
    bool gemv;
    long mtiles, units_down, units_up, wg_down, wg_up;
};
LoraPlan plan_lora(const gptq_lora_t* const* Ls, int n, int M);
hipError_t launch_lora_down(const gptq_lora_t* const* Ls, int n, const void* x, void* const* u, int M, hipStream_t st);
hipError_t launch_lora_up(const gptq_lora_t* const* Ls, int n, const void* const* u, void* const* outs, int M, hipStream_t st);
// moe_router.hip: the router of a routed layer (gptq_moe_router): logits, softmax and top-k in one launch, no workspace
constexpr int GPTQ_ROUTER_ROWS = 8;                 // up to here one token per workgroup (VALU), above 16 tokens per workgroup (matrix core)
constexpr size_t GPTQ_ROUTER_MAX_LDS = 65536;       // dynamic LDS the kernel may ask for without a grant
struct RouterPlan {
    bool rows;
    long wg;
    size_t lds_bytes;
};
RouterPlan plan_moe_router(int T, int H, int E, int topk, int dtype);
hipError_t launch_moe_router(const void* x, const void* w, int T, int H, int E, int topk, int dtype, int renorm, void* logits, int64_t* idx, float* wts,
                             hipStream_t st);
// the grouped-sigmoid form of the same kernels (gptq_moe_router_grouped): fp32 logits, sigmoid scores, group-limited top-k; plan_moe_router's grid and LDS
hipError_t launch_moe_router_grouped(const void* x, const void* w, const float* bias, int T, int H, int E, int topk, int n_group, int topk_group, float scale,
                                     int dtype, int renorm, float* logits, float* scores, int64_t* idx, float* wts, hipStream_t st);
// adapter_grad.hip: the adapters' weight gradients dA = s du^T x and dB = s dY^T u (gptq_lora_backward): one launch over all jobs, one more to add the
// M-slices where a job has more than one.  A job is one output [P][Q] with one of P, Q = r; slices are a function of (M, P, Q) alone.
constexpr int GPTQ_WGRAD_JOBS = 2 * GPTQ_LORA_MAX;
struct WgradSlices {
    int S, steps_per_slice;                         // steps are 32 rows
};
struct WgradPlan {
    int jobs;                                       // outputs asked for
    WgradSlices sl[GPTQ_WGRAD_JOBS];                // [2 i] dA of adapter i, [2 i + 1] its dB (S = 0: not asked for)
    size_t off[GPTQ_WGRAD_JOBS];                    // workspace offset of the job's partials (S > 1)
    long wg_wgrad, wg_sum;
    size_t bytes;                                   // of all adapters' two outputs, asked for or not
};
WgradSlices wgrad_slices(int M, int P, int Q);
WgradPlan plan_wgrad(const gptq_lora_t* const* Ls, const gptq_lora_grad_t* const* Gs, int n, int M);   // Gs NULL: every output
hipError_t launch_wgrad(const gptq_lora_t* const* Ls, const gptq_lora_grad_t* const* Gs, int n, const void* x, int M, const WgradPlan& pl, char* ws,
                        hipStream_t st);
// adapter_rows.hip: per-row adapter banks (gptq_adapter_route, gptq_adapter_rows_apply): moe_route_kernel with 16-row tiles, one down launch, one up launch
constexpr int GPTQ_ADAPTER_TILE_ROWS = 16;
constexpr int GPTQ_ADAPTER_MAX_SLOTS = 256;         // the routing kernel's LDS arrays
struct AdapterRoutePlan : RouteLayout {
    long tiles;                                     // tile bound: M / 16 + min(slots, M)
    size_t bytes;                                   // of the route buffer: the routing block from offset 0
};
struct AdapterRowsPlan {
    long tiles, units_down, units_up, wg_down, wg_up;
};
AdapterRoutePlan plan_adapter_route(int M, int slots);
AdapterRowsPlan plan_adapter_rows(const gptq_adapter_bank_t* const* Bs, int n, int M);
hipError_t launch_adapter_route(const int64_t* ids, int M, int slots, char* route, hipStream_t st);
hipError_t launch_adapter_rows(const gptq_adapter_bank_t* const* Bs, int n, const void* x, void* const* u, void* const* outs, const void* route, int M,
                               hipStream_t st);
hipError_t launch_unpack_weights(const uint32_t* qweight, int K, int N, int bits, uint8_t* w_out, hipStream_t st);
hipError_t launch_unpack_zeros(const uint32_t* qzeros, int G, int N, int bits, int zero_mode, int32_t* z_out, hipStream_t st);
hipError_t launch_pack_weights(const void* W, const void* scale_in, const void* zero_in, const int32_t* g_idx,
                               int K, int N, int bits, int group_size, int w_dtype, int qparam_dtype,
                               uint32_t* qweight_out, void* scales_out, hipStream_t st);
hipError_t launch_pack_zeros(const void* zero_in, int G, int N, int bits, int qparam_dtype, uint32_t* qzeros_out, hipStream_t st);
hipError_t launch_resequence(const uint32_t* qweight, const int32_t* perm, int K, int N, int bits,
                             uint32_t* out, hipStream_t st);
hipError_t launch_awq_unpack(const uint32_t* aq, const uint32_t* az, const void* scales, int K, int N, int group_size, void* w_kn, int8_t* zeros, hipStream_t st);
hipError_t launch_awq_repack(const uint32_t* aq, const uint32_t* az, int K, int N, int group_size, uint32_t* qweight, uint32_t* qzeros, hipStream_t st);
hipError_t launch_silu_mul(const void* y, void* out, int M, int N, int dtype, int act, hipStream_t st);      // act: GPTQ_EPI_SILU_MUL / GPTQ_EPI_GELU_TANH_MUL (gated_act), or RELU / GELU / GELU_TANH (plain_act) with y == out: all M N elements in place
hipError_t launch_permute_rows16(const void* x, const int32_t* perm, int M, int K, void* x_out, hipStream_t st, bool slot_order = false);
hipError_t launch_permute_columns(const void* x, const int32_t* perm, int M, int K, int dtype, void* x_out, hipStream_t st);
// peer.hip: direct peer-store all-gather (y_local / out may be NULL: scatter-only / collect-only)
hipError_t launch_peer_scatter(const gptq_peer_group_t& pg, const void* y_local, int M, int n_local, int dtype, hipStream_t st);
hipError_t launch_peer_publish(const gptq_peer_group_t& pg, hipStream_t st);
hipError_t launch_peer_collect(const gptq_peer_group_t& pg, void* out, int M, int dtype, unsigned max_spins, hipStream_t st);

}  // namespace gptq
