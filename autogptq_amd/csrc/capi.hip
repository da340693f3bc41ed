// capi.hip -- the extern "C" boundary declared in include/gptq_mi355x.h: argument validation,
// path selection, error reporting.  No allocation, no synchronisation, no global mutable state
// (the only static storage is the thread-local last-error string).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.cuh"
#include "launch.h"
#include "../../include/gptq_mi355x_lab.h"

using namespace gptq;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(GPTQ_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

// What a describe function answers for a call its checker declined: the last error as one key=value token (blanks and '=' become '_').
int describe_decline(char* out, size_t out_bytes, const char* path_word) {
    char reason[sizeof(g_err)];
    snprintf(reason, sizeof(reason), "%s", g_err);
    for (char* c = reason; *c; ++c)
        if (*c == ' ' || *c == '=') *c = '_';
    snprintf(out, out_bytes, "path=%s reason=%s", path_word, reason);
    return GPTQ_OK;
}

bool bits_ok(int b) { return b == 2 || b == 3 || b == 4 || b == 8; }
bool dtype_ok(int d) { return d == GPTQ_F16 || d == GPTQ_BF16 || d == GPTQ_F32; }

// Shape rules of the checkpoint layout (qlinear_cuda.py:51-75): K % 32 == 0 and N % 32 == 0 are
// what `infeatures // 32 * bits` / `outfeatures // 32 * bits` silently assume.
int check_layer(const gptq_layer_t* L) {
    if (!L) return fail(GPTQ_ERR_NULL, "layer is NULL");
    if (!L->qweight || !L->qzeros || !L->scales) return fail(GPTQ_ERR_NULL, "qweight/qzeros/scales must be non-NULL");
    if (!bits_ok(L->bits)) return fail(GPTQ_ERR_UNSUPPORTED, "Only 2,3,4,8 bits are supported. (got %d)", L->bits);
    if (!dtype_ok(L->dtype)) return fail(GPTQ_ERR_UNSUPPORTED, "unsupported dtype enum %d", L->dtype);
    if (L->zero_mode != GPTQ_ZERO_WRAP && L->zero_mode != GPTQ_ZERO_NOWRAP)
        return fail(GPTQ_ERR_UNSUPPORTED, "unknown zero_mode %d", L->zero_mode);
    if (L->K <= 0 || L->N <= 0 || L->K % 32 || L->N % 32)
        return fail(GPTQ_ERR_SHAPE, "in_features (%d) and out_features (%d) must be positive multiples of 32", L->K, L->N);
    if (L->group_size <= 0) return fail(GPTQ_ERR_SHAPE, "group_size must be > 0 (resolve -1 to in_features), got %d", L->group_size);
    if ((L->qweight_seq == nullptr) != (L->perm == nullptr))
        return fail(GPTQ_ERR_NULL, "qweight_seq and perm must be given together");
    // (tiled_cols may carry GPTQ_COPY_ROWS_INT2: copy_cols masks it; the flag on a layer without a copy, or of another width, means nothing)
    if ((L->qweight_tiled != nullptr) != (copy_cols(*L) != 0) || (L->qweight_tiled != nullptr) != (L->qconst_tiled != nullptr) ||
        (copy_cols(*L) != 0 && copy_cols(*L) != GPTQ_STRIP_COLS))
        return fail(GPTQ_ERR_UNSUPPORTED, "qweight_tiled, qconst_tiled and tiled_cols (%d) must be given together, tiled_cols = %d", L->tiled_cols, GPTQ_STRIP_COLS);
    if (L->epilogue != GPTQ_EPI_NONE && !is_gated(L->epilogue) && !is_plain_act(L->epilogue))
        return fail(GPTQ_ERR_UNSUPPORTED, "unknown epilogue %d", L->epilogue);
    if (is_gated(L->epilogue) && L->N % 64)
        return fail(GPTQ_ERR_SHAPE, "the %s epilogue needs out_features (%d) to be a multiple of 64 ([gate | up] halves)", L->epilogue == GPTQ_EPI_SILU_MUL ? "SILU_MUL" : "GELU_TANH_MUL", L->N);
    return GPTQ_OK;
}

int check_io(const void* x, const void* out, int M) {
    if (!x || !out) return fail(GPTQ_ERR_NULL, "x/out must be non-NULL");
    if (M <= 0) return fail(GPTQ_ERR_SHAPE, "M must be > 0, got %d", M);
    return GPTQ_OK;
}

// x / out / outs[i] / workspace of the dense entry points: the kernels load x by LDS DMA and 16-byte vectors and lay the workspace out in 16-byte
// granules -- anything else is refused before a launch (the wrappers copy a misaligned x first).  NULL passes: the NULL checks name those.
int check_align(const void* x, const void* out, const void* ws) {
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)ws) & 15) return fail(GPTQ_ERR_UNSUPPORTED, "x / out / workspace must be 16-byte aligned");
    return GPTQ_OK;
}

// The GEMM step of the ladder (route_forward).  plan() is plan_gemm(*L, M, t), computed at most once; want_gemm below hands it to the caller.
template <typename Plan>
bool gemm_rule(const gptq_layer_t* L, int M, const gptq_tuning_t* t, Plan&& plan) {
    if (t && t->path == 3) return true;
    if (t && (t->path == 1 || t->path == 2 || t->path == 4 || t->path == 5)) return false;
    // M = 5..8 on wide layers: the GEMV needs two matrix-core passes per weight word there, and a wide N gives the tiled kernel
    // enough 256-column tiles to fill the chip (4096x11008, M = 8: 22.2 us GEMV, 17.8 us tiled; narrower layers: GEMV wins)
    const bool wide_small_batch = M >= 5 && L->bits == 4 && L->N > 8192 && L->epilogue == GPTQ_EPI_NONE;
    if (L->dtype == GPTQ_F32) {
        // fp32 layers: the exact-f32 matrix-core kernel runs whole 128-row tiles with no K split; up to 64 rows the 4-rows-per-pass GEMV
        // is faster or equal on every shape (tools/cliff_scan.py --slice D: 4096x11008 M = 8: 517 us against ~60; M = 64: 528 against
        // ~510; 4096x4096 M = 64 on 32 tiles: 455 against 85)
        if (M <= 64) return false;
        const GemmPlan& gf = plan();
        return gf.supported && (long)gf.nbm * gf.nbn >= 64;      // fewer tiles than a quarter of the chip: the GEMV still wins (4096x4096 M = 128: ~170 us against 455)
    }
    if (!t && L->epilogue == GPTQ_EPI_NONE && rows_pays(*L, M)) return true;      // 5 .. 128 rows from the decode copy (gemm_rows.hip; plan_gemm picks it)
    if (!t && L->epilogue == GPTQ_EPI_NONE && dense_int2_choice(*L, M)) return true;      // a flagged 2-bit layer where its 4-bit twin has the rows / panel kernel (plan_gemm picks the low-bit form)
    if (L->bits != 4) {
        // 2/3/8-bit: the matrix-core GEMV handles 4 rows of x per pass over the weights and the generic (act-order) kernel fewer, so the
        // weight-streaming GEMMs take over early (tools/cliff_scan.py --slice C, 4096x11008, us: int8 M = 8: 47.6 GEMV, 25.6 tiled at
        // M = 16; int8 act-order M = 4: 43.7 against 29.5; int3 M = 8: 26.2 against 35.8 -- 3-bit keeps the GEMV up to 8 rows)
        // (act-order layers with the re-sequenced side copy run the same kernels on a permuted x -- GEMV and GEMM alike pay one 2.6 us
        // pre-pass -- so they share the plain layers' crossovers; only raw act-order layers, which sit on the fp32 generic GEMV, leave early)
        const bool raw_act = L->g_idx != nullptr && !(L->qweight_seq != nullptr && L->perm != nullptr);
        const bool big = (size_t)L->K * L->N >= ((size_t)32 << 20);
        // int8 fp16 on layers of at most 256 strips: the one-pass 8-row GEMV beats the GEMMs up to 8 rows (us at M = 8, GEMV / GEMM: 4096x4096
        // 12.5 / 16.6, 11008x4096 27.2 / 32.4; 4096x11008 26.0 / 23.6 keeps the GEMM from 5 rows)
        const bool int8_rows8 = L->bits == 8 && L->dtype == GPTQ_F16 && L->N <= 4096 && L->epilogue == GPTQ_EPI_NONE && !raw_act;
        const int min_m = raw_act ? (L->bits == 8 ? 3 : 5) : (L->bits == 8 ? (int8_rows8 ? 9 : 5) : ((L->bits == 2 && big) ? 5 : 9));
        if (M >= 5 && M < min_m && L->epilogue == GPTQ_EPI_NONE && !raw_act) {
            const GemmPlan& g8 = plan();                          // 5..8 rows: the 2- / 3- / 8-bit forms of gemm_mid_kernel where the planner takes them (tools/nonq4_batched.py:
            if (g8.supported && g8.kernel == GEMM_MID) return true;             // 11008x4096 M = 8 27.1 -> 16.1 us, 4096x4096 12.3 -> 11.1)
        }
        if (M < min_m) return false;
        return plan().supported;
    }
    if (M <= 2) return false;
    const GemmPlan& g = plan();
    // M = 3..4: only the unsplit streamed 64-column-strip kernel (160+ strips) beats the GEMVs there (tools/cliff_scan.py, us, M = 3 / 4 / 5:
    // 4096x11008 11.8 / 12.0 / 10.8, 5120x13824 15.0 / 15.8 / 13.1 -- the M = 5 column is that kernel, whose time barely depends on M up to 16)
    if (M <= 4 && !(g.supported && g.kernel == GEMM_STREAM64 && g.ksplit == 1 && L->epilogue == GPTQ_EPI_NONE)) return false;
    // M = 5..8: the streamed 64-column-strip kernel (one matrix-core pass for up to 16 rows, weights by LDS DMA) where it exists;
    // layers with a fused epilogue keep the GEMV that applies it
    // (and the 16-column-strip kernel on narrow layers: 4096x4096 M = 5 / 8: 7.3 / 7.9 us against the GEMV's 8.0 / 8.3)
    // (28672x1024, M = 8: GEMV 14.8, 16-column strips 17.0 -- long K keeps the GEMV)
    const bool small_batch_stream = g.supported && (g.kernel == GEMM_STREAM64 || (g.kernel == GEMM_STRIP16 && L->K <= 8192)) && L->epilogue == GPTQ_EPI_NONE;
    if (M <= 8 && !wide_small_batch && !small_batch_stream) return false;
    return g.supported;
}
// *g: plan_gemm(*L, M, t) wherever the answer is yes (M <= 0 excepted: check_io refuses the call before anything reads the plan)
bool want_gemm(const gptq_layer_t* L, int M, const gptq_tuning_t* t, GemmPlan* g) {
    bool planned = false;
    auto plan = [&]() -> const GemmPlan& { return planned ? *g : (planned = true, *g = plan_gemm(*L, M, t)); };
    const bool want = gemm_rule(L, M, t, plan);
    if (want && M > 0) plan();
    return want;
}

// The streamed GEMV (weights by LDS DMA, in-launch K-split combine) for a single layer: forced by tuning.path = 6, else by
// the planner's measured preference.
bool want_stream(const gptq_layer_t* L, int M, const gptq_tuning_t* t, StreamPlan* plan_out) {
    if (M > 4 || L->epilogue != GPTQ_EPI_NONE) return false;
    if (t && t->path != 0 && t->path != 6) return false;
    const gptq_layer_t* one[1] = {L};
    const StreamPlan& sp = *plan_out = plan_stream(one, 1, M, t);
    if (!sp.ok) return false;
    if (t && t->path == 6) return true;
    if (M >= 3) {                                      // 3..4 rows on layers of 160+ strips: the batched-decode kernel (want_gemm)
        const Stream64Plan s64 = plan_stream64(one, 1, M, nullptr);
        if (s64.ok && s64.pays && s64.ksplit == 1) return false;
    }
    return stream_preferred(*L, M);
}

// Decode from the strip-major side copy (gemv_tiled.hip): 3- / 4- / 8-bit fp16 / bf16 layers (plain or act-order) that carry qweight_tiled, M <= 4.  tuning.path = 8 forces it
// ("does not fit" is then an error), any other explicit path keeps the checkpoint-layout kernels (A/B runs).
// 5..8 rows (MT = 8: two matrix-core steps per decoded pair, 8 staged rows of x per workgroup): every 16-column strip stages its own copy of x, which is what
// this form loses to the 64-column-strip kernels on wide layers (tools/tiled_sweep.py --m 8, profiles/r04_tiled_sweep_m8.log, us, this / checkpoint-layout
// default: 11008x4096 18.7 / 12.3, 4096x11008 12.9 / 10.8, q|k|v 13.1 / 11.7, gate|up 22.1 / 18.3) and wins only on a single square-ish 4096-wide layer
// (4096^2: 6.62 / 7.20) -- the planner takes it there by itself (profiles/r04_tiled_sweep_rows8_default_rule.log, M = 8: 4096^2 6.60 / 7.29, 2048^2 4.78 / 6.89,
// 4096x2048 5.95 / 7.66, 2048x4096 5.05 / 5.25, 3072^2 6.16 / 6.10; M = 5: 6.47 / 7.11, 4.77 / 6.79), tuning.path = 8 asks for it anywhere.
constexpr int TILED_ROWS_MAX = 8;
static bool tiled_rows8_pays(const gptq_layer_t* const* Ls, int n) {
    const gptq_layer_t& L = *Ls[0];
    if (n == 1 && L.bits == 4 && !L.g_idx && L.K >= 2048 && L.K <= 4096 && L.N >= 2048 && L.N <= 4096) return true;
    // launches of 1024+ strips (gate|up of a 7B block): two strips per workgroup behind one staged x (gemv_tiled_multi.hip) -- M = 8 16.5 us against 17.3 for
    // the batched-decode kernel on the checkpoint rows (profiles/r05_multi_strip_ab.log); 8 rows of x over the whole K have to fit the LDS
    long strips = 0;
    for (int i = 0; i < n; ++i) {
        if (Ls[i]->bits != 4 || Ls[i]->g_idx || Ls[i]->N % 32) return false;
        strips += Ls[i]->N / 16;
    }
    return n >= 2 && strips >= 1024 && L.K <= 4096;
}
// plan_out: the plan the answer was derived from
bool want_tiled(const gptq_layer_t* const* Ls, int n, int M, const gptq_tuning_t* t, TiledPlan* plan_out) {
    if (M > TILED_ROWS_MAX || n < 1 || n > 4) return false;
    if (Ls[0]->qweight_tiled == nullptr) return false;
    if (Ls[0]->epilogue != GPTQ_EPI_NONE && (n != 1 || M > 4)) return false;     // a [gate | up] layer: the pair form of the kernel (gemv_tiled_pair.hip)
    if (M > 4 && !(t && t->path == 8) && n == 1 && rows_pays(*Ls[0], M)) return false;      // 5+ rows of one layer: the exchange-free batched-decode kernel (gemm_rows.hip: 4096^2 M = 5 / 8 7.1 / 7.3 -> 5.5 / 5.6 us)
    if (M > 4 && !(t && t->path == 8) && !tiled_rows8_pays(Ls, n)) return false;
    if (t && t->path != 0 && t->path != 8) return false;
    // act-order layers at 3 - 4 rows from K = 5120: the in-kernel gather holds the raw AND the gathered rows of x in LDS (2 x 4 rows x K: one workgroup per CU from
    // K = 5120) -- the permute pre-pass + the kernels of the 5+-row path are faster there (tools/m_sweep.py --act, profiles/r06_act_m4.log, 4 rows against 5:
    // 5120x13824 26.5 / 14.7 us, 8192^2 18.3 / 14.8, 6656^2 16.7 / 15.6, 5120^2 13.1 / 12.3; 4096-deep layers keep this kernel: 4096x11008 11.7 / 12.9).  (act-order
    // layers are never released to the host: nothing assumes the decode copy for them)
    // narrow layers (tensor-parallel shards, N < 4096) keep it: 8192x3584 9.2 against 10.9, 8192x1024 8.1 / 9.8
    if (!(t && t->path == 8) && M >= 3 && M <= 4 && Ls[0]->g_idx && Ls[0]->K >= 5120 && Ls[0]->N >= 4096 && n == 1) return false;
    // ... and at 2 rows from K = 12288 (2 x 2 rows x K of LDS again leave one workgroup per CU): 13824x5120 21.4 us against 18.7 at THREE rows on the pre-pass + streamed kernel
    // (layers of more than 256 strips only: 14336x4096 runs one workgroup per CU either way and keeps this kernel)
    if (!(t && t->path == 8) && M == 2 && Ls[0]->g_idx && Ls[0]->K >= 12288 && Ls[0]->N > 4096 && n == 1) return false;
    *plan_out = plan_tiled(Ls, n, M, t);                           // act-order layers: the copy holds the re-sequenced rows, the kernel gathers x through perm
    return plan_out->ok;
}

// act-order layers on the streamed GEMV: x permuted once by the column-permute pre-pass, the kernel streams the re-sequenced rows of a
// plain copy of the layer.  Where the streamed kernel is the planner's choice for that copy (tools/cliff_scan.py --slice F, us, in-kernel
// gather / register kernel -> this: 13824x5120 M = 1 / 2 / 4 19.6 / 24.7 / 26.9 -> ~17 / 17.3 / 19.8; 8192x28672 M = 1 37.0 -> ~31); with
// one row only from 33 MiB up -- below that the in-kernel gather is cheaper than the 2.6 us pre-pass (5120x5120: 9.7 against 10.1).
static bool want_stream_seq(const gptq_layer_t* L, int M, const gptq_tuning_t* t, gptq_layer_t* P, StreamPlan* plan_out) {
    if (t || !L->g_idx || !L->qweight_seq || !L->perm || L->epilogue != GPTQ_EPI_NONE || M > 4) return false;
    *P = *L;
    P->g_idx = nullptr; P->perm = nullptr; P->qweight = L->qweight_seq; P->qweight_seq = nullptr;
    if (!want_stream(P, M, nullptr, plan_out)) return false;
    if (M == 1 && (size_t)L->K * L->N * L->bits / 8 < ((size_t)33 << 20)) return false;
    return true;
}
static size_t xperm16_bytes(const gptq_layer_t* L, int M) { return ((size_t)M * L->K * 2 + 255) / 256 * 256; }

// workspace split: [ticket header | body]
struct WsView { void* header; void* body; size_t body_bytes; };
WsView split_ws(void* ws, size_t ws_bytes) {
    if (!ws || ws_bytes <= WS_HEADER_BYTES) return WsView{nullptr, nullptr, 0};
    return WsView{ws, (char*)ws + WS_HEADER_BYTES, ws_bytes - WS_HEADER_BYTES};
}
int need_body(const WsView& wv, size_t body) {      // the refusal of a call whose workspace is shorter than the header + `body` bytes
    if (wv.body_bytes >= body) return GPTQ_OK;
    return fail(GPTQ_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", WS_HEADER_BYTES + body, wv.header ? WS_HEADER_BYTES + wv.body_bytes : (size_t)0);
}

}  // namespace

extern "C" {

int gptq_abi_version(void) { return GPTQ_MI355X_ABI_VERSION; }
const char* gptq_last_error(void) { return g_err; }

const char* gptq_status_string(int s) {
    switch (s) {
        case GPTQ_OK: return "ok";
        case GPTQ_ERR_NULL: return "null pointer";
        case GPTQ_ERR_SHAPE: return "bad shape";
        case GPTQ_ERR_UNSUPPORTED: return "unsupported configuration";
        case GPTQ_ERR_WORKSPACE: return "workspace too small";
        case GPTQ_ERR_LAUNCH: return "HIP launch failure";
        default: return "unknown status";
    }
}

// Unfused SILU_MUL / GELU_TANH_MUL: y[M, N] goes to the front of the workspace, the elementwise pass writes out[M, N/2].
// Unfused RELU / GELU / GELU_TANH: y goes to out[M, N] and the pass runs on it in place -- nothing is staged.
static size_t epi_scratch_bytes(const gptq_layer_t* L, int M) {
    if (is_plain_act(L->epilogue)) return 0;
    const size_t b = (size_t)M * L->N * dtype_size(L->dtype);
    return (b + 255) / 256 * 256;
}
// A [gate | up] layer with 3..8 rows of x: the GEMV's fused forms for 3+ rows (MT = 4, two passes for 5..8 rows) lose to the streamed
// 64-column-strip kernel followed by the elementwise pass (4096 x 22016, tools/fused_small_batch.py: M = 4 27.7 -> 19.5 us,
// M = 5 / 8 47.6 / 50.8 -> 19.3 / 19.5 us; M = 1 / 2 stay fused: 16.7 / 21.2 us).  Returns the tuning the inner (epilogue-stripped)
// call runs with: the caller's, or -- for 3..4 rows, below the planner's own threshold for that kernel -- a local one that asks for it.
static bool small_batch_stream_for_epilogue(const gptq_layer_t* L, int M) {
    if (!is_gated(L->epilogue) || M < 3 || M > 8) return false;
    gptq_layer_t Lc = *L;
    Lc.epilogue = GPTQ_EPI_NONE;
    const gptq_layer_t* one[1] = {&Lc};
    const Stream64Plan sp = plan_stream64(one, 1, M, nullptr);
    return sp.ok && sp.pays;
}
static const gptq_tuning_t* inner_tuning(const gptq_layer_t* L, int M, const gptq_tuning_t* tune, gptq_tuning_t* local) {
    if (tune) return tune;
    if (M <= 4 && small_batch_stream_for_epilogue(L, M)) {
        *local = gptq_tuning_t{};
        local->path = 3;
        local->reserved[2] = 4;
        return local;
    }
    return nullptr;
}

// ---- the route of one dense forward call --------------------------------------------------------------------------------
// route_forward walks the ladder of want_* questions ONCE, in the order below, stops at the first hit and computes the one sub-plan that answer came from
// (a decode call -- tiled at the first step -- runs plan_tiled and nothing else: a launch of that kernel takes 4.5 us and the host side of an eager call is
// measured in the same unit, tools/host_cost.py).  The launch (forward_impl), the workspace query (query_body_bytes), gptq_describe_plan, the MLP entry
// points, separate_panels_pay and gptq_forward_scatter read the route; none of them asks a want_* question itself.
enum RouteKind {
    ROUTE_TILED,          // decode-copy kernel (tp)
    ROUTE_TILED_PAIR,     // ... with act(gate) * up as its epilogue (round 5): decode rows of a [gate | up] layer that carries its copy, one launch, no scratch
    ROUTE_STREAM,         // streamed GEMV (sp)
    ROUTE_STREAM_SEQ,     // x permuted by the pre-pass into the front of the body, then the streamed GEMV on `seq`, the plain copy of the act-order layer (sp)
    ROUTE_GEMM,           // gp
    ROUTE_GEMV,           // vp
};
struct ForwardRoute {             // (only the scalars are initialised: a plan is written before its kind is set)
    RouteKind kind;
    int declined = 0;     // a forced tuning.path (8 / 6) the call does not fit: gptq_forward_ex returns route_decline(); the host-only queries have always
                          // answered such a call with the rest of the ladder, so that is what kind / plans / body hold
    // SILU_MUL as an elementwise pass of its own: y = [gate | up] sits in the first epi_bytes of the body, and everything else here is the route of the
    // INNER call -- on `plain` (the layer without its epilogue), under tuning(): the caller's, or the `local` one inner_tuning made
    bool unfused_epilogue = false, own_tuning = false;
    gptq_layer_t plain, seq;
    gptq_tuning_t local;
    TiledPlan tp; StreamPlan sp; GemmPlan gp; GemvPlan vp;      // the ONE sub-plan of `kind`
    size_t epi_bytes = 0, body = 0;      // body: bytes behind the ticket header this route needs (epi_bytes included)
    const gptq_layer_t* layer(const gptq_layer_t* L) const { return unfused_epilogue ? &plain : L; }
    const gptq_tuning_t* tuning(const gptq_tuning_t* t) const { return own_tuning ? &local : t; }
    bool hit(RouteKind k, size_t need) { kind = k; body = epi_bytes + need; return true; }
};
static ForwardRoute route_forward(const gptq_layer_t* L, int M, const gptq_tuning_t* tune) {
    ForwardRoute r;
    const gptq_layer_t* one[1] = {L};
    if (want_tiled(one, 1, M, tune, &r.tp) && r.hit(L->epilogue == GPTQ_EPI_NONE ? ROUTE_TILED : ROUTE_TILED_PAIR, r.tp.partial_bytes)) return r;
    if (L->epilogue != GPTQ_EPI_NONE) {
        // fused: the GEMV applies the epilogue itself, where the GEMV is the choice and has the pair form (path = 6 does not fit a layer with an epilogue)
        if ((tune || !small_batch_stream_for_epilogue(L, M)) && is_gated(L->epilogue) && !want_gemm(L, M, tune, &r.gp)) {
            r.vp = plan_gemv(*L, M, tune);
            r.declined = (r.vp.pair && tune && tune->path == 6) ? 6 : 0;
            if (r.vp.pair && r.hit(ROUTE_GEMV, r.vp.workspace_bytes)) return r;
        }
        r.unfused_epilogue = true;
        r.epi_bytes = epi_scratch_bytes(L, M);
        r.plain = *L;
        r.plain.epilogue = GPTQ_EPI_NONE;
        r.own_tuning = inner_tuning(L, M, tune, &r.local) == &r.local;
        one[0] = L = &r.plain;
        tune = r.tuning(tune);
        if (want_tiled(one, 1, M, tune, &r.tp) && r.hit(ROUTE_TILED, r.tp.partial_bytes)) return r;
    }
    if (tune && tune->path == 8) r.declined = 8;
    if (want_stream(L, M, tune, &r.sp) && r.hit(ROUTE_STREAM, r.sp.partial_bytes)) return r;
    if (want_stream_seq(L, M, tune, &r.seq, &r.sp) && r.hit(ROUTE_STREAM_SEQ, xperm16_bytes(L, M) + r.sp.partial_bytes)) return r;
    if (tune && tune->path == 6) r.declined = 6;
    if (want_gemm(L, M, tune, &r.gp) && r.hit(ROUTE_GEMM, r.gp.supported ? r.gp.workspace_bytes : 0)) return r;
    r.hit(ROUTE_GEMV, M > 0 ? (r.vp = plan_gemv(*L, M, tune)).workspace_bytes : 0);      // (M <= 0: check_io refuses the call before anything reads the plan)
    return r;
}
static int route_decline(const ForwardRoute& r) {
    if (r.declined == 8) return fail(GPTQ_ERR_UNSUPPORTED, "tuning.path = 8: the decode-copy kernel needs M <= 8 and a plain or re-sequenced act-order 3/4/8-bit fp16/bf16 layer that carries qweight_tiled / qconst_tiled "
                                          "(gptq_prepack_decode; tiled_cols = %d)", GPTQ_STRIP_COLS);
    return fail(GPTQ_ERR_UNSUPPORTED, "tuning.path = 6: the streamed GEMV needs M <= 4, a plain 4-bit fp16/bf16 layer (no act-order, no epilogue) "
                                      "and a launch shape with rows-per-lane in {2, 4, 8} dividing the rows of a group");
}

// Body = what the kernels use behind the ticket header; the public figure adds the header whenever there is a body.
// The header documents gptq_workspace_bytes* as covering gptq_forward, gptq_gemv AND gptq_gemm on the layer: a caller may size one workspace with the query and
// then call any of the three.  So the query is max(route need, GEMV need, GEMM need) -- except for the routes that exist only behind gptq_forward and need
// (next to) nothing: the decode-copy kernel, and the exchange-free rows / panel GEMMs (nothing but the permuted x of act-order layers).
static size_t query_body_bytes(const gptq_layer_t* L, int M, const gptq_tuning_t* tune) {
    const ForwardRoute r = route_forward(L, M, tune);
    if (r.kind == ROUTE_TILED || r.kind == ROUTE_TILED_PAIR) return r.body;
    if (r.kind == ROUTE_GEMM && r.gp.supported && (r.gp.kernel == GEMM_ROWS || r.gp.kernel == GEMM_PANEL)) return r.body;
    const gptq_layer_t* Lr = r.layer(L);
    const size_t a = r.kind == ROUTE_GEMV ? r.vp.workspace_bytes : plan_gemv(*Lr, M, r.tuning(tune)).workspace_bytes;
    const GemmPlan g = r.kind == ROUTE_GEMM ? r.gp : plan_gemm(*Lr, M, r.tuning(tune));
    const size_t b = g.supported ? g.workspace_bytes : 0;
    return std::max(r.body, r.epi_bytes + std::max(a, b));      // (the inner call of an unfused epilogue shares the ONE zeroed ticket header; its body starts behind y)
}

size_t gptq_workspace_bytes_ex(const gptq_layer_t* L, int M, const gptq_tuning_t* tune) {
    if (check_layer(L) != GPTQ_OK || M <= 0) return 0;
    const size_t b = query_body_bytes(L, M, tune);
    return b ? WS_HEADER_BYTES + b : 0;
}

size_t gptq_workspace_bytes(const gptq_layer_t* L, int M) { return gptq_workspace_bytes_ex(L, M, nullptr); }

size_t gptq_workspace_bytes_max(const gptq_layer_t* L, int max_M) {
    size_t best = 0;
    for (int M = 1; M <= max_M; ++M) best = std::max(best, gptq_workspace_bytes_ex(L, M, nullptr));   // host arithmetic only
    return best;
}

int gptq_init(void) {
    hipError_t e = init_gemm_device();
    if (e == hipSuccess) e = init_gemv_device();
    if (e == hipSuccess) e = init_mlp_device();
    if (e == hipSuccess) e = init_gemm_mid_device();
    if (e == hipSuccess) e = init_gemv_tiled_device();
    if (e == hipSuccess) e = init_gemm_wide_sk_device();
    if (e == hipSuccess) e = init_gemm_rows_device();
    if (e == hipSuccess) e = init_gemm_panel_device();
    if (e == hipSuccess) e = init_moe_decode_device();
    if (e == hipSuccess) e = init_moe_shared_device();
    if (e == hipSuccess) e = init_moe_batch_device();
    if (e == hipSuccess) e = init_moe_prefill_device();
    if (e != hipSuccess) return hip_fail(e, "gptq_init (hipFuncSetAttribute)");
    return GPTQ_OK;
}

int gptq_validate_g_idx(const int32_t* g_idx, int K, int G) {
    if (!g_idx) return fail(GPTQ_ERR_NULL, "g_idx is NULL");
    if (K <= 0 || G <= 0) return fail(GPTQ_ERR_SHAPE, "K (%d) and G (%d) must be > 0", K, G);
    for (int k = 0; k < K; ++k)
        if (g_idx[k] < 0 || g_idx[k] >= G)
            return fail(GPTQ_ERR_SHAPE, "g_idx[%d] = %d is outside [0, %d) (rows of scales / qzeros)", k, g_idx[k], G);
    return GPTQ_OK;
}

// The kernels see the workspace as (ticket header, body): the header is the caller's zeroed first 64 KiB and is NEVER relocated -- a call
// that nests another one (the unfused SILU_MUL epilogue) hands the inner call the same header and the rest of its body.  (The cores take the plan their
// caller computed: the route's, or the public gptq_gemv / gptq_gemm's own.)
static int gemv_core(const gptq_layer_t* L, const GemvPlan& pl, const void* x, void* out, int M, const WsView& wv, void* stream, const gptq_tuning_t* tune) {
    if (tune && tune->lanes_n && tune->lanes_n != 4 && tune->lanes_n != 8 && tune->lanes_n != 16 && tune->lanes_n != 64)   // = the header's list
        return fail(GPTQ_ERR_UNSUPPORTED, "tuning.lanes_n must be 4, 8, 16 or 64");
    if (tune && (tune->waves < 0 || tune->waves > 16)) return fail(GPTQ_ERR_UNSUPPORTED, "tuning.waves must be 1..16");
    if (L->epilogue != GPTQ_EPI_NONE && !pl.pair)
        return fail(GPTQ_ERR_UNSUPPORTED, "this GEMV kernel has no fused epilogue; call gptq_forward[_ex], which stages y in the workspace");
    if (tune && tune->path == 5 && !pl.mfma && !pl.mfmag)
        return fail(GPTQ_ERR_UNSUPPORTED, "matrix-core GEMV needs fp16 / bf16, groups of whole packing units (4-bit: a power-of-two group_size >= 8), "
                                          "16-column strips for 2/3/8-bit and no raw act-order g_idx");
    if (pl.mfma && pl.ln != 4 && (L->dtype != GPTQ_F16 || pl.mt > 4 || pl.use_seq || pl.pair || (pl.ln != 8 && pl.ln != 16)))
        return fail(GPTQ_ERR_UNSUPPORTED, "matrix-core GEMV: 32- / 64-column strips (lanes_n = 8 / 16) exist for plain fp16 layers at up to 4 rows only");
    if (!pl.mfma && !pl.mfmag && pl.ln != 4 && pl.ln != 16 && !(pl.ln == 8 && L->dtype == GPTQ_F32))
        return fail(GPTQ_ERR_UNSUPPORTED, "fp32-math GEMV: strips of 16 or 64 columns only (lanes_n = 4 / 16; fp32 layers also 8)");
    if (tune && (tune->path == 2 || tune->path == 4))
        return fail(GPTQ_ERR_UNSUPPORTED, "tuning.path = %d (round 1's LDS-staged / v_dot2 comparison GEMVs) was retired in round 6", tune->path);
    if (int rc = need_body(wv, pl.workspace_bytes)) return rc;
    hipError_t e = launch_gemv(*L, pl, x, out, M, wv.body, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_gemv launch");
    return GPTQ_OK;
}
int gptq_gemv(const gptq_layer_t* L, const void* x, void* out, int M, void* ws, size_t ws_bytes, void* stream,
              const gptq_tuning_t* tune) {
    if (int rc = check_align(x, out, ws)) return rc;
    if (int rc = check_layer(L)) return rc;
    if (int rc = check_io(x, out, M)) return rc;
    return gemv_core(L, plan_gemv(*L, M, tune), x, out, M, split_ws(ws, ws_bytes), stream, tune);
}

static int gemm_core(const gptq_layer_t* L, const GemmPlan& pl, const void* x, void* out, int M, const WsView& wv, void* stream) {
    if (L->epilogue != GPTQ_EPI_NONE)
        return fail(GPTQ_ERR_UNSUPPORTED, "the MFMA GEMM has no fused epilogue; call gptq_forward[_ex], which stages y in the workspace");
    if (!pl.supported)
        return fail(GPTQ_ERR_UNSUPPORTED,
                    "MFMA GEMM needs sequential or re-sequenced groups made of whole packing units (fp16/bf16: group_size %% 32 == 0) (bits=%d dtype=%d group_size=%d)",
                    L->bits, L->dtype, L->group_size);
    if (int rc = need_body(wv, pl.workspace_bytes)) return rc;
    hipError_t e = launch_gemm(*L, pl, x, out, M, wv.header, wv.body, (hipStream_t)stream);
    if (e != hipSuccess)
        return hip_fail(e, pl.kg == 2 ? "gptq_gemm launch (this kernel needs > 64 KiB of LDS: was gptq_init() called on this device?)"
                                      : "gptq_gemm launch");
    return GPTQ_OK;
}
int gptq_gemm(const gptq_layer_t* L, const void* x, void* out, int M, void* ws, size_t ws_bytes, void* stream,
              const gptq_tuning_t* tune) {
    if (int rc = check_align(x, out, ws)) return rc;
    if (int rc = check_layer(L)) return rc;
    if (int rc = check_io(x, out, M)) return rc;
    return gemm_core(L, plan_gemm(*L, M, tune), x, out, M, split_ws(ws, ws_bytes), stream);
}

static int stream_call(const gptq_layer_t* const* Ls, int n, const StreamPlan& sp, const void* x, void* const* outs, int M, const WsView& wv,
                       void* stream) {
    if (int rc = need_body(wv, sp.partial_bytes)) return rc;
    hipError_t e = launch_stream(Ls, sp, x, outs, M, wv.header, wv.body, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq streamed GEMV launch (16 waves x U = 8 needs > 64 KiB of LDS: was gptq_init() called on this device?)");
    return GPTQ_OK;
}

static int tiled_call(const gptq_layer_t* const* Ls, int n, const TiledPlan& tp, const void* x, void* const* outs, int M, const WsView& wv, void* stream) {
    if (int rc = need_body(wv, tp.partial_bytes)) return rc;
    hipError_t e = launch_tiled(Ls, tp, x, outs, M, wv.header, wv.body, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq strip-major decode launch (was gptq_init() called on this device?)");
    return GPTQ_OK;
}

// One routed call on the layer its route's kind applies to (the layer itself, or `plain` inside an unfused epilogue).
static int forward_routed(const ForwardRoute& r, const gptq_layer_t* L, const void* x, void* out, int M, const WsView& wv, void* stream, const gptq_tuning_t* tune) {
    if (r.declined) return route_decline(r);
    if (int rc = check_io(x, out, M)) return rc;
    const gptq_layer_t* one[1] = {r.kind == ROUTE_STREAM_SEQ ? &r.seq : L};
    void* outs[1] = {out};
    switch (r.kind) {
        case ROUTE_TILED:
        case ROUTE_TILED_PAIR: return tiled_call(one, 1, r.tp, x, outs, M, wv, stream);
        case ROUTE_STREAM: return stream_call(one, 1, r.sp, x, outs, M, wv, stream);
        case ROUTE_STREAM_SEQ: {
            const size_t xb = xperm16_bytes(L, M);
            if (int rc = need_body(wv, xb + r.sp.partial_bytes)) return rc;
            hipError_t e = launch_permute_columns(x, L->perm, M, L->K, L->dtype, wv.body, (hipStream_t)stream);
            if (e != hipSuccess) return hip_fail(e, "gptq_permute_columns launch");
            e = launch_stream(one, r.sp, wv.body, outs, M, wv.header, (char*)wv.body + xb, (hipStream_t)stream);
            if (e != hipSuccess) return hip_fail(e, "gptq streamed GEMV launch (was gptq_init() called on this device?)");
            return GPTQ_OK;
        }
        case ROUTE_GEMM: return gemm_core(L, r.gp, x, out, M, wv, stream);
        case ROUTE_GEMV: return gemv_core(L, r.vp, x, out, M, wv, stream, tune);
    }
    return fail(GPTQ_ERR_UNSUPPORTED, "unknown route %d", (int)r.kind);
}

static int forward_impl(const gptq_layer_t* L, const void* x, void* out, int M, const WsView& wv, void* stream, const gptq_tuning_t* tune) {
    if (int rc = check_layer(L)) return rc;
    const ForwardRoute r = route_forward(L, M, tune);
    if (!r.unfused_epilogue) return forward_routed(r, L, x, out, M, wv, stream, tune);
    if (int rc = check_io(x, out, M)) return rc;
    const size_t yb = r.epi_bytes;
    if (wv.body_bytes < yb)
        return fail(GPTQ_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", gptq_workspace_bytes_ex(L, M, tune), wv.header ? WS_HEADER_BYTES + wv.body_bytes : (size_t)0);
    // y = [gate | up] at the front of the body; the inner call gets the SAME zeroed ticket header and the body behind y (a header carved
    // out of the body would sit on whatever an earlier, larger call left there: its tickets would never reach ksplit - 1)
    if (is_plain_act(L->epilogue)) {      // an ungated layer: y = out, the whole workspace is the inner call's, the pass runs in place
        if (int rc = forward_routed(r, &r.plain, x, out, M, wv, stream, r.tuning(tune))) return rc;
        hipError_t e = launch_silu_mul(out, out, M, L->N, L->dtype, L->epilogue, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "activation pass launch");
        return GPTQ_OK;
    }
    if (int rc = forward_routed(r, &r.plain, x, wv.body, M, WsView{wv.header, (char*)wv.body + yb, wv.body_bytes - yb}, stream, r.tuning(tune))) return rc;
    hipError_t e = launch_silu_mul(wv.body, out, M, L->N, L->dtype, L->epilogue, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "silu_mul launch");
    return GPTQ_OK;
}

int gptq_forward_ex(const gptq_layer_t* L, const void* x, void* out, int M, void* ws, size_t ws_bytes, void* stream,
                    const gptq_tuning_t* tune) {
    if (int rc = check_align(x, out, ws)) return rc;
    return forward_impl(L, x, out, M, split_ws(ws, ws_bytes), stream, tune);
}

size_t gptq_workspace_bytes_multi(const gptq_layer_t* const* layers, int n_layers, int M) {
    return gptq_workspace_bytes_multi_ex(layers, n_layers, M, nullptr);
}

// Batched decode of 2..4 layers sharing x in ONE gemm_stream64_kernel launch: by the planner's measured preference, or forced
// with tuning.path = 3 and tuning.reserved[2] = 4.
static bool want_stream64_multi(const gptq_layer_t* const* layers, int n, int M, const gptq_tuning_t* t, Stream64Plan* plan_out) {
    if (n < 2 || n > 4 || M > 64) return false;
    const bool forced = t && t->path == 3 && t->reserved[2] == 4;
    if (t && t->path != 0 && !forced) return false;
    if (M <= 2 && !forced) return false;                         // up to 2 rows: the streamed GEMV (or layer by layer)
    const Stream64Plan& sp = *plan_out = plan_stream64(layers, n, M, t);
    // 3..4 rows: only one unsplit round of 16-wave workgroups beats the streamed GEMV (tools/misc_bench.py, us, GEMV at M = 4 against this kernel
    // at M = 8: q|k|v, 192 strips: 12.0 against 11.2; gate|up, 344 strips in 8-wave workgroups: 17.5 against 18.8)
    if (M <= 4 && !forced && !(sp.ok && sp.ksplit == 1 && sp.strips_total <= 256)) return false;
    return sp.ok && (sp.pays || forced);
}

// 17 .. 128 rows, 2..4 layers sharing x in ONE gemm_mid_kernel launch: by the planner's measured preference, or forced with tuning.path = 3 and
// tuning.reserved[2] = 5.
static bool want_mid_multi(const gptq_layer_t* const* layers, int n, int M, const gptq_tuning_t* t, MidPlan* plan_out) {
    if (n < 2 || n > 4 || M > 256) return false;
    const bool forced = t && t->path == 3 && t->reserved[2] == 5;
    if (t && t->path != 0 && !forced) return false;
    const MidPlan& mp = *plan_out = plan_mid(layers, n, M, t);
    return mp.ok && (mp.pays || forced);
}

// 33+ rows of a group whose weights are mostly (>= 3/4) in layers the panel kernel takes with well-filled rounds: the layers run ONE BY ONE -- the multi-layer
// forms of the rows / mid / stream64 kernels were fitted before that kernel existed and lose to it (tools/multi_rows_sweep.py, profiles/r06_multi_rows_sweep.log, group
// call -> one by one: 8B gate|up at 64 rows 45.7 -> 32.8 us, 70B q|k|v at 128 rows 59.5 -> 46.9, 70B TP8 gate|up at 128 rows 42.0 -> 37.9; 13B q|k|v at 128 rows --
// 160 tiles of 256 per layer -- keeps its group launch: 45.0 against 52.8)
static bool separate_panels_pay(const gptq_layer_t* const* layers, int n, int M) {
    if (n < 2 || M < 33) return false;
    size_t all = 0, paneled = 0;
    for (int i = 0; i < n; ++i) {
        const size_t kn = (size_t)layers[i]->K * layers[i]->N;
        all += kn;
        if (layers[i]->epilogue == GPTQ_EPI_NONE && route_forward(layers[i], M, nullptr).kind == ROUTE_GEMM && panel_pays_filled(*layers[i], M)) paneled += kn;      // (33+ rows: the GEMM step is the first that can hit)
    }
    return paneled * 4 >= all * 3;
}

// ---- the route of one layer-group call: to gptq_forward_multi_ex and gptq_workspace_bytes_multi_ex what route_forward is to the single-layer entry points ----
enum MultiKind {
    MULTI_TILED,          // ONE decode-copy launch over the strips of all layers (tp)
    MULTI_ROWS,           // ONE gemm_rows.hip launch over the strip groups of all layers (rp); act-order layers of one order read one permuted x
    MULTI_MID,            // ONE gemm_mid_kernel launch (mp)
    MULTI_STREAM64,       // ONE gemm_stream64_kernel launch (s64)
    MULTI_STREAM,         // ONE streamed-GEMV launch (sp)
    MULTI_SHARED_PERM,    // a GEMM per layer (pls) behind ONE permuted x -- where the workspace that is passed fits every plan, else one by one
    MULTI_ONE_BY_ONE,     // gptq_forward per layer
};
struct MultiRoute {
    MultiKind kind;
    int declined = 0;     // a forced route the group does not fit (multi_decline): tuning.path 8 / 6, or reserved[2] = 4 / 5 of path 3; the query answers with the rest of the ladder
    TiledPlan tp; RowsPlan rp; MidPlan mp; Stream64Plan s64; StreamPlan sp; GemmPlan pls[4];      // the sub-plan(s) of `kind`
    size_t body = 0;      // bytes behind the ticket header (MULTI_SHARED_PERM / MULTI_ONE_BY_ONE: every layer's own query)
    bool hit(MultiKind k, size_t need) { kind = k; body = need; return true; }
};
static MultiRoute route_forward_multi(const gptq_layer_t* const* layers, int n_layers, int M, const gptq_tuning_t* tune) {
    MultiRoute r;
    // decode rows on layers that carry the decode copy: one launch over the strips of all layers (tools/tiled_sweep.py, M = 4, us: q|k|v 8.6 against
    // 11.1 for the batched-decode kernel, gate|up 12.9 against 18.9)
    // (no byte cap on the group for this kernel -- multi_preferred's 128 MB was measured on the round-2 kernels: 70B gate|up, 235 MB, M = 1 / 4 one by one
    // 48.5 / 57.3 us, ONE decode-copy launch 42.2 / 50.9: profiles/r06_multi_geom_sweep.log)
    if (want_tiled(layers, n_layers, M, tune, &r.tp) && (n_layers >= 2 || (tune && tune->path == 8)) && r.hit(MULTI_TILED, r.tp.partial_bytes)) return r;
    if (tune && tune->path == 8) r.declined = 8;
    // 5 .. 128 rows on layers that carry the decode copy: the exchange-free kernel over the strip groups of all layers (gemm_rows.hip); act-order layers of
    // ONE order (the same perm pointer: QuantLinear.share_act_order) read one permuted x -- and nothing else is staged
    const bool rows_forced = tune && tune->path == 3 && tune->reserved[3] == GPTQ_LAB_VARIANT_ROWS_ON && rows_multi_ok(layers, n_layers, M);      // lab knob 50
    // (a group with a flagged 2-bit layer in the band where that layer runs on its copy: layer by layer too -- the low-bit forms have no group launch)
    bool lowbit_single = false;
    for (int i = 0; !tune && i < n_layers; ++i) lowbit_single = lowbit_single || (layers[i]->epilogue == GPTQ_EPI_NONE && dense_int2_choice(*layers[i], M) != 0);
    const bool separate = !tune && (lowbit_single || separate_panels_pay(layers, n_layers, M));
    if (n_layers >= 2 && (rows_forced || (!tune && !separate && rows_multi_pays(layers, n_layers, M))) && (r.rp = plan_rows_multi(layers, n_layers, M, nullptr)).ok &&
        r.hit(MULTI_ROWS, layers[0]->g_idx ? xperm16_bytes(layers[0], M) : 0))
        return r;
    if (!separate && want_mid_multi(layers, n_layers, M, tune, &r.mp) && r.hit(MULTI_MID, r.mp.partial_bytes)) return r;
    if (!separate && want_stream64_multi(layers, n_layers, M, tune, &r.s64) && r.hit(MULTI_STREAM64, r.s64.partial_bytes)) return r;
    if (n_layers <= 4 && M <= 4) {
        if ((r.sp = plan_stream(layers, n_layers, M, tune)).ok && multi_preferred(layers, n_layers, M) && r.hit(MULTI_STREAM, r.sp.partial_bytes)) return r;
        if (tune && tune->path == 6) r.declined = 6;
    }
    if (tune && tune->path == 3 && (tune->reserved[2] == 4 || tune->reserved[2] == 5)) r.declined = tune->reserved[2];
    // Act-order layers that share ONE perm -- q / k / v and gate / up of a GPTQ checkpoint do: the activation order comes from the Hessian of the
    // layers' common input (the reference's fused q/k/v caller relies on it: fused_llama_attn.py:188 hands the kernels q_proj's order for all three) --
    // read ONE permuted x: the first layer's GEMM call permutes into the head of the workspace, the others find it there.  The caller says so by
    // passing the same `perm` pointer (QuantLinear.share_act_order / forward_multi do that once the g_idx tensors compared equal).
    bool shared = n_layers >= 2 && n_layers <= 4 && !tune && layers[0]->perm && layers[0]->qweight_seq && layers[0]->g_idx;
    for (int i = 0; shared && i < n_layers; ++i) {
        const gptq_layer_t* L = layers[i];
        const GemmPlan& pl = r.pls[i];
        shared = L->perm == layers[0]->perm && L->qweight_seq && L->g_idx && L->epilogue == GPTQ_EPI_NONE && L->K == layers[0]->K &&
                 L->dtype == layers[0]->dtype && L->dtype != GPTQ_F32 && want_gemm(L, M, nullptr, &r.pls[i]) &&
                 pl.supported && pl.use_seq && pl.kernel != GEMM_F32 && pl.xslot == r.pls[0].xslot && pl.xnat == r.pls[0].xnat && pl.xperm_bytes == r.pls[0].xperm_bytes;
    }
    r.kind = shared ? MULTI_SHARED_PERM : MULTI_ONE_BY_ONE;      // one by one: anything the one-launch kernels do not cover, the same result layer by layer
    return r;
}
static int multi_decline(const MultiRoute& r) {
    switch (r.declined) {
        case 8: return fail(GPTQ_ERR_UNSUPPORTED, "tuning.path = 8: these layers do not fit one decode-copy launch (1..4 layers of one packing with qweight_tiled, all plain or all act-order, M <= 8)");
        case 6: return fail(GPTQ_ERR_UNSUPPORTED, "tuning.path = 6: these layers / this launch shape do not fit the streamed GEMV");
        case 4: return fail(GPTQ_ERR_UNSUPPORTED, "tuning.path = 3 / reserved[2] = 4: these layers do not fit one batched-decode launch (2..4 plain 4-bit layers, M <= 64)");
        default: return fail(GPTQ_ERR_UNSUPPORTED, "tuning.path = 3 / reserved[2] = 5: these layers do not fit one gemm_mid_kernel launch (2..4 plain 4-bit layers, N %% 64 == 0, M <= 256)");
    }
}

size_t gptq_workspace_bytes_multi_ex(const gptq_layer_t* const* layers, int n_layers, int M, const gptq_tuning_t* tune) {
    if (!layers || n_layers <= 0 || M <= 0) return 0;
    for (int i = 0; i < n_layers; ++i)
        if (check_layer(layers[i]) != GPTQ_OK) return 0;
    const MultiRoute r = route_forward_multi(layers, n_layers, M, tune);
    if (r.kind != MULTI_SHARED_PERM && r.kind != MULTI_ONE_BY_ONE) return r.body ? WS_HEADER_BYTES + r.body : 0;
    size_t need = 0;
    for (int i = 0; i < n_layers; ++i) need = std::max(need, gptq_workspace_bytes_ex(layers[i], M, nullptr));
    return need;
}

int gptq_forward_multi(const gptq_layer_t* const* layers, int n_layers, const void* x, void* const* outs, int M, void* ws,
                       size_t ws_bytes, void* stream) {
    return gptq_forward_multi_ex(layers, n_layers, x, outs, M, ws, ws_bytes, stream, nullptr);
}

static int forward_multi_core(const gptq_layer_t* const* layers, int n_layers, const void* x, void* const* outs, int M, const WsView& wv,
                              void* stream, const gptq_tuning_t* tune) {
    if (!layers || !outs) return fail(GPTQ_ERR_NULL, "layers/outs must be non-NULL");
    if (n_layers <= 0) return fail(GPTQ_ERR_SHAPE, "n_layers must be > 0, got %d", n_layers);
    for (int i = 0; i < n_layers; ++i) {
        int rc = check_layer(layers[i]);
        if (rc) return rc;
        rc = check_io(x, outs[i], M);
        if (rc) return rc;
        if (layers[i]->K != layers[0]->K) return fail(GPTQ_ERR_SHAPE, "layers of one gptq_forward_multi call read the same x: in_features %d != %d", layers[i]->K, layers[0]->K);
        if (layers[i]->dtype != layers[0]->dtype) return fail(GPTQ_ERR_UNSUPPORTED, "layers of one gptq_forward_multi call share the dtype of x");
    }
    const MultiRoute r = route_forward_multi(layers, n_layers, M, tune);
    if (r.declined) return multi_decline(r);
    if (r.kind == MULTI_ROWS || r.kind == MULTI_MID || r.kind == MULTI_STREAM64)
        if (int rc = need_body(wv, r.body)) return rc;
    hipError_t e;
    switch (r.kind) {
        case MULTI_TILED: return tiled_call(layers, n_layers, r.tp, x, outs, M, wv, stream);
        case MULTI_ROWS: {
            const void* xin = x;
            if (layers[0]->g_idx) {
                e = launch_permute_rows16(x, layers[0]->perm, M, layers[0]->K, wv.body, (hipStream_t)stream, false);
                if (e != hipSuccess) return hip_fail(e, "gptq x permute launch");
                xin = wv.body;
            }
            e = launch_gemm_rows_multi(layers, n_layers, r.rp, xin, outs, M, (hipStream_t)stream);
            if (e != hipSuccess) return hip_fail(e, "gptq batched-decode launch (gemm_rows; was gptq_init() called on this device?)");
            return GPTQ_OK;
        }
        case MULTI_MID:
            e = launch_mid(layers, r.mp, x, outs, M, wv.header, wv.body, nullptr, (hipStream_t)stream);
            if (e != hipSuccess) return hip_fail(e, "gptq 17..128-row launch (needs > 64 KiB of LDS: was gptq_init() called on this device?)");
            return GPTQ_OK;
        case MULTI_STREAM64:
            e = launch_stream64(layers, r.s64, x, outs, M, wv.header, wv.body, nullptr, (hipStream_t)stream);
            if (e != hipSuccess) return hip_fail(e, "gptq batched-decode launch (needs > 64 KiB of LDS: was gptq_init() called on this device?)");
            return GPTQ_OK;
        case MULTI_STREAM: return stream_call(layers, n_layers, r.sp, x, outs, M, wv, stream);
        case MULTI_SHARED_PERM: {
            bool fits = true;
            for (int i = 0; i < n_layers; ++i) fits = fits && r.pls[i].workspace_bytes <= wv.body_bytes;
            if (!fits) break;
            for (int i = 0; i < n_layers; ++i) {
                e = launch_gemm(*layers[i], r.pls[i], x, outs[i], M, wv.header, wv.body, (hipStream_t)stream, i > 0);
                if (e != hipSuccess) return hip_fail(e, "gptq_gemm launch (shared permuted x)");
            }
            return GPTQ_OK;
        }
        case MULTI_ONE_BY_ONE: break;
    }
    for (int i = 0; i < n_layers; ++i) {
        int rc = forward_impl(layers[i], x, outs[i], M, wv, stream, nullptr);
        if (rc) return rc;
    }
    return GPTQ_OK;
}

int gptq_forward_multi_ex(const gptq_layer_t* const* layers, int n_layers, const void* x, void* const* outs, int M, void* ws,
                          size_t ws_bytes, void* stream, const gptq_tuning_t* tune) {
    if (int rc = check_align(x, nullptr, ws)) return rc;
    for (int i = 0; outs && i < n_layers; ++i)
        if ((uintptr_t)outs[i] & 15) return fail(GPTQ_ERR_UNSUPPORTED, "outs[%d] must be 16-byte aligned", i);
    return forward_multi_core(layers, n_layers, x, outs, M, split_ws(ws, ws_bytes), stream, tune);
}

// ---- fused gated MLP (mlp.hip) -----------------------------------------------------------------------------------------
static int check_mlp(const gptq_layer_t* gate, const gptq_layer_t* up, const gptq_layer_t* down) {
    int rc = check_layer(gate);
    if (rc) return rc;
    if ((rc = check_layer(up))) return rc;
    if ((rc = check_layer(down))) return rc;
    if (gate->K != up->K || gate->N != up->N)
        return fail(GPTQ_ERR_SHAPE, "gate (%d -> %d) and up (%d -> %d) must have the same shape", gate->K, gate->N, up->K, up->N);
    if (down->K != gate->N)
        return fail(GPTQ_ERR_SHAPE, "down reads the intermediate activation: its in_features (%d) must be gate's out_features (%d)", down->K, gate->N);
    if (gate->dtype != up->dtype || gate->dtype != down->dtype) return fail(GPTQ_ERR_UNSUPPORTED, "the three layers of an MLP share the dtype of x");
    if (gate->epilogue != GPTQ_EPI_NONE || up->epilogue != GPTQ_EPI_NONE || down->epilogue != GPTQ_EPI_NONE)
        return fail(GPTQ_ERR_UNSUPPORTED, "gptq_mlp_forward takes plain layers (the SiLU * mul is its own)");
    return GPTQ_OK;
}
static size_t mlp_stage_bytes(const gptq_layer_t* gate, int M) { return ((size_t)M * gate->N * dtype_size(gate->dtype) + 255) / 256 * 256; }

size_t gptq_workspace_bytes_mlp(const gptq_layer_t* gate, const gptq_layer_t* up, const gptq_layer_t* down, int M) {
    return gptq_workspace_bytes_mlp_ex(gate, up, down, M, nullptr);
}

size_t gptq_workspace_bytes_mlp_ex(const gptq_layer_t* gate, const gptq_layer_t* up, const gptq_layer_t* down, int M, const gptq_tuning_t* tune) {
    (void)tune;
    if (check_mlp(gate, up, down) != GPTQ_OK || M <= 0) return 0;
    const gptq_layer_t* gu[2] = {gate, up};
    size_t inner = gptq_workspace_bytes_multi_ex(gu, 2, M, nullptr);
    inner = std::max(inner, gptq_workspace_bytes_ex(down, M, nullptr));
    inner = inner > WS_HEADER_BYTES ? inner - WS_HEADER_BYTES : 0;
    return WS_HEADER_BYTES + 2 * mlp_stage_bytes(gate, M) + inner;
}

// down of gptq_mlp_forward: does its call at M rows run an MFMA GEMM that reads x permuted in NATURAL order of its re-sequenced rows (GemmPlan.xnat)?  Then the
// SiLU * mul pass writes that permuted x itself.  (Decode rows gather inside the kernel, fp32 and the checkpoint-row kernels have their own orders: unchanged.)
// r: route_forward(down, M, nullptr) -- the GEMM plan the fused pass feeds is r.gp
static bool mlp_fused_permute(const gptq_layer_t* down, int M, const gptq_tuning_t* tune, const ForwardRoute& r) {
    if (tune && tune->reserved[3] == GPTQ_LAB_VARIANT_MLP_TWO_PASSES) return false;      // lab (bench.py: the two passes of round 5, interleaved with the default)
    if (!down->g_idx || !down->perm || !down->qweight_seq || down->epilogue != GPTQ_EPI_NONE) return false;
    if (!silu_mul2_permute_ok(down->K, down->dtype)) return false;
    const GemmPlan& pl = r.gp;
    return r.kind == ROUTE_GEMM && pl.supported && pl.use_seq && pl.xnat && pl.kernel != GEMM_F32 && pl.xperm_bytes > 0;
}

int gptq_mlp_forward(const gptq_layer_t* gate, const gptq_layer_t* up, const gptq_layer_t* down, const void* x, void* out, int M,
                     void* ws, size_t ws_bytes, void* stream) {
    return gptq_mlp_forward_act(gate, up, down, GPTQ_EPI_SILU_MUL, x, out, M, ws, ws_bytes, stream);
}

static int mlp_forward_core(const gptq_layer_t* gate, const gptq_layer_t* up, const gptq_layer_t* down, int act, const void* x, void* out, int M,
                            void* ws, size_t ws_bytes, void* stream, const gptq_tuning_t* tune);

int gptq_mlp_forward_act(const gptq_layer_t* gate, const gptq_layer_t* up, const gptq_layer_t* down, int act, const void* x, void* out, int M,
                         void* ws, size_t ws_bytes, void* stream) {
    return mlp_forward_core(gate, up, down, act, x, out, M, ws, ws_bytes, stream, nullptr);
}

// (tuning: only the lab variant of reserved[3] and the refusal of a path override; without one this is gptq_mlp_forward_act)
int gptq_mlp_forward_ex(const gptq_layer_t* gate, const gptq_layer_t* up, const gptq_layer_t* down, const void* x, void* out, int M,
                        void* ws, size_t ws_bytes, void* stream, const gptq_tuning_t* tune) {
    if (!tune) return gptq_mlp_forward_act(gate, up, down, GPTQ_EPI_SILU_MUL, x, out, M, ws, ws_bytes, stream);
    return mlp_forward_core(gate, up, down, GPTQ_EPI_SILU_MUL, x, out, M, ws, ws_bytes, stream, tune);
}

static int mlp_forward_core(const gptq_layer_t* gate, const gptq_layer_t* up, const gptq_layer_t* down, int act, const void* x, void* out, int M,
                            void* ws, size_t ws_bytes, void* stream, const gptq_tuning_t* tune) {
    if (!is_gated(act)) return fail(GPTQ_ERR_UNSUPPORTED, "gptq_mlp_forward_act: act must be GPTQ_EPI_SILU_MUL (1) or GPTQ_EPI_GELU_TANH_MUL (2), got %d", act);
    int rc = check_mlp(gate, up, down);
    if (rc) return rc;
    if ((rc = check_io(x, out, M))) return rc;
    if ((rc = check_align(x, out, ws))) return rc;
    const WsView wv = split_ws(ws, ws_bytes);
    const size_t have = wv.header ? WS_HEADER_BYTES + wv.body_bytes : (size_t)0;
    if (tune && tune->path != 0)
        return fail(GPTQ_ERR_UNSUPPORTED, "gptq_mlp_forward_ex takes no path override (tuning.path = %d): the one-launch persistent kernel of round 3 is a lab now "
                                          "(tools/lab/mlp_ring.hip), not part of this library", tune->path);
    // Three steps -- gate and up through the multi-layer entry point (ONE launch for decode rows) into two staging buffers at the front of the body,
    // SiLU * mul in place, down -- each inner call on the ONE ticket header and the body behind the staging buffers.
    const size_t sb = mlp_stage_bytes(gate, M);
    if (wv.body_bytes < 2 * sb)
        return fail(GPTQ_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", gptq_workspace_bytes_mlp_ex(gate, up, down, M, tune), have);
    void* hg = wv.body;
    void* hu = (char*)wv.body + sb;
    const WsView inner{wv.header, (char*)wv.body + 2 * sb, wv.body_bytes - 2 * sb};
    const gptq_layer_t* gu[2] = {gate, up};
    void* outs[2] = {hg, hu};
    if ((rc = forward_multi_core(gu, 2, x, outs, M, inner, stream, nullptr))) return rc;
    // An act-order `down` whose kernel reads x permuted in natural order (the decode-copy GEMMs: panel / rows / stream-K / wide tiles): SiLU * mul and that
    // permute are ONE pass into the spot down's own pre-pass would have filled (round 6; the reference's fused MLP, fused_llama_mlp.py:131-306)
    const ForwardRoute rd = route_forward(down, M, nullptr);
    if (mlp_fused_permute(down, M, tune, rd)) {
        const GemmPlan& pl = rd.gp;
        if (pl.workspace_bytes > inner.body_bytes)
            return fail(GPTQ_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", gptq_workspace_bytes_mlp_ex(gate, up, down, M, tune), have);
        hipError_t e = launch_silu_mul2_permute(hg, hu, down->perm, M, down->K, down->dtype, act, inner.body, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "silu_mul + permute launch (was gptq_init() called on this device?)");
        e = launch_gemm(*down, pl, inner.body, out, M, inner.header, inner.body, (hipStream_t)stream, /*x_permuted=*/true);
        if (e != hipSuccess) return hip_fail(e, "gptq_gemm launch (down projection of gptq_mlp_forward)");
        return GPTQ_OK;
    }
    hipError_t e = launch_silu_mul2(hg, hu, hg, (size_t)M * gate->N, gate->dtype, act, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "silu_mul launch");
    return forward_routed(rd, down, hg, out, M, inner, stream, nullptr);      // (check_mlp: down has no epilogue)
}

int gptq_describe_mlp_plan(const gptq_layer_t* gate, const gptq_layer_t* up, const gptq_layer_t* down, int M, const gptq_tuning_t* tune, char* out,
                           size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out must be non-NULL");
    out[0] = 0;
    int rc = check_mlp(gate, up, down);
    if (rc) return rc;
    if (M <= 0) return fail(GPTQ_ERR_SHAPE, "M must be > 0, got %d", M);
    const ForwardRoute rd = route_forward(down, M, nullptr);
    if (mlp_fused_permute(down, M, tune, rd)) snprintf(out, out_bytes, "kernel=unfused launches=3 steps=forward_multi(gate,up)|silu_mul+permute|gemm(down) down_permute=fused");
    else {
        const char* dp = !down->g_idx ? "none" : (rd.kind == ROUTE_TILED ? "in_kernel" : "own_pass");      // (decode rows: the decode kernel gathers x through perm itself)
        snprintf(out, out_bytes, "kernel=unfused launches=3+ steps=forward_multi(gate,up)|silu_mul|forward(down) down_permute=%s", dp);
    }
    return GPTQ_OK;
}

int gptq_forward(const gptq_layer_t* L, const void* x, void* out, int M, void* ws, size_t ws_bytes, void* stream) {
    return gptq_forward_ex(L, x, out, M, ws, ws_bytes, stream, nullptr);
}

int gptq_dequant(const gptq_layer_t* L, void* W_out, void* stream) {
    int rc = check_layer(L);
    if (rc) return rc;
    if (!W_out) return fail(GPTQ_ERR_NULL, "W_out is NULL");
    hipError_t e = launch_dequant(*L, W_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_dequant launch");
    return GPTQ_OK;
}

int gptq_grad_input(const gptq_layer_t* L, const void* dy, void* dx, int M, int accumulate, void* stream) {
    int rc = check_layer(L);
    if (rc) return rc;
    if ((rc = check_io(dy, dx, M))) return rc;
    if (((uintptr_t)dy | (uintptr_t)dx) & 15) return fail(GPTQ_ERR_UNSUPPORTED, "dy / dx must be 16-byte aligned");
    hipError_t e = launch_grad_input(*L, dy, dx, M, accumulate, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_grad_input launch");
    return GPTQ_OK;
}

// ---- the router of a routed layer (moe_router.hip) ----
static int router_check(int T, int H, int E, int topk, int dtype, int flags) {
    if (dtype == GPTQ_F32) return fail(GPTQ_ERR_UNSUPPORTED, "fp32 router: the router kernel takes fp16 / bf16");
    if (dtype != GPTQ_F16 && dtype != GPTQ_BF16) return fail(GPTQ_ERR_UNSUPPORTED, "unknown dtype enum %d", dtype);
    if (flags & ~GPTQ_ROUTER_RENORM) return fail(GPTQ_ERR_UNSUPPORTED, "unknown router flags 0x%x", flags);
    if (E < 1 || E > 256) return fail(GPTQ_ERR_UNSUPPORTED, "E = %d experts: the router kernel takes 1..256", E);
    if (topk < 1 || topk > 8 || topk > E) return fail(GPTQ_ERR_UNSUPPORTED, "topk = %d: the router kernel takes 1..min(E, 8) (E = %d)", topk, E);
    if (H <= 0 || H % 64) return fail(GPTQ_ERR_UNSUPPORTED, "H = %d must be a positive multiple of 64", H);
    if (T < 0) return fail(GPTQ_ERR_SHAPE, "T must be >= 0, got %d", T);
    const RouterPlan pl = plan_moe_router(T, H, E, topk, dtype);
    if (pl.lds_bytes > GPTQ_ROUTER_MAX_LDS) return fail(GPTQ_ERR_UNSUPPORTED, "H = %d: the staged row of x needs %zu bytes of LDS, more than %zu", H, pl.lds_bytes, GPTQ_ROUTER_MAX_LDS);
    return GPTQ_OK;
}

int gptq_moe_router(const void* x, const void* w, int T, int H, int E, int topk, int dtype, int flags, void* logits_out, int64_t* topk_idx, float* topk_w,
                    void* stream) {
    if (!x || !w || !topk_idx || !topk_w) return fail(GPTQ_ERR_NULL, "x / w / topk_idx / topk_w must be non-NULL");
    if (int rc = router_check(T, H, E, topk, dtype, flags)) return rc;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)logits_out | (uintptr_t)topk_idx | (uintptr_t)topk_w) & 15)
        return fail(GPTQ_ERR_UNSUPPORTED, "x / w / logits_out / topk_idx / topk_w must be 16-byte aligned");
    if (T == 0) return GPTQ_OK;
    hipError_t e = launch_moe_router(x, w, T, H, E, topk, dtype, flags & GPTQ_ROUTER_RENORM, logits_out, topk_idx, topk_w, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_moe_router launch");
    return GPTQ_OK;
}

int gptq_describe_moe_router_plan(int T, int H, int E, int topk, int dtype, int flags, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    if (router_check(T, H, E, topk, dtype, flags)) return describe_decline(out, out_bytes, "none");
    const RouterPlan pl = plan_moe_router(T, H, E, topk, dtype);
    snprintf(out, out_bytes, "path=router form=%s wg=%ld waves=8 lds=%zu launches=1", pl.rows ? "rows" : "tiles", pl.wg, pl.lds_bytes);
    return GPTQ_OK;
}

// ---- the grouped-sigmoid form of the router (DeepSeek-V3 / GLM-4 MoE) ----
static int router_grouped_check(int T, int H, int E, int topk, int n_group, int topk_group, float scale, int dtype, int flags) {
    if (dtype == GPTQ_F32) return fail(GPTQ_ERR_UNSUPPORTED, "fp32 router: the router kernel takes fp16 / bf16");
    if (dtype != GPTQ_F16 && dtype != GPTQ_BF16) return fail(GPTQ_ERR_UNSUPPORTED, "unknown dtype enum %d", dtype);
    if (flags & ~GPTQ_ROUTER_RENORM) return fail(GPTQ_ERR_UNSUPPORTED, "unknown router flags 0x%x", flags);
    if (E < 1 || E > 256) return fail(GPTQ_ERR_UNSUPPORTED, "E = %d experts: the router kernel takes 1..256", E);
    if (topk < 1 || topk > 8) return fail(GPTQ_ERR_UNSUPPORTED, "topk = %d: the router kernel takes 1..8", topk);
    if (n_group < 1 || n_group > 32) return fail(GPTQ_ERR_UNSUPPORTED, "n_group = %d: the grouped router takes 1..32 groups", n_group);
    if (topk_group < 1 || topk_group > n_group) return fail(GPTQ_ERR_UNSUPPORTED, "topk_group = %d: the grouped router takes 1..n_group (n_group = %d)", topk_group, n_group);
    if (E % n_group) return fail(GPTQ_ERR_UNSUPPORTED, "E = %d is not a multiple of n_group = %d", E, n_group);
    if (n_group > 1 && E / n_group < 2) return fail(GPTQ_ERR_UNSUPPORTED, "E / n_group = %d: a group's score is the sum of its two largest, so groups hold 2 experts or more", E / n_group);
    if (topk > topk_group * (E / n_group)) return fail(GPTQ_ERR_UNSUPPORTED, "topk = %d is more than the %d experts of the %d groups that stay", topk, topk_group * (E / n_group), topk_group);
    if (!(scale - scale == 0.f)) return fail(GPTQ_ERR_UNSUPPORTED, "scale must be finite");
    if (H <= 0 || H % 64) return fail(GPTQ_ERR_UNSUPPORTED, "H = %d must be a positive multiple of 64", H);
    if (T < 0) return fail(GPTQ_ERR_SHAPE, "T must be >= 0, got %d", T);
    const RouterPlan pl = plan_moe_router(T, H, E, topk, dtype);
    if (pl.lds_bytes > GPTQ_ROUTER_MAX_LDS) return fail(GPTQ_ERR_UNSUPPORTED, "H = %d: the staged row of x needs %zu bytes of LDS, more than %zu", H, pl.lds_bytes, GPTQ_ROUTER_MAX_LDS);
    return GPTQ_OK;
}

int gptq_moe_router_grouped(const void* x, const void* w, const float* bias, int T, int H, int E, int topk, int n_group, int topk_group, float scale, int dtype,
                            int flags, float* logits_out, float* scores_out, int64_t* topk_idx, float* topk_w, void* stream) {
    if (!x || !w || !topk_idx || !topk_w) return fail(GPTQ_ERR_NULL, "x / w / topk_idx / topk_w must be non-NULL");
    if (int rc = router_grouped_check(T, H, E, topk, n_group, topk_group, scale, dtype, flags)) return rc;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)logits_out | (uintptr_t)scores_out | (uintptr_t)topk_idx | (uintptr_t)topk_w) & 15)
        return fail(GPTQ_ERR_UNSUPPORTED, "x / w / logits_out / scores_out / topk_idx / topk_w must be 16-byte aligned");
    if ((uintptr_t)bias & 3) return fail(GPTQ_ERR_UNSUPPORTED, "bias must be 4-byte aligned");
    if (T == 0) return GPTQ_OK;
    hipError_t e = launch_moe_router_grouped(x, w, bias, T, H, E, topk, n_group, topk_group, scale, dtype, flags & GPTQ_ROUTER_RENORM, logits_out, scores_out,
                                             topk_idx, topk_w, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_moe_router_grouped launch");
    return GPTQ_OK;
}

int gptq_describe_moe_router_grouped_plan(int T, int H, int E, int topk, int n_group, int topk_group, int dtype, int flags, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    if (router_grouped_check(T, H, E, topk, n_group, topk_group, 1.f, dtype, flags)) return describe_decline(out, out_bytes, "none");
    const RouterPlan pl = plan_moe_router(T, H, E, topk, dtype);
    snprintf(out, out_bytes, "path=router_grouped form=%s wg=%ld waves=8 lds=%zu groups=%d launches=1", pl.rows ? "rows" : "tiles", pl.wg, pl.lds_bytes, n_group);
    return GPTQ_OK;
}

// ---- LoRA adapters (lora.hip) ----
static int lora_check(const gptq_lora_t* const* Ls, int n) {
    if (!Ls) return fail(GPTQ_ERR_NULL, "loras is NULL");
    if (n < 1 || n > GPTQ_LORA_MAX) return fail(GPTQ_ERR_UNSUPPORTED, "n = %d adapters: one call takes 1..%d", n, GPTQ_LORA_MAX);
    for (int i = 0; i < n; ++i) {
        const gptq_lora_t* L = Ls[i];
        if (!L) return fail(GPTQ_ERR_NULL, "loras[%d] is NULL", i);
        if (!L->A || !L->B) return fail(GPTQ_ERR_NULL, "loras[%d]: A/B must be non-NULL", i);
        if (L->dtype == GPTQ_F32) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: fp32 layer: the adapter kernels take fp16 / bf16", i);
        if (L->dtype != GPTQ_F16 && L->dtype != GPTQ_BF16) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: unknown dtype enum %d", i, L->dtype);
        if (L->r < 8 || L->r > 64 || L->r % 8) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: r = %d: the adapter kernels take r in 8, 16, .., 64", i, L->r);
        if (L->K <= 0 || L->K % 32) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: K = %d must be a positive multiple of 32", i, L->K);
        if (L->N <= 0 || L->N % 16) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: N = %d must be a positive multiple of 16", i, L->N);
        if (((uintptr_t)L->A | (uintptr_t)L->B) & 15) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: A / B must be 16-byte aligned", i);
        if (L->K != Ls[0]->K || L->dtype != Ls[0]->dtype) return fail(GPTQ_ERR_UNSUPPORTED, "the adapters of one call share K and dtype (adapter %d differs)", i);
    }
    return GPTQ_OK;
}

static int lora_check_ptrs(const void* const* ps, int n, const char* name) {
    if (!ps) return fail(GPTQ_ERR_NULL, "%s is NULL", name);
    for (int i = 0; i < n; ++i) {
        if (!ps[i]) return fail(GPTQ_ERR_NULL, "%s[%d] is NULL", name, i);
        if ((uintptr_t)ps[i] & 15) return fail(GPTQ_ERR_UNSUPPORTED, "%s[%d] must be 16-byte aligned", name, i);
    }
    return GPTQ_OK;
}

int gptq_lora_down(const gptq_lora_t* const* Ls, int n, const void* x, void* const* u, int M, void* stream) {
    if (int rc = lora_check(Ls, n)) return rc;
    if (!x) return fail(GPTQ_ERR_NULL, "x must be non-NULL");
    if ((uintptr_t)x & 15) return fail(GPTQ_ERR_UNSUPPORTED, "x must be 16-byte aligned");
    if (int rc = lora_check_ptrs((const void* const*)u, n, "u")) return rc;
    if (M < 0) return fail(GPTQ_ERR_SHAPE, "M must be >= 0, got %d", M);
    if (M == 0) return GPTQ_OK;
    hipError_t e = launch_lora_down(Ls, n, x, u, M, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_lora_down launch");
    return GPTQ_OK;
}

int gptq_lora_up(const gptq_lora_t* const* Ls, int n, const void* const* u, void* const* outs, int M, void* stream) {
    if (int rc = lora_check(Ls, n)) return rc;
    if (int rc = lora_check_ptrs(u, n, "u")) return rc;
    if (int rc = lora_check_ptrs((const void* const*)outs, n, "outs")) return rc;
    if (M < 0) return fail(GPTQ_ERR_SHAPE, "M must be >= 0, got %d", M);
    if (M == 0) return GPTQ_OK;
    hipError_t e = launch_lora_up(Ls, n, u, outs, M, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_lora_up launch");
    return GPTQ_OK;
}

int gptq_lora_apply(const gptq_lora_t* const* Ls, int n, const void* x, void* const* u, void* const* outs, int M, void* stream) {
    if (int rc = lora_check(Ls, n)) return rc;                 // everything is validated before the first launch
    if (!x) return fail(GPTQ_ERR_NULL, "x must be non-NULL");
    if ((uintptr_t)x & 15) return fail(GPTQ_ERR_UNSUPPORTED, "x must be 16-byte aligned");
    if (int rc = lora_check_ptrs((const void* const*)u, n, "u")) return rc;
    if (int rc = lora_check_ptrs((const void* const*)outs, n, "outs")) return rc;
    if (int rc = gptq_lora_down(Ls, n, x, u, M, stream)) return rc;
    return gptq_lora_up(Ls, n, (const void* const*)u, outs, M, stream);
}

int gptq_describe_lora_plan(const gptq_lora_t* const* Ls, int n, int M, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    int rc = lora_check(Ls, n);
    if (!rc && M < 0) rc = fail(GPTQ_ERR_SHAPE, "M must be >= 0, got %d", M);
    if (rc) return describe_decline(out, out_bytes, "none");
    const LoraPlan pl = plan_lora(Ls, n, M);
    snprintf(out, out_bytes, "path=lora rows=%s wg_down=%ld wg_up=%ld launches=2", pl.gemv ? "gemv" : "mfma", M ? pl.wg_down : 0L, M ? pl.wg_up : 0L);
    return GPTQ_OK;
}

// ---- the adapters' backward (lora.hip's kernels on the transposed copies + adapter_grad.hip) ----
static int lora_grad_check(const gptq_lora_t* const* Ls, int n) {     // as lora_check, but A / B are not read and N is a summed length
    if (!Ls) return fail(GPTQ_ERR_NULL, "loras is NULL");
    if (n < 1 || n > GPTQ_LORA_MAX) return fail(GPTQ_ERR_UNSUPPORTED, "n = %d adapters: one call takes 1..%d", n, GPTQ_LORA_MAX);
    for (int i = 0; i < n; ++i) {
        const gptq_lora_t* L = Ls[i];
        if (!L) return fail(GPTQ_ERR_NULL, "loras[%d] is NULL", i);
        if (L->dtype == GPTQ_F32) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: fp32 layer: the adapter kernels take fp16 / bf16", i);
        if (L->dtype != GPTQ_F16 && L->dtype != GPTQ_BF16) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: unknown dtype enum %d", i, L->dtype);
        if (L->r < 8 || L->r > 64 || L->r % 8) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: r = %d: the adapter kernels take r in 8, 16, .., 64", i, L->r);
        if (L->K <= 0 || L->K % 32) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: K = %d must be a positive multiple of 32", i, L->K);
        if (L->N <= 0 || L->N % 32) return fail(GPTQ_ERR_UNSUPPORTED, "loras[%d]: N = %d must be a positive multiple of 32 (the backward sums over N)", i, L->N);
        if (L->K != Ls[0]->K || L->dtype != Ls[0]->dtype) return fail(GPTQ_ERR_UNSUPPORTED, "the adapters of one call share K and dtype (adapter %d differs)", i);
    }
    return GPTQ_OK;
}

// the reused kernels' view of adapter L: down with A := Bt [r][N], K := N; up with B := At [K][r], N := K
static gptq_lora_t lora_grad_down_view(const gptq_lora_t& L, const void* Bt) {
    gptq_lora_t d = L;
    d.A = d.B = Bt;
    d.K = L.N;
    return d;
}
static gptq_lora_t lora_grad_up_view(const gptq_lora_t& L, const void* At) {
    gptq_lora_t d = L;
    d.A = d.B = At;
    d.N = L.K;
    return d;
}

size_t gptq_lora_backward_workspace_bytes(const gptq_lora_t* const* Ls, int n, int M) {
    if (lora_grad_check(Ls, n) || M < 0) return 0;
    return plan_wgrad(Ls, nullptr, n, M).bytes;
}

int gptq_lora_backward(const gptq_lora_t* const* Ls, const gptq_lora_grad_t* const* Gs, int n, const void* x, void* dX, int M, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (int rc = lora_grad_check(Ls, n)) return rc;              // everything is validated before the first launch
    if (!Gs) return fail(GPTQ_ERR_NULL, "grads is NULL");
    if (!x) return fail(GPTQ_ERR_NULL, "x must be non-NULL");
    uintptr_t bits = (uintptr_t)x | (uintptr_t)dX | (uintptr_t)workspace;
    for (int i = 0; i < n; ++i) {
        const gptq_lora_grad_t* G = Gs[i];
        if (!G) return fail(GPTQ_ERR_NULL, "grads[%d] is NULL", i);
        if (!G->At || !G->Bt || !G->u || !G->dY || !G->du) return fail(GPTQ_ERR_NULL, "grads[%d]: At / Bt / u / dY / du must be non-NULL", i);
        bits |= (uintptr_t)G->At | (uintptr_t)G->Bt | (uintptr_t)G->u | (uintptr_t)G->dY | (uintptr_t)G->du | (uintptr_t)G->dA | (uintptr_t)G->dB;
    }
    if (bits & 15) return fail(GPTQ_ERR_UNSUPPORTED, "x, dX, the workspace and every pointer of grads[] must be 16-byte aligned");
    if (M < 0) return fail(GPTQ_ERR_SHAPE, "M must be >= 0, got %d", M);
    if (M == 0) return GPTQ_OK;
    const WgradPlan pl = plan_wgrad(Ls, Gs, n, M);
    if (pl.bytes && (!workspace || workspace_bytes < pl.bytes))
        return fail(GPTQ_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", pl.bytes, workspace ? workspace_bytes : (size_t)0);
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < n; ++i) {                                   // 1. du_i: each adapter has its own dY, so a launch each
        const gptq_lora_t d = lora_grad_down_view(*Ls[i], Gs[i]->Bt);
        const gptq_lora_t* dp = &d;
        void* du = Gs[i]->du;
        hipError_t e = launch_lora_down(&dp, 1, Gs[i]->dY, &du, M, st);
        if (e != hipSuccess) return hip_fail(e, "gptq_lora_backward du launch");
    }
    hipError_t e = launch_wgrad(Ls, Gs, n, x, M, pl, (char*)workspace, st);   // 2. + 3.
    if (e != hipSuccess) return hip_fail(e, "gptq_lora_backward wgrad launch");
    if (dX) {
        for (int i = 0; i < n; ++i) {                               // 4. one shared dX: read-modify-write, so in index order
            const gptq_lora_t d = lora_grad_up_view(*Ls[i], Gs[i]->At);
            const gptq_lora_t* dp = &d;
            const void* du = Gs[i]->du;
            e = launch_lora_up(&dp, 1, &du, &dX, M, st);
            if (e != hipSuccess) return hip_fail(e, "gptq_lora_backward dX launch");
        }
    }
    return GPTQ_OK;
}

int gptq_describe_lora_backward_plan(const gptq_lora_t* const* Ls, int n, int M, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    int rc = lora_grad_check(Ls, n);
    if (!rc && M < 0) rc = fail(GPTQ_ERR_SHAPE, "M must be >= 0, got %d", M);
    if (rc) return describe_decline(out, out_bytes, "none");
    const WgradPlan pl = plan_wgrad(Ls, nullptr, n, M);
    long wg_down = 0, wg_up = 0;
    char sa[64] = "", sb[64] = "";
    bool sliced = false;
    for (int i = 0; i < n; ++i) {
        const gptq_lora_t d = lora_grad_down_view(*Ls[i], nullptr), u = lora_grad_up_view(*Ls[i], nullptr);
        const gptq_lora_t *dp = &d, *up = &u;
        if (M) {
            wg_down += plan_lora(&dp, 1, M).wg_down;
            wg_up += plan_lora(&up, 1, M).wg_up;
        }
        const int a = wgrad_slices(M, Ls[i]->r, Ls[i]->K).S, b = wgrad_slices(M, Ls[i]->N, Ls[i]->r).S;
        sliced = sliced || a > 1 || b > 1;
        snprintf(sa + strlen(sa), sizeof(sa) - strlen(sa), "%s%d", i ? "," : "", a);
        snprintf(sb + strlen(sb), sizeof(sb) - strlen(sb), "%s%d", i ? "," : "", b);
    }
    snprintf(out, out_bytes, "path=lora_backward S_dA=%s S_dB=%s wg_down=%ld wg_wgrad=%ld wg_sum=%ld wg_up=%ld workspace=%zu launches=%d", sa, sb, wg_down,
             pl.wg_wgrad, pl.wg_sum, wg_up, pl.bytes, M ? 2 * n + 1 + (sliced ? 1 : 0) : 0);
    return GPTQ_OK;
}

// ---- per-row adapter banks (adapter_rows.hip) ----
static int adapter_check_slots(int slots) {
    if (slots < 1 || slots > GPTQ_ADAPTER_MAX_SLOTS)
        return fail(GPTQ_ERR_UNSUPPORTED, "slots = %d: a bank holds 1..%d adapters (the routing kernel's tables)", slots, GPTQ_ADAPTER_MAX_SLOTS);
    return GPTQ_OK;
}

static int adapter_check(const gptq_adapter_bank_t* const* Bs, int n) {
    if (!Bs) return fail(GPTQ_ERR_NULL, "banks is NULL");
    if (n < 1 || n > GPTQ_LORA_MAX) return fail(GPTQ_ERR_UNSUPPORTED, "n = %d banks: one call takes 1..%d", n, GPTQ_LORA_MAX);
    for (int i = 0; i < n; ++i) {
        const gptq_adapter_bank_t* L = Bs[i];
        if (!L) return fail(GPTQ_ERR_NULL, "banks[%d] is NULL", i);
        if (!L->A || !L->B || !L->scales) return fail(GPTQ_ERR_NULL, "banks[%d]: A / B / scales must be non-NULL", i);
        if (L->dtype == GPTQ_F32) return fail(GPTQ_ERR_UNSUPPORTED, "banks[%d]: fp32 layer: the adapter kernels take fp16 / bf16", i);
        if (L->dtype != GPTQ_F16 && L->dtype != GPTQ_BF16) return fail(GPTQ_ERR_UNSUPPORTED, "banks[%d]: unknown dtype enum %d", i, L->dtype);
        if (L->r < 8 || L->r > 64 || L->r % 8) return fail(GPTQ_ERR_UNSUPPORTED, "banks[%d]: r = %d: the adapter kernels take r in 8, 16, .., 64", i, L->r);
        if (L->K <= 0 || L->K % 32) return fail(GPTQ_ERR_UNSUPPORTED, "banks[%d]: K = %d must be a positive multiple of 32", i, L->K);
        if (L->N <= 0 || L->N % 16) return fail(GPTQ_ERR_UNSUPPORTED, "banks[%d]: N = %d must be a positive multiple of 16", i, L->N);
        if (int rc = adapter_check_slots(L->slots)) return rc;
        if (((uintptr_t)L->A | (uintptr_t)L->B) & 15) return fail(GPTQ_ERR_UNSUPPORTED, "banks[%d]: A / B must be 16-byte aligned", i);
        if ((uintptr_t)L->scales & 3) return fail(GPTQ_ERR_UNSUPPORTED, "banks[%d]: scales must be 4-byte aligned", i);
        if (L->K != Bs[0]->K || L->dtype != Bs[0]->dtype || L->slots != Bs[0]->slots)
            return fail(GPTQ_ERR_UNSUPPORTED, "the banks of one call share K, dtype and slots (bank %d differs)", i);
    }
    return GPTQ_OK;
}

size_t gptq_adapter_route_bytes(int M, int slots) {
    if (M < 0 || slots < 1 || slots > GPTQ_ADAPTER_MAX_SLOTS) return 0;
    return plan_adapter_route(M, slots).bytes;
}

int gptq_adapter_route(const int64_t* ids, int M, int slots, void* route, size_t route_bytes, void* stream) {
    if (int rc = adapter_check_slots(slots)) return rc;
    if (M < 0) return fail(GPTQ_ERR_SHAPE, "M must be >= 0, got %d", M);
    if (M == 0) return GPTQ_OK;
    if (!ids || !route) return fail(GPTQ_ERR_NULL, "ids / route must be non-NULL");
    if ((uintptr_t)ids & 7) return fail(GPTQ_ERR_UNSUPPORTED, "ids must be 8-byte aligned");
    if ((uintptr_t)route & 15) return fail(GPTQ_ERR_UNSUPPORTED, "route must be 16-byte aligned");
    const size_t need = plan_adapter_route(M, slots).bytes;
    if (route_bytes < need)
        return fail(GPTQ_ERR_UNSUPPORTED, "route_bytes = %zu is too small: M = %d rows over %d slots need %zu", route_bytes, M, slots, need);
    hipError_t e = launch_adapter_route(ids, M, slots, (char*)route, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_adapter_route launch");
    return GPTQ_OK;
}

int gptq_adapter_rows_apply(const gptq_adapter_bank_t* const* Bs, int n, const void* x, void* const* u, void* const* outs, const void* route, int M,
                            void* stream) {
    if (int rc = adapter_check(Bs, n)) return rc;                // everything is validated before the first launch
    if (M < 0) return fail(GPTQ_ERR_SHAPE, "M must be >= 0, got %d", M);
    if (M == 0) return GPTQ_OK;
    if (!x || !route) return fail(GPTQ_ERR_NULL, "x / route must be non-NULL");
    if ((uintptr_t)x & 15) return fail(GPTQ_ERR_UNSUPPORTED, "x must be 16-byte aligned");
    if ((uintptr_t)route & 15) return fail(GPTQ_ERR_UNSUPPORTED, "route must be 16-byte aligned");
    if (int rc = lora_check_ptrs((const void* const*)u, n, "u")) return rc;
    if (int rc = lora_check_ptrs((const void* const*)outs, n, "outs")) return rc;
    hipError_t e = launch_adapter_rows(Bs, n, x, u, outs, route, M, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_adapter_rows_apply launch");
    return GPTQ_OK;
}

int gptq_describe_adapter_rows_plan(const gptq_adapter_bank_t* const* Bs, int n, int M, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    int rc = adapter_check(Bs, n);
    if (!rc && M < 0) rc = fail(GPTQ_ERR_SHAPE, "M must be >= 0, got %d", M);
    if (rc) return describe_decline(out, out_bytes, "none");
    const AdapterRowsPlan pl = plan_adapter_rows(Bs, n, M);
    snprintf(out, out_bytes, "path=adapter_rows tiles=%ld wg_down=%ld wg_up=%ld launches=2", pl.tiles, pl.wg_down, pl.wg_up);
    return GPTQ_OK;
}

// ---- routed mixture-of-experts layers: the grouped path (moe.hip, moe_grad.hip) and the three paths on the experts' decode copy ----
// What the paths' checks differ in.  The grouped path is the one without a decode copy (copy_hint NULL); where it orders or words a check differently,
// moe_check and moe_check_proj branch on that.
struct MoePathRules {
    const char* word;                               // the path's name in messages
    int max_T, max_rows;                            // the largest T / T topk the path takes (0: no such limit)
    int multiple;                                   // of H and I
    const char* copy_hint;                          // the post_init(...) argument that builds the decode copy the path needs (NULL: it needs none)
    bool (*group_ok)(const gptq_layer_t&);          // the path's group-size rule (NULL: the decode copy's own, tiled_layer_ok) and what its message says
    const char* group_text;
    bool copy_aligned;                              // the decode copy is read by 16-byte vectors
    int low_bit_flag;                               // the gptq_moe_t flag that opens 2- and 3-bit experts (0: 4 or 8 bits only)
    bool lds_fit;                                   // plan_moe_decode has the last word
};
static const MoePathRules MOE_GROUPED = {"grouped", 0, 0, 64, nullptr, nullptr, nullptr, false, GPTQ_MOE_LOW_BIT, false};
static const MoePathRules MOE_DECODE = {"decode", 4, 0, 64, "decode_copy=True", nullptr, nullptr, false, GPTQ_MOE_LOW_BIT_DECODE, true};
static const MoePathRules MOE_BATCH = {"batch", 64, 0, 128, "batch=True", moe_batch_group_ok, "32, 64, 128 times a power of two, or one group", false,
                                       GPTQ_MOE_LOW_BIT_BATCH, false};
static const MoePathRules MOE_PREFILL = {"prefill", 0, GPTQ_MOE_PREFILL_MAX_ROWS, 128, "prefill=True", moe_prefill_group_ok, "64 times a power of two, or one group",
                                         true, GPTQ_MOE_LOW_BIT_PREFILL, false};

static int moe_check_bits(const MoePathRules& r, int bits, int flags) {
    if (bits == 4 || bits == 8) return GPTQ_OK;
    if (!(flags & r.low_bit_flag)) return fail(GPTQ_ERR_UNSUPPORTED, "%d-bit experts: the %s path takes 4 or 8 bits", bits, r.word);
    if (bits != 2 && bits != 3) return fail(GPTQ_ERR_UNSUPPORTED, "%d-bit experts: the %s path takes 2, 3, 4 or 8 bits", bits, r.word);      // (check_layer: 2, 3, 4 or 8)
    return GPTQ_OK;
}

// One projection's experts against the shape [K -> N] and gate[0] (G).
static int moe_check_proj(const MoePathRules& r, const gptq_layer_t* const* Ls, int E, int K, int N, const gptq_layer_t* G, int flags, const char* name) {
    if (!Ls) return fail(GPTQ_ERR_NULL, "moe->%s is NULL", name);
    const bool grouped = !r.copy_hint;
    for (int e = 0; e < E; ++e) {
        const gptq_layer_t* L = Ls[e];
        if (int rc = check_layer(L)) return rc;
        if (L->K != K || L->N != N)
            return fail(GPTQ_ERR_SHAPE, "expert %d %s is [%d -> %d], expected [%d -> %d]", e, name, L->K, L->N, K, N);
        const gptq_layer_t* B = grouped ? Ls[0] : G;      // bits: the grouped path compares within the projection (gate against up: moe_check), the copy paths against gate[0]
        if (L->bits != B->bits || L->group_size != Ls[0]->group_size || L->dtype != G->dtype || L->zero_mode != Ls[0]->zero_mode)
            return fail(GPTQ_ERR_UNSUPPORTED, "the %s layers of all experts must share bits, group_size, dtype and zero_mode (expert %d differs)", name, e);
        if (L->bias || L->epilogue != GPTQ_EPI_NONE)
            return fail(GPTQ_ERR_UNSUPPORTED, "expert %d %s: the %s path takes no bias and no epilogue", e, name, r.word);
        if (grouped) {
            if (L->g_idx && !L->qweight_seq)
                return fail(GPTQ_ERR_UNSUPPORTED, "expert %d %s: raw act-order (no re-sequenced rows) is not taken by the grouped path", e, name);
            continue;
        }
        if (r.group_ok && !r.group_ok(*L)) return fail(GPTQ_ERR_UNSUPPORTED, "group_size %d: the %s path takes %s", L->group_size, r.word, r.group_text);
        if (!L->qweight_tiled || !L->qconst_tiled)
            return fail(GPTQ_ERR_UNSUPPORTED, "expert %d %s carries no decode copy (QuantMoEExperts.post_init(%s) builds it)", e, name, r.copy_hint);
        if (!tiled_layer_ok(*L)) {
            if (r.group_ok) return fail(GPTQ_ERR_UNSUPPORTED, "expert %d %s: raw act-order (no re-sequenced rows) is not taken by the decode copy", e, name);
            return fail(GPTQ_ERR_UNSUPPORTED, "expert %d %s: group_size %d (or raw act-order) is not taken by the decode copy", e, name, L->group_size);
        }
        if (r.copy_aligned && (((uintptr_t)L->qweight_tiled | (uintptr_t)L->qconst_tiled) & 15))
            return fail(GPTQ_ERR_UNSUPPORTED, "expert %d %s: the decode copy must be 16-byte aligned", e, name);
    }
    if (!grouped) return GPTQ_OK;
    const gptq_layer_t* A = Ls[0];
    if (int rc = moe_check_bits(r, A->bits, flags)) return rc;
    if (A->group_size % 32 && A->group_size < K)
        return fail(GPTQ_ERR_UNSUPPORTED, "group_size %d: the grouped path takes multiples of 32 (or one group)", A->group_size);
    return GPTQ_OK;
}

static int moe_check(const MoePathRules& r, const gptq_moe_t* m, int T, int topk) {
    const bool grouped = !r.copy_hint;
    if (!m) return fail(GPTQ_ERR_NULL, "moe is NULL");
    // (GPTQ_MOE_LOW_BIT_DECODE: a known bit of the decode path's, nothing here reads it.  GPTQ_MOE_LOW_BIT_BATCH and GPTQ_MOE_LOW_BIT_PREFILL stay among the
    // unknown ones here: 0x10 and 0x20 were refused by these entry points before the copy paths gave them a meaning, and they answer as they did -- a caller
    // of both kinds of path keeps two gptq_moe_t)
    if (grouped && (m->flags & ~(GPTQ_MOE_LOW_BIT | GPTQ_MOE_LOW_BIT_DECODE)))
        return fail(GPTQ_ERR_UNSUPPORTED, "moe->flags = 0x%x: unknown flag bits (GPTQ_MOE_LOW_BIT and GPTQ_MOE_LOW_BIT_DECODE are the only ones)", (unsigned)m->flags);
    if (m->E < 1 || m->E > 256) return fail(GPTQ_ERR_UNSUPPORTED, "E = %d experts: the %s path takes 1..256", m->E, r.word);
    if (topk < 1 || topk > 8) return fail(GPTQ_ERR_UNSUPPORTED, "topk = %d: the %s path takes 1..8", topk, r.word);
    if (T < 0) return fail(GPTQ_ERR_SHAPE, "T must be >= 0, got %d", T);
    if (r.max_T && T > r.max_T) return fail(GPTQ_ERR_UNSUPPORTED, "T = %d tokens: the %s path takes 1..%d (the grouped path serves more)", T, r.word, r.max_T);
    if (r.max_rows && (long)T * topk > r.max_rows)
        return fail(GPTQ_ERR_UNSUPPORTED, "T topk = %ld rows: the %s path takes up to %d (the grouped path serves more)", (long)T * topk, r.word, r.max_rows);
    if (!m->gate || !m->up || !m->down || !m->gate[0]) return fail(GPTQ_ERR_NULL, "moe->gate / up / down must be non-NULL");
    const gptq_layer_t* G = m->gate[0];
    if (int rc = check_layer(G)) return rc;
    if (G->dtype != GPTQ_F16 && G->dtype != GPTQ_BF16) return fail(GPTQ_ERR_UNSUPPORTED, "fp32 experts: the %s path takes fp16 / bf16", r.word);
    if (!grouped)      // (the grouped path judges each projection's own bits: moe_check_proj.  With the decode path's flag the 2- / 3-bit forms of moe_shared.hip serve them)
        if (int rc = moe_check_bits(r, G->bits, m->flags)) return rc;
    const int H = G->K, I = G->N;
    if (H % r.multiple || I % r.multiple)
        return fail(GPTQ_ERR_UNSUPPORTED, "hidden (%d) and intermediate (%d) sizes must be multiples of %d", H, I, r.multiple);
    if (grouped && (long)T * topk > 0x3fffffffL / 4) return fail(GPTQ_ERR_SHAPE, "T = %d is too large", T);
    if (int rc = moe_check_proj(r, m->gate, m->E, H, I, G, m->flags, "gate")) return rc;
    if (int rc = moe_check_proj(r, m->up, m->E, H, I, G, m->flags, "up")) return rc;
    const gptq_layer_t* U = m->up[0];
    if (U->bits != G->bits || U->group_size != G->group_size || U->zero_mode != G->zero_mode)      // (the copy paths: every expert's bits are gate[0]'s by now)
        return fail(GPTQ_ERR_UNSUPPORTED, "gate and up layers must share bits, group_size and zero_mode");
    if (int rc = moe_check_proj(r, m->down, m->E, I, H, G, m->flags, "down")) return rc;
    if (r.lds_fit) {
        const MoeDecodePlan pl = plan_moe_decode(*m, T, topk);
        if (!pl.ok) return fail(GPTQ_ERR_UNSUPPORTED, "hidden (%d) / intermediate (%d) sizes: the staged row and constants (%d / %d bytes) do not fit the LDS", H, I, pl.lds_pair, pl.lds_down);
    }
    return GPTQ_OK;
}

// The three tables: [gate | up | down][E] entries of the kernels' own pointer structs, built on the host and copied once.
static int moe_build_table_impl(const MoePathRules& r, const gptq_moe_t* m, void* table, void* stream, size_t eb, void (*entry)(const gptq_layer_t&, void*),
                                const char* what) {
    if (int rc = moe_check(r, m, 0, 1)) return rc;
    if (!table) return fail(GPTQ_ERR_NULL, "table is NULL");
    const size_t E = (size_t)m->E;
    std::vector<char> host(3 * E * eb);
    for (size_t e = 0; e < E; ++e) {
        entry(*m->gate[e], host.data() + e * eb);
        entry(*m->up[e], host.data() + (E + e) * eb);
        entry(*m->down[e], host.data() + (2 * E + e) * eb);
    }
    hipError_t e = hipMemcpyAsync(table, host.data(), host.size(), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);      // the host copy dies with this call
    if (e != hipSuccess) return hip_fail(e, what);
    return GPTQ_OK;
}

// The front of the forward entry points behind their check and plan: the pointers, their alignment, the workspace.
static int moe_forward_args(const char* table_word, const void* table, const void* x, const int64_t* idx, const float* w, const void* out, const void* ws,
                            size_t ws_bytes, size_t need) {
    if (!table || !x || !idx || !w || !out) return fail(GPTQ_ERR_NULL, "%s / x / topk_idx / topk_w / out must be non-NULL", table_word);
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)ws) & 15) return fail(GPTQ_ERR_UNSUPPORTED, "x / out / workspace must be 16-byte aligned");
    if (!ws || ws_bytes < need) return fail(GPTQ_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", need, ws ? ws_bytes : (size_t)0);
    return GPTQ_OK;
}

// ... and their tail: h_out = [H_sorted [R, I] | pos [R]] out of the workspace (h_out NULL: nothing)
static int moe_copy_h_out(const gptq_moe_t* m, void* h_out, const void* ws, size_t off_h, size_t off_pos, int T, int topk, void* stream, const char* what) {
    if (!h_out) return GPTQ_OK;
    const gptq_layer_t* G = m->gate[0];
    const size_t R = (size_t)T * topk, hb = R * G->N * dtype_size(G->dtype);
    hipError_t e = hipMemcpyAsync(h_out, (const char*)ws + off_h, hb, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpyAsync((char*)h_out + hb, (const char*)ws + off_pos, 4 * R, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, what);
    return GPTQ_OK;
}

size_t gptq_moe_table_bytes(int E) { return E > 0 ? 3 * (size_t)E * moe_table_entry_bytes() : 0; }

int gptq_moe_build_table(const gptq_moe_t* m, void* table, void* stream) {
    return moe_build_table_impl(MOE_GROUPED, m, table, stream, moe_table_entry_bytes(), moe_table_entry, "gptq_moe_build_table copy");
}

size_t gptq_moe_workspace_bytes(const gptq_moe_t* m, int T, int topk) {
    if (moe_check(MOE_GROUPED, m, T, topk)) return 0;
    const gptq_layer_t* G = m->gate[0];
    return plan_moe(m->E, T, topk, G->K, G->N, G->dtype).bytes;
}

int gptq_moe_forward(const gptq_moe_t* m, const void* table, const void* x, const int64_t* idx, const float* w, int T, int topk, void* out, void* h_out,
                     void* ws, size_t ws_bytes, void* stream) {
    if (int rc = moe_check(MOE_GROUPED, m, T, topk)) return rc;
    if (T == 0) return GPTQ_OK;
    const gptq_layer_t* G = m->gate[0];
    const MoePlan pl = plan_moe(m->E, T, topk, G->K, G->N, G->dtype);
    if (int rc = moe_forward_args("table", table, x, idx, w, out, ws, ws_bytes, pl.bytes)) return rc;
    hipError_t e = launch_moe(*m, table, pl, x, idx, w, T, topk, out, (char*)ws, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_moe_forward launch");
    return moe_copy_h_out(m, h_out, ws, pl.off_h, pl.off_pos, T, topk, stream, "gptq_moe_forward h_out copy");
}

int gptq_describe_moe_plan(const gptq_moe_t* m, int T, int topk, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    if (moe_check(MOE_GROUPED, m, T, topk)) return describe_decline(out, out_bytes, "per_expert");
    const gptq_layer_t* G = m->gate[0];
    const MoePlan pl = plan_moe(m->E, T, topk, G->K, G->N, G->dtype);
    snprintf(out, out_bytes, "path=grouped bm=%d bn=%d tiles=%d ksplit=%d launches=%d", pl.bm, pl.bn, pl.tiles, pl.ksplit, T > 0 ? 4 : 0);
    return GPTQ_OK;
}

// ---- the backward of the grouped path (moe_grad.hip) ----
size_t gptq_moe_grad_table_bytes(int E) { return E > 0 ? 3 * (size_t)E * moe_grad_table_entry_bytes() : 0; }

int gptq_moe_build_grad_table(const gptq_moe_t* m, void* table, void* stream) {
    return moe_build_table_impl(MOE_GROUPED, m, table, stream, moe_grad_table_entry_bytes(), moe_grad_table_entry, "gptq_moe_build_grad_table copy");
}

size_t gptq_moe_backward_workspace_bytes(const gptq_moe_t* m, int T, int topk) {
    if (moe_check(MOE_GROUPED, m, T, topk)) return 0;
    const gptq_layer_t* G = m->gate[0];
    return plan_moe_grad(m->E, T, topk, G->K, G->N, G->dtype).bytes;
}

int gptq_moe_backward(const gptq_moe_t* m, const void* table, const void* grad_table, const void* x, const int64_t* idx, const float* w, const void* dout,
                      int T, int topk, void* dx, float* dw, void* dgu_out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = moe_check(MOE_GROUPED, m, T, topk)) return rc;
    if (T == 0) return GPTQ_OK;
    if (!dx && !dw) return fail(GPTQ_ERR_NULL, "dx and dw are both NULL: nothing to compute");
    if (!table || !grad_table || !x || !idx || !w || !dout)
        return fail(GPTQ_ERR_NULL, "table / grad_table / x / topk_idx / topk_w / dout must be non-NULL");
    if (((uintptr_t)x | (uintptr_t)dout | (uintptr_t)dx | (uintptr_t)ws) & 15)
        return fail(GPTQ_ERR_UNSUPPORTED, "x / dout / dx / workspace must be 16-byte aligned");
    const gptq_layer_t* G = m->gate[0];
    const MoeGradPlan pl = plan_moe_grad(m->E, T, topk, G->K, G->N, G->dtype);
    if (!ws || ws_bytes < pl.bytes) return fail(GPTQ_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", pl.bytes, ws ? ws_bytes : (size_t)0);
    hipError_t e = launch_moe_grad(*m, table, grad_table, pl, x, idx, w, dout, T, topk, dx, dw, (char*)ws, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_moe_backward launch");
    if (dgu_out) {
        const size_t R = (size_t)T * topk, gb = R * G->N * dtype_size(G->dtype);
        e = hipMemcpyAsync(dgu_out, (char*)ws + pl.off_g, gb, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemcpyAsync((char*)dgu_out + gb, (char*)ws + pl.off_u, gb, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemcpyAsync((char*)dgu_out + 2 * gb, (char*)ws + pl.off_pos, 4 * R, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "gptq_moe_backward dgu_out copy");
    }
    return GPTQ_OK;
}

int gptq_describe_moe_backward_plan(const gptq_moe_t* m, int T, int topk, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    if (moe_check(MOE_GROUPED, m, T, topk)) return describe_decline(out, out_bytes, "per_expert");
    const gptq_layer_t* G = m->gate[0];
    const MoeGradPlan pl = plan_moe_grad(m->E, T, topk, G->K, G->N, G->dtype);
    snprintf(out, out_bytes, "path=grouped_backward tiles=%d launches=%d wg_recompute=%ld wg_down=%ld wg_up=%ld", pl.tiles, T > 0 ? 5 : 0,
             (long)pl.tiles * (G->N / 64), (long)pl.tiles * pl.nblk_i, (long)pl.tiles * pl.nblk_h);
    return GPTQ_OK;
}

// ---- the same layers at 1..4 tokens on the experts' decode copy (moe_decode.hip) ----
size_t gptq_moe_decode_table_bytes(int E) { return E > 0 ? 3 * (size_t)E * moe_decode_table_entry_bytes() : 0; }

int gptq_moe_build_decode_table(const gptq_moe_t* m, void* table, void* stream) {
    // 2- / 3-bit experts opened for a copy path other than the decode path (GPTQ_MOE_LOW_BIT_BATCH / GPTQ_MOE_LOW_BIT_PREFILL without
    // GPTQ_MOE_LOW_BIT_DECODE): the check of the first such path whose flag is set -- batch, then prefill -- stands in front of the table it reads; every
    // other set, flagged or not, is checked as before
    const bool low_copy = m && !(m->flags & GPTQ_MOE_LOW_BIT_DECODE) && m->gate && m->gate[0] && (m->gate[0]->bits == 2 || m->gate[0]->bits == 3);
    const MoePathRules& r = low_copy && (m->flags & GPTQ_MOE_LOW_BIT_BATCH) ? MOE_BATCH : (low_copy && (m->flags & GPTQ_MOE_LOW_BIT_PREFILL) ? MOE_PREFILL : MOE_DECODE);
    return moe_build_table_impl(r, m, table, stream, moe_decode_table_entry_bytes(), moe_decode_table_entry, "gptq_moe_build_decode_table copy");
}

size_t gptq_moe_decode_workspace_bytes(const gptq_moe_t* m, int T, int topk) {
    if (moe_check(MOE_DECODE, m, T, topk)) return 0;
    return plan_moe_decode(*m, T, topk).bytes;
}

int gptq_moe_decode_forward(const gptq_moe_t* m, const void* table, const void* x, const int64_t* idx, const float* w, int T, int topk, void* out, void* h_out,
                            void* ws, size_t ws_bytes, void* stream) {
    if (int rc = moe_check(MOE_DECODE, m, T, topk)) return rc;
    if (T == 0) return GPTQ_OK;
    const MoeDecodePlan pl = plan_moe_decode(*m, T, topk);
    if (int rc = moe_forward_args("table", table, x, idx, w, out, ws, ws_bytes, pl.bytes)) return rc;
    hipError_t e = launch_moe_decode(*m, table, pl, x, idx, w, T, topk, out, (char*)ws, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_moe_decode_forward launch (was gptq_init() called on this device?)");
    return moe_copy_h_out(m, h_out, ws, pl.off_h, pl.off_pos, T, topk, stream, "gptq_moe_decode_forward h_out copy");
}

int gptq_describe_moe_decode_plan(const gptq_moe_t* m, int T, int topk, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    if (moe_check(MOE_DECODE, m, T, topk)) return describe_decline(out, out_bytes, "none");
    const MoeDecodePlan pl = plan_moe_decode(*m, T, topk);
    snprintf(out, out_bytes, "path=decode launches=%d wg_pair=%d wg_down=%d waves_pair=%d waves_down=%d lds_pair=%d lds_down=%d", T > 0 ? 2 : 0, pl.wg_pair, pl.wg_down,
             pl.waves_pair, pl.waves_down, pl.lds_pair, pl.lds_down);
    return GPTQ_OK;
}

// ---- the shared expert of a Qwen-MoE block next to the routed experts (moe_shared.hip) ----
static int moe_shared_check_layer(const gptq_layer_t* L, int K, int N, const gptq_layer_t* R, const char* name, const char* routed) {
    if (!L) return fail(GPTQ_ERR_NULL, "shared->%s is NULL", name);
    if (int rc = check_layer(L)) return rc;
    if (L->K != K || L->N != N) return fail(GPTQ_ERR_SHAPE, "shared %s is [%d -> %d], expected [%d -> %d]", name, L->K, L->N, K, N);
    if (L->bits != R->bits)
        return fail(GPTQ_ERR_UNSUPPORTED, "shared %s has %d bits, the routed %s layers %d: the shared decode form takes equal bits", name, L->bits, routed, R->bits);
    if (L->dtype != R->dtype)
        return fail(GPTQ_ERR_UNSUPPORTED, "shared %s has dtype %d, the routed %s layers dtype %d: the shared decode form takes equal dtypes", name, L->dtype, routed, R->dtype);
    if (L->bias || L->epilogue != GPTQ_EPI_NONE) return fail(GPTQ_ERR_UNSUPPORTED, "shared %s: the decode path takes no bias and no epilogue", name);
    if (!L->qweight_tiled || !L->qconst_tiled)
        return fail(GPTQ_ERR_UNSUPPORTED, "shared %s carries no decode copy (QuantLinear.post_init builds it)", name);
    if (!tiled_layer_ok(*L))
        return fail(GPTQ_ERR_UNSUPPORTED, "shared %s: group_size %d (or raw act-order) is not taken by the decode copy", name, L->group_size);
    return GPTQ_OK;
}

static int moe_shared_check(const gptq_moe_t* m, const gptq_moe_shared_t* sh, int T, int topk) {
    if (int rc = moe_check(MOE_DECODE, m, T, topk)) return rc;
    if (m->gate[0]->bits == 2 || m->gate[0]->bits == 3)      // (in front of everything that reads the shared layers: no form of the fused launches decodes these widths)
        return fail(GPTQ_ERR_UNSUPPORTED, "%d-bit routed experts: the shared decode form takes 4 or 8 bits (2- and 3-bit experts run gptq_moe_decode_forward and the combine tail)", m->gate[0]->bits);
    if (!sh) return fail(GPTQ_ERR_NULL, "shared is NULL");
    if (sh->flags || sh->reserved) return fail(GPTQ_ERR_UNSUPPORTED, "shared->flags / reserved must be 0");
    if (!sh->gate || !sh->up || !sh->down) return fail(GPTQ_ERR_NULL, "shared->gate / up / down must be non-NULL");
    const gptq_layer_t* G = m->gate[0];
    const gptq_layer_t* D = m->down[0];
    const int H = G->K, Is = sh->gate->N;
    if (Is <= 0 || Is % 64) return fail(GPTQ_ERR_UNSUPPORTED, "shared intermediate size %d: I_s %% 64 must be 0", Is);
    if (int rc = moe_shared_check_layer(sh->gate, H, Is, G, "gate", "gate")) return rc;
    if (int rc = moe_shared_check_layer(sh->up, H, Is, G, "up", "up")) return rc;
    if (int rc = moe_shared_check_layer(sh->down, Is, H, D, "down", "down")) return rc;
    if (sh->up->group_size != sh->gate->group_size) return fail(GPTQ_ERR_UNSUPPORTED, "shared gate and up must share their group_size");
    if ((uintptr_t)sh->gate_w & 15) return fail(GPTQ_ERR_UNSUPPORTED, "shared->gate_w must be 16-byte aligned");
    const MoeSharedPlan pl = plan_moe_shared_decode(*m, *sh, T, topk);
    if (!pl.ok) return fail(GPTQ_ERR_UNSUPPORTED, "shared intermediate size %d: the staged rows and constants (%d / %d bytes) do not fit the LDS", Is, pl.lds_pair, pl.lds_down);
    return GPTQ_OK;
}

size_t gptq_moe_shared_decode_workspace_bytes(const gptq_moe_t* m, const gptq_moe_shared_t* sh, int T, int topk) {
    if (moe_shared_check(m, sh, T, topk)) return 0;
    return plan_moe_shared_decode(*m, *sh, T, topk).bytes;
}

int gptq_moe_shared_decode_forward(const gptq_moe_t* m, const gptq_moe_shared_t* sh, const void* table, const void* x, const int64_t* idx, const float* w, int T,
                                   int topk, void* out, void* h_out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = moe_shared_check(m, sh, T, topk)) return rc;
    if (T == 0) return GPTQ_OK;
    const MoeSharedPlan pl = plan_moe_shared_decode(*m, *sh, T, topk);
    if (int rc = moe_forward_args("decode_table", table, x, idx, w, out, ws, ws_bytes, pl.bytes)) return rc;
    hipError_t e = launch_moe_shared_decode(*m, *sh, table, pl, x, idx, w, T, topk, out, (char*)ws, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_moe_shared_decode_forward launch (was gptq_init() called on this device?)");
    if (int rc = moe_copy_h_out(m, h_out, ws, pl.off_h, pl.off_pos, T, topk, stream, "gptq_moe_shared_decode_forward h_out copy")) return rc;
    if (h_out) {                                    // ... then hs [T, I_s] and s [T]
        const size_t R = (size_t)T * topk, es = dtype_size(m->gate[0]->dtype), hb = R * m->gate[0]->N * es, sb = (size_t)T * sh->gate->N * es;
        e = hipMemcpyAsync((char*)h_out + hb + 4 * R, (char*)ws + pl.off_hs, sb, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemcpyAsync((char*)h_out + hb + 4 * R + sb, (char*)ws + pl.off_s, 4 * (size_t)T, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "gptq_moe_shared_decode_forward h_out copy");
    }
    return GPTQ_OK;
}

int gptq_describe_moe_shared_decode_plan(const gptq_moe_t* m, const gptq_moe_shared_t* sh, int T, int topk, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    if (moe_shared_check(m, sh, T, topk)) return describe_decline(out, out_bytes, "none");
    const MoeSharedPlan pl = plan_moe_shared_decode(*m, *sh, T, topk);
    snprintf(out, out_bytes, "path=decode_shared launches=%d wg_pair=%d wg_down=%d waves_pair=%d waves_down=%d lds_pair=%d lds_down=%d", T > 0 ? 2 : 0, pl.wg_pair,
             pl.wg_down, pl.waves_pair, pl.waves_down, pl.lds_pair, pl.lds_down);
    return GPTQ_OK;
}

int gptq_moe_shared_combine(const void* x, const void* gate_w, const void* ys, void* out, int T, int H, int dtype, void* stream) {
    if (dtype == GPTQ_F32) return fail(GPTQ_ERR_UNSUPPORTED, "fp32: the shared combine kernel takes fp16 / bf16");
    if (dtype != GPTQ_F16 && dtype != GPTQ_BF16) return fail(GPTQ_ERR_UNSUPPORTED, "unknown dtype enum %d", dtype);
    if (H <= 0 || H % 8) return fail(GPTQ_ERR_UNSUPPORTED, "H = %d must be a positive multiple of 8", H);
    if (T < 0) return fail(GPTQ_ERR_SHAPE, "T must be >= 0, got %d", T);
    if (T == 0) return GPTQ_OK;
    if (!ys || !out || (gate_w && !x)) return fail(GPTQ_ERR_NULL, "x / ys / out must be non-NULL");
    if (((uintptr_t)x | (uintptr_t)gate_w | (uintptr_t)ys | (uintptr_t)out) & 15) return fail(GPTQ_ERR_UNSUPPORTED, "x / gate_w / ys / out must be 16-byte aligned");
    hipError_t e = launch_moe_shared_combine(x, gate_w, ys, out, T, H, dtype, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_moe_shared_combine launch");
    return GPTQ_OK;
}

// ---- the same layers at 5..64 tokens on the experts' decode copy (moe_rows.hip) ----
size_t gptq_moe_batch_workspace_bytes(const gptq_moe_t* m, int T, int topk) {
    if (moe_check(MOE_BATCH, m, T, topk)) return 0;
    return plan_moe_batch(*m, T, topk).bytes;
}

int gptq_moe_batch_forward(const gptq_moe_t* m, const void* table, const void* x, const int64_t* idx, const float* w, int T, int topk, void* out, void* h_out,
                           void* ws, size_t ws_bytes, void* stream) {
    if (int rc = moe_check(MOE_BATCH, m, T, topk)) return rc;
    if (T == 0) return GPTQ_OK;
    const MoeBatchPlan pl = plan_moe_batch(*m, T, topk);
    if (int rc = moe_forward_args("table", table, x, idx, w, out, ws, ws_bytes, pl.bytes)) return rc;
    hipError_t e = launch_moe_batch(*m, table, pl, x, idx, w, T, topk, out, (char*)ws, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_moe_batch_forward launch (was gptq_init() called on this device?)");
    return moe_copy_h_out(m, h_out, ws, pl.off_h, pl.off_pos, T, topk, stream, "gptq_moe_batch_forward h_out copy");
}

int gptq_describe_moe_batch_plan(const gptq_moe_t* m, int T, int topk, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    if (moe_check(MOE_BATCH, m, T, topk)) return describe_decline(out, out_bytes, "none");
    const MoeBatchPlan pl = plan_moe_batch(*m, T, topk);
    const int n = snprintf(out, out_bytes, "path=batch bm=%d s=%d tiles=%d launches=%d waves_pair=%d waves_down=%d lds_pair=%d lds_down=%d", pl.bm, pl.s, pl.tiles,
                           pl.launches, pl.waves_pair, pl.waves_down, pl.lds_pair, pl.lds_down);
    const int bits = m->gate[0]->bits;                         // 2 / 3 bits (GPTQ_MOE_LOW_BIT_BATCH): the width is named; 4 / 8 bits answer as they did
    if ((bits == 2 || bits == 3) && n > 0 && (size_t)n < out_bytes) snprintf(out + n, out_bytes - (size_t)n, " bits=%d", bits);
    return GPTQ_OK;
}

// ---- the same layers at prompt row counts on the experts' decode copy (moe_panel.hip) ----
size_t gptq_moe_prefill_workspace_bytes(const gptq_moe_t* m, int T, int topk) {
    if (moe_check(MOE_PREFILL, m, T, topk)) return 0;
    return plan_moe_prefill(*m, T, topk).bytes;
}

int gptq_moe_prefill_forward(const gptq_moe_t* m, const void* table, const void* x, const int64_t* idx, const float* w, int T, int topk, void* out, void* h_out,
                             void* ws, size_t ws_bytes, void* stream) {
    if (int rc = moe_check(MOE_PREFILL, m, T, topk)) return rc;
    if (T == 0) return GPTQ_OK;
    const MoePrefillPlan pl = plan_moe_prefill(*m, T, topk);
    if (int rc = moe_forward_args("table", table, x, idx, w, out, ws, ws_bytes, pl.bytes)) return rc;
    hipError_t e = launch_moe_prefill(*m, table, pl, x, idx, w, T, topk, out, (char*)ws, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_moe_prefill_forward launch (was gptq_init() called on this device?)");
    return moe_copy_h_out(m, h_out, ws, pl.off_h, pl.off_pos, T, topk, stream, "gptq_moe_prefill_forward h_out copy");
}

int gptq_describe_moe_prefill_plan(const gptq_moe_t* m, int T, int topk, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out is NULL");
    if (moe_check(MOE_PREFILL, m, T, topk)) return describe_decline(out, out_bytes, "none");
    const MoePrefillPlan pl = plan_moe_prefill(*m, T, topk);
    const int n = snprintf(out, out_bytes, "path=prefill bm=%d launches=%d tiles=%d nt_pair=%d nt_down=%d waves=%d waves_pair=%d spw_pair=%d spw_down=%d lds=%d", pl.bm,
                           pl.launches, pl.tiles, pl.nt_pair, pl.nt_down, pl.waves_down, pl.waves_pair, pl.spw_pair, pl.spw_down, pl.lds_down);
    const int bits = m->gate[0]->bits;                         // 2 / 3 bits (GPTQ_MOE_LOW_BIT_PREFILL): the width is named; 4 / 8 bits answer as they did
    if ((bits == 2 || bits == 3) && n > 0 && (size_t)n < out_bytes) snprintf(out + n, out_bytes - (size_t)n, " bits=%d", bits);
    return GPTQ_OK;
}

int gptq_unpack_weights(const uint32_t* qweight, int K, int N, int bits, uint8_t* w_out, void* stream) {
    if (!qweight || !w_out) return fail(GPTQ_ERR_NULL, "qweight/w_out must be non-NULL");
    if (!bits_ok(bits)) return fail(GPTQ_ERR_UNSUPPORTED, "Only 2,3,4,8 bits are supported. (got %d)", bits);
    if (K <= 0 || N <= 0 || K % 32 || N % 32) return fail(GPTQ_ERR_SHAPE, "K (%d), N (%d) must be positive multiples of 32", K, N);
    hipError_t e = launch_unpack_weights(qweight, K, N, bits, w_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_unpack_weights launch");
    return GPTQ_OK;
}

int gptq_unpack_zeros(const uint32_t* qzeros, int G, int N, int bits, int zero_mode, int32_t* z_out, void* stream) {
    if (!qzeros || !z_out) return fail(GPTQ_ERR_NULL, "qzeros/z_out must be non-NULL");
    if (!bits_ok(bits)) return fail(GPTQ_ERR_UNSUPPORTED, "Only 2,3,4,8 bits are supported. (got %d)", bits);
    if (G <= 0 || N <= 0 || N % 32) return fail(GPTQ_ERR_SHAPE, "G (%d) must be > 0 and N (%d) a positive multiple of 32", G, N);
    hipError_t e = launch_unpack_zeros(qzeros, G, N, bits, zero_mode, z_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_unpack_zeros launch");
    return GPTQ_OK;
}

int gptq_pack_weights(const void* W, const void* scale_in, const void* zero_in, const int32_t* g_idx, int K, int N,
                      int bits, int group_size, int w_dtype, int qparam_dtype, uint32_t* qweight_out, void* scales_out,
                      void* stream) {
    if (!W || !scale_in || !zero_in || !qweight_out) return fail(GPTQ_ERR_NULL, "W/scale_in/zero_in/qweight_out must be non-NULL");
    if (!bits_ok(bits)) return fail(GPTQ_ERR_UNSUPPORTED, "Only 2,3,4,8 bits are supported. (got %d)", bits);
    if (!dtype_ok(w_dtype) || !dtype_ok(qparam_dtype)) return fail(GPTQ_ERR_UNSUPPORTED, "unsupported dtype enum");
    if (K <= 0 || N <= 0 || K % 32 || N % 32 || group_size <= 0)
        return fail(GPTQ_ERR_SHAPE, "K (%d), N (%d) must be positive multiples of 32 and group_size (%d) > 0", K, N, group_size);
    hipError_t e = launch_pack_weights(W, scale_in, zero_in, g_idx, K, N, bits, group_size, w_dtype, qparam_dtype,
                                       qweight_out, scales_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_pack_weights launch");
    return GPTQ_OK;
}

int gptq_pack_zeros(const void* zero_in, int G, int N, int bits, int qparam_dtype, uint32_t* qzeros_out, void* stream) {
    if (!zero_in || !qzeros_out) return fail(GPTQ_ERR_NULL, "zero_in/qzeros_out must be non-NULL");
    if (!bits_ok(bits)) return fail(GPTQ_ERR_UNSUPPORTED, "Only 2,3,4,8 bits are supported. (got %d)", bits);
    if (!dtype_ok(qparam_dtype)) return fail(GPTQ_ERR_UNSUPPORTED, "unsupported dtype enum");
    if (G <= 0 || N <= 0 || N % 32) return fail(GPTQ_ERR_SHAPE, "G (%d) must be > 0 and N (%d) a positive multiple of 32", G, N);
    hipError_t e = launch_pack_zeros(zero_in, G, N, bits, qparam_dtype, qzeros_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_pack_zeros launch");
    return GPTQ_OK;
}

int gptq_make_sequential(const int32_t* g_idx, int K, int group_size, int32_t* perm_out, int* uniform_out) {
    if (!g_idx || !perm_out) return fail(GPTQ_ERR_NULL, "g_idx/perm_out must be non-NULL");
    if (K <= 0 || group_size <= 0) return fail(GPTQ_ERR_SHAPE, "K (%d) and group_size (%d) must be > 0", K, group_size);
    int gmax = 0;
    for (int k = 0; k < K; ++k) {
        if (g_idx[k] < 0) return fail(GPTQ_ERR_SHAPE, "g_idx[%d] = %d is negative", k, g_idx[k]);
        gmax = std::max(gmax, g_idx[k]);
    }
    // stable counting sort by group (same ordering rule as Q4Matrix::make_sequential)
    std::vector<int> start((size_t)gmax + 2, 0);
    for (int k = 0; k < K; ++k) start[(size_t)g_idx[k] + 1]++;
    for (int g = 0; g <= gmax; ++g) start[(size_t)g + 1] += start[g];
    std::vector<int> cursor(start.begin(), start.end() - 1);
    for (int k = 0; k < K; ++k) perm_out[cursor[g_idx[k]]++] = k;
    if (uniform_out) {
        int uni = 1;
        for (int i = 0; i < K && uni; ++i) uni = (g_idx[perm_out[i]] == i / group_size);
        *uniform_out = uni;
    }
    return GPTQ_OK;
}

int gptq_resequence_qweight(const uint32_t* qweight, const int32_t* perm, int K, int N, int bits, uint32_t* out, void* stream) {
    if (!qweight || !perm || !out) return fail(GPTQ_ERR_NULL, "qweight/perm/out must be non-NULL");
    if (!bits_ok(bits)) return fail(GPTQ_ERR_UNSUPPORTED, "Only 2,3,4,8 bits are supported. (got %d)", bits);
    if (K <= 0 || N <= 0 || K % 32 || N % 32) return fail(GPTQ_ERR_SHAPE, "K (%d), N (%d) must be positive multiples of 32", K, N);
    hipError_t e = launch_resequence(qweight, perm, K, N, bits, out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_resequence_qweight launch");
    return GPTQ_OK;
}

// the layer as the decode copy sees it: plain 3/4/8-bit, source rows = qweight_seq when the layer has one
static int decode_copy_source(const gptq_layer_t* L, gptq_layer_t* S) {
    int rc = check_layer(L);
    if (rc) return rc;
    *S = *L;
    S->qweight_tiled = (const uint32_t*)(uintptr_t)16;       // placeholders: tiled_layer_ok() only asks whether the copy COULD exist
    S->qconst_tiled = (const void*)(uintptr_t)16;
    S->tiled_cols = GPTQ_STRIP_COLS;
    // a plain [gate | up] layer with the fused epilogue gets a copy too (round 5: its decode kernel pairs strip s of the two halves); act-order ones do not
    // an ungated layer (RELU / GELU / GELU_TANH) gets whatever copy the layer without its epilogue gets: the pair form reads it where it fits, the inner call of the separate pass elsewhere
    if (is_plain_act(L->epilogue)) S->epilogue = GPTQ_EPI_NONE;
    if (S->epilogue != GPTQ_EPI_NONE && (L->g_idx != nullptr || L->N % (2 * GPTQ_STRIP_COLS) != 0)) S->epilogue = -1;
    if (S->epilogue == -1 || !tiled_layer_ok(*S))
        return fail(GPTQ_ERR_UNSUPPORTED, "the decode copy needs a 2-, 3-, 4- or 8-bit fp16/bf16 layer (2 bits: no fused epilogue), group_size a power-of-two multiple of 32 (16 at 8 bits) or >= K, "
                                          "and for act-order layers qweight_seq + perm (bits=%d dtype=%d group_size=%d)", L->bits, L->dtype, L->group_size);
    return GPTQ_OK;
}

int gptq_prepack_decode_bytes(const gptq_layer_t* L, size_t* tiled_bytes, size_t* const_bytes) {
    if (tiled_bytes) *tiled_bytes = 0;
    if (const_bytes) *const_bytes = 0;
    if (!tiled_bytes || !const_bytes) return fail(GPTQ_ERR_NULL, "tiled_bytes/const_bytes must be non-NULL");
    gptq_layer_t S;
    if (int rc = decode_copy_source(L, &S)) return rc;
    *tiled_bytes = tiled_weight_bytes(*L);
    *const_bytes = tiled_const_bytes(*L);
    return GPTQ_OK;
}

int gptq_prepack_decode(const gptq_layer_t* L, uint32_t* tiled_out, void* const_out, void* stream) {
    if (!tiled_out || !const_out) return fail(GPTQ_ERR_NULL, "qweight_tiled_out/qconst_tiled_out must be non-NULL");
    gptq_layer_t S;
    if (int rc = decode_copy_source(L, &S)) return rc;
    const uint32_t* src = L->qweight_seq ? L->qweight_seq : L->qweight;
    if (tiled_out == src || tiled_out == L->qweight) return fail(GPTQ_ERR_UNSUPPORTED, "gptq_prepack_decode does not work in place (the checkpoint tensors are never rewritten)");
    hipError_t e = launch_prepack_decode(src, L->qzeros, L->scales, L->K, L->N, L->bits, L->group_size, L->zero_mode, tiled_out, const_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_prepack_decode launch");
    return GPTQ_OK;
}

int gptq_unprepack_decode(const uint32_t* qweight_tiled, int K, int N, int bits, uint32_t* qweight_out, void* stream) {
    if (!qweight_tiled || !qweight_out) return fail(GPTQ_ERR_NULL, "qweight_tiled/qweight_out must be non-NULL");
    if (bits != 2 && bits != 3 && bits != 4 && bits != 8) return fail(GPTQ_ERR_UNSUPPORTED, "the decode copy exists for 2-, 3-, 4- and 8-bit layers (got %d)", bits);
    if (K <= 0 || N <= 0 || K % 32 || N % GPTQ_STRIP_COLS) return fail(GPTQ_ERR_SHAPE, "K (%d) must be a positive multiple of 32 and N (%d) of %d", K, N, GPTQ_STRIP_COLS);
    if ((const void*)qweight_tiled == (const void*)qweight_out) return fail(GPTQ_ERR_UNSUPPORTED, "gptq_unprepack_decode does not work in place");
    hipError_t e = launch_unprepack_decode(qweight_tiled, K, N, bits, qweight_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_unprepack_decode launch");
    return GPTQ_OK;
}

int gptq_permute_columns(const void* x, const int32_t* perm, int M, int K, int dtype, void* x_out, void* stream) {
    if (!x || !perm || !x_out) return fail(GPTQ_ERR_NULL, "x/perm/x_out must be non-NULL");
    if (!dtype_ok(dtype)) return fail(GPTQ_ERR_UNSUPPORTED, "unsupported dtype enum %d", dtype);
    if (M <= 0 || K <= 0) return fail(GPTQ_ERR_SHAPE, "M (%d) and K (%d) must be > 0", M, K);
    hipError_t e = launch_permute_columns(x, perm, M, K, dtype, x_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_permute_columns launch");
    return GPTQ_OK;
}

int gptq_describe_plan_xstage(const gptq_layer_t* L, int M, const gptq_tuning_t* tune) {
    if (check_layer(L) || M <= 0 || (tune && (tune->path == 2 || tune->path == 4))) return 0;
    const ForwardRoute r = route_forward(L, M, tune);
    return (r.kind == ROUTE_TILED || r.kind == ROUTE_TILED_PAIR) ? r.tp.xsteps : 0;
}

int gptq_describe_plan(const gptq_layer_t* L, int M, const gptq_tuning_t* tune, char* out, size_t out_bytes) {
    if (!out || out_bytes == 0) return fail(GPTQ_ERR_NULL, "out must be non-NULL");
    out[0] = 0;
    int rc = check_layer(L);
    if (rc) return rc;
    if (M <= 0) return fail(GPTQ_ERR_SHAPE, "M must be > 0, got %d", M);
    if (tune && (tune->path == 2 || tune->path == 4)) return fail(GPTQ_ERR_UNSUPPORTED, "tuning.path = %d was retired in round 6", tune->path);
    const ForwardRoute r = route_forward(L, M, tune);
    const char* separate = r.unfused_epilogue ? "separate" : "none";
    switch (r.kind) {
        case ROUTE_TILED:
        case ROUTE_TILED_PAIR: {
            const bool pair = r.kind == ROUTE_TILED_PAIR;
            snprintf(out, out_bytes, "path=gemv kernel=strips ln=4 waves=%d u=%d ksplit=%d mt=%d strips=%d pair=%d perm=0 epilogue=%s aligned=%d", r.tp.waves, r.tp.u, r.tp.ksplit, r.tp.mt,
                     r.tp.strips_total, pair ? 1 : 0, pair ? "fused" : separate, r.tp.aligned ? 1 : 0);
            break;
        }
        case ROUTE_STREAM:
        case ROUTE_STREAM_SEQ:
            snprintf(out, out_bytes, "path=gemv kernel=stream ln=%d waves=%d u=%d ksplit=%d mt=%d strips=%d pair=0 perm=%d epilogue=%s", r.sp.ln, r.sp.waves,
                     r.sp.u, r.sp.ksplit, r.sp.mt, r.sp.strips_total, r.kind == ROUTE_STREAM_SEQ ? 2 : 0,
                     is_plain_act(L->epilogue) ? separate : "none");      // ("none" also in front of a separate SiLU * mul pass: the string this kernel has always had; the ungated epilogues say what runs)
            break;
        case ROUTE_GEMM: {
            const GemmPlan& g = r.gp;
            const char* kern = (g.kernel == GEMM_WIDE && g.wide_tiled) ? "wide_copy" : gemm_kernel_names[g.kernel];
            snprintf(out, out_bytes, "path=gemm kernel=%s mt=%d bk=%d kg=%d ksplit=%d tiles=%dx%d tail=%d tail_slices=%d perm=%d dma=%d waves=%d u=%d epilogue=%s%s", kern, g.mt, g.bk,
                     g.kg == 2 ? 2 : 1, g.ksplit, g.nbm, g.nbn, g.tail, g.tail ? (1 << g.tail_lg) : 1, g.use_seq ? 1 : 0,
                     (g.glds || g.kernel == GEMM_STREAM64 || g.kernel == GEMM_MID) ? 1 : 0, g.waves, g.u, separate,
                     g.lowbit ? " body=lowbit" : "");      // (a flagged 2-bit layer on the dense form of the low-bit routed-expert kernels; every other line is what it was)
            break;
        }
        case ROUTE_GEMV: {
            const GemvPlan& v = r.vp;
            const char* kern = v.mfma ? "mfma" : (v.mfmag ? "mfma_generic" : "generic");
            snprintf(out, out_bytes, "path=gemv kernel=%s ln=%d waves=%d u=%d ksplit=%d mt=%d strips=%d pair=%d perm=%d epilogue=%s%s", kern, v.ln,
                     v.waves, v.u, v.ksplit, v.mt, v.strips, v.pair ? 1 : 0, v.xperm ? 2 : (v.use_seq ? 1 : 0),
                     v.pair ? "fused" : separate, v.magic ? " deq=magic" : "");
            break;
        }
    }
    return GPTQ_OK;
}

static int awq_shape_check(int K, int N, int group_size) {
    if (K <= 0 || N <= 0 || group_size <= 0) return fail(GPTQ_ERR_SHAPE, "K (%d), N (%d), group_size (%d) must be > 0", K, N, group_size);
    if (K % 8 || N % 8) return fail(GPTQ_ERR_SHAPE, "K (%d) and N (%d) must be multiples of 8 (4-bit words)", K, N);
    if (K % group_size) return fail(GPTQ_ERR_SHAPE, "K (%d) must be a multiple of group_size (%d)", K, group_size);
    return GPTQ_OK;
}

int gptq_awq_unpack(const uint32_t* awq_qweight, const uint32_t* awq_qzeros, const void* awq_scales, int K, int N,
                    int group_size, void* weight_kn_out, int8_t* zeros_out, void* stream) {
    if (!awq_qweight || !awq_qzeros || !awq_scales || !weight_kn_out || !zeros_out)
        return fail(GPTQ_ERR_NULL, "awq_qweight/awq_qzeros/awq_scales/weight_kn_out/zeros_out must be non-NULL");
    if (int rc = awq_shape_check(K, N, group_size)) return rc;
    hipError_t e = launch_awq_unpack(awq_qweight, awq_qzeros, awq_scales, K, N, group_size, weight_kn_out, zeros_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_awq_unpack launch");
    return GPTQ_OK;
}

int gptq_awq_repack(const uint32_t* awq_qweight, const uint32_t* awq_qzeros, int K, int N, int group_size,
                    uint32_t* qweight_out, uint32_t* qzeros_out, void* stream) {
    if (!awq_qweight || !awq_qzeros || !qweight_out || !qzeros_out)
        return fail(GPTQ_ERR_NULL, "awq_qweight/awq_qzeros/qweight_out/qzeros_out must be non-NULL");
    if (int rc = awq_shape_check(K, N, group_size)) return rc;
    hipError_t e = launch_awq_repack(awq_qweight, awq_qzeros, K, N, group_size, qweight_out, qzeros_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_awq_repack launch");
    return GPTQ_OK;
}


// ---- direct peer-store all-gather (peer.hip) ---------------------------------------------------------------------------
static int check_peer_group(const gptq_peer_group_t* pg, int M, int dtype) {
    if (!pg) return fail(GPTQ_ERR_NULL, "peer group is NULL");
    if (pg->world < 1 || pg->world > GPTQ_PEER_MAX) return fail(GPTQ_ERR_SHAPE, "peer group world (%d) must be 1..%d", pg->world, GPTQ_PEER_MAX);
    if (pg->rank < 0 || pg->rank >= pg->world) return fail(GPTQ_ERR_SHAPE, "peer group rank (%d) outside 0..%d", pg->rank, pg->world - 1);
    if (!pg->state) return fail(GPTQ_ERR_NULL, "peer group state is NULL");
    for (int r = 0; r < pg->world; ++r)
        if (!pg->xbuf[0][r] || !pg->xbuf[1][r] || !pg->flags[r]) return fail(GPTQ_ERR_NULL, "peer group: buffers / flags of rank %d are NULL", r);
    if (!dtype_ok(dtype)) return fail(GPTQ_ERR_UNSUPPORTED, "unsupported dtype enum %d", dtype);
    if (pg->N <= 0 || pg->N % pg->world || (pg->N / pg->world) % 32)
        return fail(GPTQ_ERR_SHAPE, "peer group: out_features (%d) must split over %d ranks in multiples of 32 columns", pg->N, pg->world);
    if (M <= 0 || M > pg->rows_max) return fail(GPTQ_ERR_SHAPE, "M (%d) must be 1..rows_max (%d) of the exchange buffers", M, pg->rows_max);
    return GPTQ_OK;
}

int gptq_peer_scatter(const gptq_peer_group_t* pg, const void* y_local, int M, int n_local, int dtype, void* stream) {
    if (int rc = check_peer_group(pg, M, dtype)) return rc;
    if (!y_local) return fail(GPTQ_ERR_NULL, "y_local must be non-NULL");
    if (n_local != pg->N / pg->world) return fail(GPTQ_ERR_SHAPE, "n_local (%d) must be N / world = %d", n_local, pg->N / pg->world);
    hipError_t e = launch_peer_scatter(*pg, y_local, M, n_local, dtype, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_peer_scatter launch");
    return GPTQ_OK;
}

int gptq_peer_publish(const gptq_peer_group_t* pg, void* stream) {
    if (int rc = check_peer_group(pg, 1, GPTQ_F16)) return rc;
    hipError_t e = launch_peer_publish(*pg, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_peer_publish launch");
    return GPTQ_OK;
}

int gptq_peer_collect(const gptq_peer_group_t* pg, void* out, int M, int dtype, uint32_t max_spins, void* stream) {
    if (int rc = check_peer_group(pg, M, dtype)) return rc;
    if (!out) return fail(GPTQ_ERR_NULL, "out must be non-NULL");
    if (max_spins == 0) return fail(GPTQ_ERR_SHAPE, "max_spins must be > 0 (the wait is bounded by design)");
    hipError_t e = launch_peer_collect(*pg, out, M, dtype, max_spins, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "gptq_peer_collect launch");
    return GPTQ_OK;
}

// The column shard's decode kernel with the scatter as its epilogue: local kernel + one collect launch per tensor-parallel layer.
int gptq_forward_scatter(const gptq_layer_t* L, const void* x, int M, const gptq_peer_group_t* pg, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_layer(L);
    if (rc) return rc;
    if (!x) return fail(GPTQ_ERR_NULL, "x must be non-NULL");
    if ((rc = check_align(x, nullptr, ws))) return rc;
    if ((rc = check_peer_group(pg, M, L->dtype))) return rc;
    if (L->N != pg->N / pg->world) return fail(GPTQ_ERR_SHAPE, "the layer's out_features (%d) must be the rank's shard N / world = %d", L->N, pg->N / pg->world);
    const gptq_layer_t* one[1] = {L};
    const ForwardRoute r = route_forward(L, M, nullptr);
    const TiledPlan& tp = r.tp;
    if (M > 4 || L->epilogue != GPTQ_EPI_NONE || L->g_idx || r.kind != ROUTE_TILED || (tp.u != 2 && tp.u != 4))
        return fail(GPTQ_ERR_UNSUPPORTED, "gptq_forward_scatter: the fused scatter is the epilogue of the decode-copy kernel (M <= 4, a plain 3/4/8-bit fp16/bf16 "
                                          "layer that carries qweight_tiled / qconst_tiled); use gptq_forward + gptq_peer_scatter for this call");
    const WsView wv = split_ws(ws, ws_bytes);
    if (int rc = need_body(wv, tp.partial_bytes)) return rc;
    void* outs[1] = {nullptr};                                  // the rank's own slice travels through its own exchange buffer like every peer's
    hipError_t e = launch_tiled(one, tp, x, outs, M, wv.header, wv.body, (hipStream_t)stream, pg);
    if (e != hipSuccess) return hip_fail(e, "gptq_forward_scatter launch (was gptq_init() called on this device?)");
    return GPTQ_OK;
}

int gptq_forward_gather(const gptq_layer_t* L, const void* x, void* out, int M, const gptq_peer_group_t* pg, uint32_t max_spins, void* ws, size_t ws_bytes,
                        void* stream) {
    if (!out) return fail(GPTQ_ERR_NULL, "out must be non-NULL");
    if (max_spins == 0) return fail(GPTQ_ERR_SHAPE, "max_spins must be > 0 (the wait is bounded by design)");
    if (int rc = check_align(x, out, ws)) return rc;
    if (int rc = gptq_forward_scatter(L, x, M, pg, ws, ws_bytes, stream)) return rc;
    return gptq_peer_collect(pg, out, M, L->dtype, max_spins, stream);
}

int gptq_peer_gather(const gptq_peer_group_t* pg, const void* y_local, void* out, int M, int n_local, int dtype,
                     uint32_t max_spins, void* stream) {
    if (!out) return fail(GPTQ_ERR_NULL, "out must be non-NULL");
    if (max_spins == 0) return fail(GPTQ_ERR_SHAPE, "max_spins must be > 0 (the wait is bounded by design)");
    if (int rc = gptq_peer_scatter(pg, y_local, M, n_local, dtype, stream)) return rc;
    return gptq_peer_collect(pg, out, M, dtype, max_spins, stream);
}

}  // extern "C"
