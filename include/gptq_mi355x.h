/* gptq_mi355x.h -- C ABI of libgptq_mi355x.so: the MI355X (gfx950) quantized-linear hot path.
 *
 * This is the drop-in boundary.  Every entry point takes plain device pointers, ints and an
 * opaque stream handle (a hipStream_t passed as void*); no torch / pybind types.  Each one
 * replaces a pybind11 function (or group of functions) of the reference's native extensions,
 * cited as `file:line` into the AutoGPTQ tree (v0.8.0.dev0):
 *
 *   gptq_forward / gptq_gemv / gptq_gemm
 *       <- autogptq_cuda_{64,256}: vecquant{2,3,4,8}matmul            autogptq_extension/cuda_256/autogptq_cuda_256.cpp:5-64,175-178
 *                                  vecquant{2,3,4,8}matmul_old        :68-126,180-183
 *                                  vecquant{2,3,4}matmul_faster_old   :128-171,184-186
 *       <- exllama_kernels.q4_matmul                                  autogptq_extension/exllama/exllama_ext.cpp:176-217,258
 *       <- exllamav2_kernels.gemm_half_q_half                         autogptq_extension/exllamav2/ext.cpp:95-126,133
 *       <- autogptq_marlin_cuda.mul                                   autogptq_extension/marlin/marlin_cuda.cpp:30-75,78
 *       and the pure-PyTorch fallback they all share                  auto_gptq/nn_modules/qlinear/qlinear_cuda_old.py:291-355, qlinear_cuda.py:253-317
 *   gptq_dequant
 *       <- the `reconstruct` step of exllama / exllamav2              exllama/cuda_func/q4_matrix.cu:171-225, exllamav2/cuda/q_matrix.cu:158-279,452-500
 *   gptq_moe_forward
 *       <- the expert loop of the reference's Mixtral (per-expert QuantLinears, auto_gptq/modeling/mixtral.py) as one routed, grouped call
 *   gptq_moe_decode_forward, gptq_moe_batch_forward, gptq_moe_prefill_forward
 *       <- the same expert loop at the row counts of token generation (1..4 tokens) and of batched generation (5..64), on the experts' decode copy
 *   gptq_moe_router
 *       <- the router in front of that loop (transformers' MixtralTopKRouter: F.linear, softmax, topk, renormalise) as one launch
 *   gptq_moe_router_grouped
 *       <- the sigmoid / group-limited router of DeepSeek-V3 and GLM-4 MoE blocks (transformers' DeepseekV3TopkRouter) as one launch
 *   gptq_moe_shared_decode_forward, gptq_moe_shared_combine
 *       <- the shared expert next to that loop (transformers' Qwen2MoeSparseMoeBlock: + sigmoid(shared_expert_gate(x)) * shared_expert(x)), inside the two
 *          decode launches at 1..4 tokens, and its linear / sigmoid / mul / add tail as one launch at any token count
 *   gptq_moe_backward
 *       <- autograd through the same expert loop (dequantise + torch.matmul per expert), as one routed, grouped call
 *   gptq_grad_input
 *       <- the backward of the reference's training route: dequantise + torch.matmul under autograd
 *                                                                     qlinear_cuda_old.py:291-355, qlinear_cuda.py:253-317
 *          and the triton backend's QuantLinearFunction.backward      auto_gptq/nn_modules/triton_utils/kernels.py:408-426
 *   gptq_lora_down, gptq_lora_up, gptq_lora_apply
 *       <- GPTQLoraLinear.forward's adapter branch (torch matmuls on the base output)   auto_gptq/utils/peft_utils.py:100-123
 *   gptq_lora_backward
 *       <- autograd through that branch (torch matmuls; get_gptq_peft_model's training use)   auto_gptq/utils/peft_utils.py:126-176
 *   gptq_make_sequential + gptq_resequence_qweight + gptq_permute_columns
 *       <- exllama_kernels.make_q4 (Q4Matrix::make_sequential)        exllama/exllama_ext.cpp:134-171, cuda_func/q4_matrix.cu:63-169
 *          exllamav2_kernels.make_q_matrix                            exllamav2/ext.cpp:26-93, cuda/q_matrix.cu:502-627
 *          column_remap_cuda                                          exllama/cuda_func/column_remap.cu:9-63
 *       (unlike those, never mutates qweight in place: results go to caller-owned side buffers)
 *   gptq_prepack_decode / gptq_prepack_decode_bytes
 *       <- the load-time weight re-layouts: exllamav2 shuffle_kernel   exllamav2/cuda/q_matrix.cu:19-42,149
 *          exllama Q4Matrix::make_sequential's row rewrite             exllama/cuda_func/q4_matrix.cu:105-169
 *          Marlin's repack kernel                                      marlin/marlin_repack.cu:8-92
 *       (into a caller-owned side buffer; the checkpoint tensor stays as it is)
 *   gptq_pack_weights / gptq_pack_zeros
 *       <- QuantLinear.pack (CPU-only in the reference)               auto_gptq/nn_modules/qlinear/qlinear_cuda.py:108-203
 *   gptq_unpack_weights / gptq_unpack_zeros
 *       <- the integer unpack of the Python path                      qlinear_cuda_old.py:295-344, qlinear_cuda.py:257-295
 *
 * Tensor layout = the GPTQ v1 checkpoint ABI (K = in_features, N = out_features):
 *   qweight uint32 [K/32*bits, N]   row-major; values packed along K, LSB first
 *   qzeros  uint32 [G, N/32*bits]   G = ceil(K/group_size); packed along N; stores zero-1
 *   scales  dtype  [G, N]
 *   g_idx   int32  [K] or NULL      NULL = sequential groups (k / group_size)
 *   bias    dtype  [N] or NULL
 *   x       dtype  [M, K] row-major; out dtype [M, N] row-major
 *
 * Conventions
 *   - every function returns GPTQ_OK (0) or a gptq_status_t > 0; gptq_last_error() returns a
 *     thread-local human-readable message for the last failure on the calling thread.
 *   - nothing allocates or frees device memory; scratch is caller-provided and sized by
 *     gptq_workspace_bytes().  The first GPTQ_WORKSPACE_HEADER_BYTES of a workspace hold the arrival
 *     tickets of the in-launch K-split combine: they must be ZERO when the buffer is first handed to
 *     the library (one hipMemset at allocation).  Its first half (32 KiB: arrival tickets, and the per-slice
 *     flag words of the 17..128-row kernel's K-split combine, which its owner slices clear again) is left zero by
 *     every launch; its second half carries state from one launch to the next and is NOT zero afterwards: one
 *     launch-epoch word per column strip for the streamed GEMV's K-split combine (partial sums travel as
 *     {value, tag} granules through the body and are validated by their tag), and in the last 64 bytes the
 *     launch epoch / arrival count / sticky error word ([2]: a bounded wait gave up) of the exchanges.
 *     One workspace serves one stream at a time (launches that may overlap need their own).  Kernels are enqueued on the caller's stream, never synchronise,
 *     and are legal inside hipGraph capture: besides the kernel launches the forward entry points make one kind of runtime-API call, hipGetDevice(), and only
 *     for launches whose workgroups wait for each other inside the launch (K slices of the 17..256-row kernel): their grid is checked against the CU count.
 *     Process-global state of the library: the per-device CU count and the > 64 KiB dynamic-LDS grants, both written once per device by gptq_init(), which
 *     the caller runs once per device, outside any capture, before the first forward (a launch that needs the CU count and does not find it is refused).
 *     A bounded wait inside a launch that gives up (another process held the CUs) sets word [2] of the header's last 64 bytes and never hangs the queue:
 *     that launch's result is wrong and the word stays set -- poll it (autogptq_amd.qlinear_mi355x.exchange_error) where CUs are shared.
 *   - results are run-to-run deterministic (no floating-point atomics, fixed summation orders): every entry point is bit-reproducible.
 *   - alignment: `x`, `out`, every `outs[i]` and `workspace` of the dense forward entry points -- gptq_forward[_ex], gptq_gemv, gptq_gemm,
 *     gptq_forward_multi[_ex], gptq_mlp_forward[_ex], gptq_forward_scatter / _gather -- are 16-byte aligned (the kernels load x by LDS DMA and 16-byte
 *     vectors); anything else is refused with GPTQ_ERR_UNSUPPORTED before a launch.  A contiguous view at an odd element offset (a slice of a flat
 *     arena) is copied by the caller first -- the Python wrappers do.  gptq_grad_input, the gptq_lora_* and the gptq_moe_* entries state the same rule.
 */
#ifndef GPTQ_MI355X_H
#define GPTQ_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPTQ_MI355X_ABI_VERSION 8
#define GPTQ_WORKSPACE_HEADER_BYTES 65536

typedef enum gptq_status_t {
    GPTQ_OK = 0,
    GPTQ_ERR_NULL = 1,         /* required pointer is NULL */
    GPTQ_ERR_SHAPE = 2,        /* K/N/M/group_size violate the layout rules */
    GPTQ_ERR_UNSUPPORTED = 3,  /* bits/dtype/mode combination not implemented by this entry point */
    GPTQ_ERR_WORKSPACE = 4,    /* workspace missing or smaller than gptq_workspace_bytes() */
    GPTQ_ERR_LAUNCH = 5        /* HIP reported a launch/runtime error */
} gptq_status_t;

typedef enum gptq_dtype_t { GPTQ_F16 = 0, GPTQ_BF16 = 1, GPTQ_F32 = 2 } gptq_dtype_t;

/* Zero-point convention:
 *   WRAP   z = (field + 1) & maxq   -- qlinear_cuda_old.py:301-304 and every native 4-bit kernel
 *   NOWRAP z =  field + 1           -- qlinear_cuda.py:262-264; also cuda_old's 3-bit branch */
typedef enum gptq_zero_mode_t { GPTQ_ZERO_WRAP = 0, GPTQ_ZERO_NOWRAP = 1 } gptq_zero_mode_t;

/* Fused epilogue of the caller.  SILU_MUL is the gate/up pair of a gated MLP stored as ONE layer
 * whose columns are [gate | up] (the reference concatenates packed tensors along out_features the same way,
 * fused_llama_attn.py:171-173):  out[M, N/2] = silu(y[:, :N/2]) * y[:, N/2:]  with y = x @ W (+ bias), silu and the
 * product evaluated on the fp32 sums and rounded once -- the arithmetic of the reference's fused MLP kernel
 * (fused_llama_mlp.py:237-239).  Needs N % 64 == 0.
 * GELU_TANH_MUL is the same pair layer with the gate of Gemma's GeGLU MLP: layout, shape rules, plans, workspace sizes and gptq_describe_plan strings are
 * those of SILU_MUL;  out[M, N/2] = T( gelu_tanh(y_gate) * y_up ),  gelu_tanh(g) = g / (1 + exp(-c(g))),  c(g) = 2 sqrt(2/pi) (g + 0.044715 g^3),
 * 2 sqrt(2/pi) = 1.5957691216057308 -- the tanh approximation of GELU (torch: F.gelu(approximate='tanh'), "gelu_new"), since
 * 0.5 (1 + tanh(v)) = 1 / (1 + exp(-2 v)); SiLU is the same form with c(g) = g.  Activation and product on the fp32 sums (bias included), rounded once.
 * RELU / GELU / GELU_TANH (16 .. 18; 3 .. 15 are unassigned and refused) are the activation of an UNGATED MLP, act(fc1(x) + b) of OPT, GPT-NeoX, Falcon, BLOOM,
 * GPT-J, Phi-1/2, StarCoder2:  out[M, N] = T( act(y) ),  y = x @ W (+ bias) -- any legal layer, no N % 64 rule, the activation on the fp32 sum, rounded once.
 *   RELU       max(y, 0)
 *   GELU       0.5 y (1 + erf(y / sqrt(2)))                      torch: F.gelu(y)
 *   GELU_TANH  y / (1 + exp(-c(y))), c as above                  torch: F.gelu(y, approximate='tanh'), "gelu_new"
 * Decode rows (M <= 4) of a plain 3- / 4- / 8-bit fp16 / bf16 layer that carries its decode copy run as ONE launch (the pair form of the decode kernel with
 * two stores in place of the product: gptq_describe_plan says pair=1 epilogue=fused).  Every other call (M >= 5, act-order, 2-bit, fp32, no copy) runs the
 * layer without its epilogue INTO `out` and then an elementwise pass IN PLACE on `out` (epilogue=separate): y is rounded to T once in between, nothing is
 * staged, and gptq_workspace_bytes* of the layer equal those of the same layer with epilogue NONE.  gptq_gemv / gptq_gemm / gptq_mlp_forward_act,
 * the grouped, tensor-parallel and MoE entry points take no such layer (gptq_forward_multi runs it as a single call). */
typedef enum gptq_epilogue_t {
    GPTQ_EPI_NONE = 0, GPTQ_EPI_SILU_MUL = 1, GPTQ_EPI_GELU_TANH_MUL = 2,
    GPTQ_EPI_RELU = 16, GPTQ_EPI_GELU = 17, GPTQ_EPI_GELU_TANH = 18
} gptq_epilogue_t;

/* One quantized linear layer.  POD; the caller owns every pointer and keeps it alive. */
typedef struct gptq_layer_t {
    const uint32_t *qweight;   /* [K/32*bits, N] */
    const uint32_t *qzeros;    /* [G, N/32*bits] */
    const void     *scales;    /* [G, N] dtype */
    const int32_t  *g_idx;     /* [K] or NULL (sequential) */
    const void     *bias;      /* [N] dtype or NULL */
    int32_t K, N, bits, group_size;   /* group_size > 0 (the module resolves -1 to K) */
    int32_t dtype;             /* gptq_dtype_t of x / scales / bias / out */
    int32_t zero_mode;         /* gptq_zero_mode_t */
    /* Optional derived (post_init) side buffers; all NULL = run straight from the checkpoint
     * tensors.  Built by gptq_make_sequential + gptq_resequence_qweight for act-order layers:
     * rows of qweight_seq are in group-sorted order and perm[i] is the original k of sorted
     * position i, so group(i) = i / group_size. */
    const uint32_t *qweight_seq;  /* [K/32*bits, N] or NULL */
    const int32_t  *perm;         /* [K] or NULL */
    int32_t epilogue;             /* gptq_epilogue_t; with SILU_MUL / GELU_TANH_MUL `out` is [M, N/2] */
    int32_t tiled_cols;           /* GPTQ_STRIP_COLS when the two side buffers below are given, else 0; | GPTQ_COPY_ROWS_INT2: opt-in, below */
    /* Optional derived (post_init) DECODE COPY of a 2-, 3-, 4- or 8-bit layer, built by gptq_prepack_decode (sizes: gptq_prepack_decode_bytes); both NULL =
     * decode streams the checkpoint layout.  With w[k][n] the layer's unpacked integers (rows taken from qweight_seq when the layer has one, else qweight;
     * k past K read as 0), KPL = 32 (16 at 8 bits) and WPL = 4 (3 at 3 bits, 2 at 2 bits):
     *   qweight_tiled [strip s of 16 columns][chunk c of 4 KPL k][k-slot kb 0..3][column 0..15][word 0..WPL-1]: the lane (kb, col) holds the KPL consecutive
     *                 k from k0 = 4 KPL c + KPL kb of column 16 s + col, re-encoded so that masking a word in place yields (k, k + 1) pairs in the order x lies:
     *                   4 bits  word w, stored nibble p = w[k0 + 8 w + {0,2,4,6,1,3,5,7}[p]]     (= a nibble shuffle of qweight[16 c + 4 kb + w][16 s + col])
     *                   8 bits  word w, stored byte p   = w[k0 + 4 w + {0,2,1,3}[p]]
     *                   3 bits  word j: pair p = 5 j + i (i = 0..4) at bit 3 i of the low (k0 + 2 p) and high (k0 + 2 p + 1) 16 bits; bit 15 / 31 = bit j of
     *                           w[k0 + 30] / w[k0 + 31] -- the checkpoint's word-straddling values are resolved here, once
     *                   2 bits  (round 6) word w: pair p (0..7) at bit 2 p of the low (k0 + 16 w + 2 p) and high (k0 + 16 w + 2 p + 1) 16 bits; read by the
     *                           decode kernel (plain and act-order layers, up to 4 rows; no fused epilogue) and -- OPT-IN, per layer: tiled_cols =
     *                           GPTQ_STRIP_COLS | GPTQ_COPY_ROWS_INT2 -- from 5 rows up by the dense forms of the low-bit routed-expert kernels
     *                           (moe_rows_lowbit_kernel<T, 2> at 5 .. 64 rows, moe_panel_lowbit_kernel<T, 2> from 65 rows through the panel band, inside the band
     *                           where the planner would give the 4-bit layer of the same shape the rows / panel kernel -- all of it with
     *                           GPTQ_COPY_ROWS_INT2_WIDE, the measured part of it without: below; gptq_describe_plan: kernel=rows|panel ... body=lowbit).
     *                           Without the flag, and outside those bands, the batched / prefill kernels keep the checkpoint rows.
     *                           The flag rides in tiled_cols because the struct's layout is the ABI: every reader masks it (GPTQ_COPY_COLS), a layer of
     *                           another width, or one without a copy, that carries it behaves exactly as without it
     *                 A strip is one contiguous run, a chunk one contiguous 1024 (3 bits: 768, 2 bits: 512) bytes = one wave load;
     *   qconst_tiled  [strip][group g][REC bytes] = 16 scales (layer dtype) at byte 0, then from byte 32 the 16 zero-points AS USED (zero_mode applied):
     *                 uint8 each, REC = 48, at 2 / 3 / 4 bits; uint16 each, REC = 64, at 8 bits (no-wrap reaches 256).
     * The reference re-lays its weights at load time in every fast backend (exllamav2 q_matrix.cu:19-42,149; exllama q4_matrix.cu:105-169;
     * marlin_repack.cu:8-92 + the scale permutation of qlinear_marlin.py:133-176), in place; here the checkpoint tensors are left as they are. */
    const uint32_t *qweight_tiled;
    const void     *qconst_tiled;
} gptq_layer_t;

#define GPTQ_STRIP_COLS 16
/* OR-ed into gptq_layer_t.tiled_cols: this 2-bit layer's copy is also read at 5+ rows (see qweight_tiled above).  GPTQ_COPY_COLS(tiled_cols) is the strip width.
 * GPTQ_COPY_ROWS_INT2 alone: where the forms measured faster than the checkpoint-row kernels with both layouts resident (profiles/dense_int2_ab.log):
 *   rows form   5 .. 16 rows of layers with N >= 8192 and K <= 4096;   panel form   from 256 rows, and from 128 rows where N >= 8192
 * -- each inside the band where the planner gives the 4-bit layer of the same shape its rows / panel kernel.
 * | GPTQ_COPY_ROWS_INT2_WIDE (means nothing without the first bit): that whole band (5 .. 64 rows: rows form, 65 rows and more: panel form) -- for a layer whose
 * checkpoint rows are NOT resident (QuantLinear sets it on a released layer), where every call that reads rows first pays gptq_unprepack_decode. */
#define GPTQ_COPY_ROWS_INT2 0x100
#define GPTQ_COPY_ROWS_INT2_WIDE 0x200
#define GPTQ_COPY_COLS(tiled_cols) ((tiled_cols) & ~(GPTQ_COPY_ROWS_INT2 | GPTQ_COPY_ROWS_INT2_WIDE))

/* Kernel families a caller may force with gptq_tuning_t.path ("does not fit" is then an error instead of a silent fallback). */
typedef enum gptq_path_t {
    GPTQ_PATH_AUTO = 0,           /* the planner's choice */
    GPTQ_PATH_GEMV_GENERIC = 1,   /* fp32-math GEMV: any bits / dtype / raw act-order g_idx */
    GPTQ_PATH_GEMV_LDS = 2,       /* RETIRED in round 6 (round-1 LDS-staged comparison GEMV): GPTQ_ERR_UNSUPPORTED */
    GPTQ_PATH_GEMM = 3,           /* the MFMA GEMMs (tiled, wide, strips, 17..256-row kernel: the planner picks among them) */
    GPTQ_PATH_GEMV_DIRECT = 4,    /* RETIRED in round 6 (v_dot2 comparison GEMV): GPTQ_ERR_UNSUPPORTED */
    GPTQ_PATH_GEMV_MFMA = 5,      /* matrix-core GEMV on the checkpoint layout (4-bit fp16 / bf16 kernel, or the 2/3/8-bit one) */
    GPTQ_PATH_GEMV_STREAM = 6,    /* streamed (LDS-DMA) GEMV on the checkpoint layout */
    GPTQ_PATH_GEMV_DECODE_COPY = 8 /* decode kernel on the load-time decode copy (qweight_tiled / qconst_tiled): M <= 8; the planner's own choice up to 4 rows, and at
                                    * 5..8 rows on single plain 4-bit layers with K and N in 2048..4096 */
} gptq_path_t;

/* Optional launch-shape override; NULL = the planner's choice, which is what a drop-in caller passes.  lanes_n / waves / ksplit / path force a documented
 * geometry or kernel family.  reserved[] must be zero for a drop-in caller: the measurement tools under tools/ and the forced-geometry grids of the test
 * suite use these four words as LAB switches (A/B runs, ablations); their slots and values are named in include/gptq_mi355x_lab.h and are not part of
 * the drop-in contract. */
typedef struct gptq_tuning_t {
    int32_t lanes_n;     /* checkpoint-layout GEMVs: lanes of a wave laid along N (4, 8, 16, 64); 4 columns per lane */
    int32_t waves;       /* waves per workgroup (1..16) */
    int32_t ksplit;      /* workgroups along K (1 = no cross-workgroup reduction) */
    int32_t path;        /* gptq_path_t */
    int32_t reserved[4]; /* 0; lab switches: gptq_mi355x_lab.h */
} gptq_tuning_t;

int         gptq_abi_version(void);
const char *gptq_last_error(void);
const char *gptq_status_string(int status);

/* Once per device (the calling thread's current HIP device), outside stream capture, before the first forward on it:
 * grants the dynamic-LDS size of the kernels that use more than the 64 KiB default.  Idempotent.  The reference's
 * equivalents are the one-time per-device set-up calls of its backends (exllama_ext.cpp:100-131 prepare_buffers /
 * set_tuning_params; exllamav2 ext.cpp:26-93 make_q_matrix's temp_dq hand-over). */
int gptq_init(void);

/* Bytes of scratch gptq_forward/gptq_gemv/gptq_gemm may need for this layer and M (0 possible). */
size_t gptq_workspace_bytes(const gptq_layer_t *layer, int M);
/* Same for an explicit launch shape (what gptq_forward_ex/gptq_gemv/gptq_gemm need with `tuning`). */
size_t gptq_workspace_bytes_ex(const gptq_layer_t *layer, int M, const gptq_tuning_t *tuning);

/* max over M = 1..max_M of gptq_workspace_bytes(layer, M): the need is not monotone in M (K splits appear and disappear as
 * the planner changes kernels), so a caller that sizes ONE scratch buffer before hipGraph capture asks for this. */
size_t gptq_workspace_bytes_max(const gptq_layer_t *layer, int max_M);

/* out[M,N] = x[M,K] @ dequant(layer) (+ bias).  Picks GEMV (small M) or MFMA GEMM. */
int gptq_forward(const gptq_layer_t *layer, const void *x, void *out, int M,
                 void *workspace, size_t workspace_bytes, void *stream);

/* n_layers independent layers that read the SAME x[M, K] -- q/k/v of an attention block, gate/up of a gated MLP -- in one
 * call: outs[i] is [M, layers[i]->N].  The reference fuses such layers by concatenating their packed tensors along
 * out_features into one QuantLinear (fused_llama_attn.py:171-203, fused_llama_mlp.py:157-242); this entry point gives the
 * same single launch (<= 4 layers: up to 4 rows the decode-copy kernel over the column strips of all layers -- 3- / 4- / 8-bit fp16 / bf16 layers that
 * carry qweight_tiled, all plain or all act-order; 5 to 128 rows the batched-decode / 17..128-row kernels on plain 4-bit layers where the planner
 * prefers them) without touching or copying the checkpoint tensors, and runs the layers one after the other in every other case -- except that
 * act-order layers which share ONE `perm` pointer (q / k / v, gate / up of a GPTQ checkpoint: the order comes from their common input) read ONE
 * permuted x per call.  CONTRACT of a shared `perm` pointer: the layers that carry it have IDENTICAL g_idx, and every one's qweight_seq was built with
 * that permutation (gptq_make_sequential + gptq_resequence_qweight) -- pointer equality is all this entry point checks; a caller that reuses one perm
 * buffer for layers with different activation orders gets wrong results (the Python side compares the g_idx tensors once: share_act_order).
 * Results are those of n gptq_forward calls either way (same values within fp rounding: the K split may differ).
 * Workspace: gptq_workspace_bytes_multi. */
size_t gptq_workspace_bytes_multi(const gptq_layer_t *const *layers, int n_layers, int M);
int gptq_forward_multi(const gptq_layer_t *const *layers, int n_layers, const void *x, void *const *outs, int M,
                       void *workspace, size_t workspace_bytes, void *stream);
/* ... with an explicit launch shape for the one-launch kernel (experiments; tuning.path = 6 -- streamed GEMV -- or
 * tuning.path = 3 with tuning.reserved[2] = 4 -- batched-decode kernel -- or 5 -- the 17..128-row kernel -- make "does not fit" an error). */
size_t gptq_workspace_bytes_multi_ex(const gptq_layer_t *const *layers, int n_layers, int M, const gptq_tuning_t *tuning);
int gptq_forward_multi_ex(const gptq_layer_t *const *layers, int n_layers, const void *x, void *const *outs, int M,
                          void *workspace, size_t workspace_bytes, void *stream, const gptq_tuning_t *tuning);

/* The gated MLP of a decoder block, out[M, N] = down( silu(gate(x)) * up(x) ), as ONE call: replaces the reference's fused MLP caller
 * (auto_gptq/nn_modules/fused_llama_mlp.py:157-242: FusedLlamaMLPForQuantizedModel.forward = one fused gate|up kernel with the SiLU * mul
 * inside + c_proj).  gate and up are [K -> I], down is [I -> N]; plain layers (epilogue NONE), checkpoint tensors untouched; any bits / dtype /
 * act-order the single-layer entry points take.  Default: gate and up through gptq_forward_multi (one launch for decode rows) into two staging
 * buffers in the workspace, SiLU * mul (silu and the product on fp32, rounded once to the layer dtype, as fused_llama_mlp.py:237-239), down.
 * gptq_mlp_forward_ex takes no path override (round 3's one-launch persistent kernel was measured slower than these three steps and is a lab now:
 * tools/lab/mlp_ring.hip); it exists for signature symmetry with the other _ex entry points. */
size_t gptq_workspace_bytes_mlp(const gptq_layer_t *gate, const gptq_layer_t *up, const gptq_layer_t *down, int M);
size_t gptq_workspace_bytes_mlp_ex(const gptq_layer_t *gate, const gptq_layer_t *up, const gptq_layer_t *down, int M, const gptq_tuning_t *tuning);
int gptq_mlp_forward(const gptq_layer_t *gate, const gptq_layer_t *up, const gptq_layer_t *down, const void *x, void *out, int M,
                     void *workspace, size_t workspace_bytes, void *stream);
int gptq_mlp_forward_ex(const gptq_layer_t *gate, const gptq_layer_t *up, const gptq_layer_t *down, const void *x, void *out, int M,
                        void *workspace, size_t workspace_bytes, void *stream, const gptq_tuning_t *tuning);
/* The same call with the gate's activation as an argument: out = down( act(gate(x)) * up(x) ), act = GPTQ_EPI_SILU_MUL (gptq_mlp_forward, bit for bit) or
 * GPTQ_EPI_GELU_TANH_MUL (Gemma's GeGLU; the formula at gptq_epilogue_t).  Same steps, same workspace (gptq_workspace_bytes_mlp), same
 * gptq_describe_mlp_plan; any other act: GPTQ_ERR_UNSUPPORTED.  gptq_mlp_forward and gptq_mlp_forward_ex are calls of it. */
int gptq_mlp_forward_act(const gptq_layer_t *gate, const gptq_layer_t *up, const gptq_layer_t *down, int act, const void *x, void *out, int M,
                         void *workspace, size_t workspace_bytes, void *stream);
/* Host-only: "kernel=unfused launches=3+ steps=..." for (gate, up, down, M, tuning); as gptq_describe_plan. */
int gptq_describe_mlp_plan(const gptq_layer_t *gate, const gptq_layer_t *up, const gptq_layer_t *down, int M, const gptq_tuning_t *tuning, char *out,
                           size_t out_bytes);

/* Same, with an explicit launch shape / path (tuning may be NULL). */
int gptq_forward_ex(const gptq_layer_t *layer, const void *x, void *out, int M,
                    void *workspace, size_t workspace_bytes, void *stream,
                    const gptq_tuning_t *tuning);

/* Memory-bound decode path (wavefront reductions); any M, intended for M <= 8. */
int gptq_gemv(const gptq_layer_t *layer, const void *x, void *out, int M,
              void *workspace, size_t workspace_bytes, void *stream, const gptq_tuning_t *tuning);

/* MFMA prefill path; fp16/bf16 only. */
int gptq_gemm(const gptq_layer_t *layer, const void *x, void *out, int M,
              void *workspace, size_t workspace_bytes, void *stream, const gptq_tuning_t *tuning);

/* W_out[K,N] (dtype) = scales[g(k),n] * (w[k,n] - z[g(k),n]); bit-exact vs the reference's
 * `weights` tensor (one rounding of the exact product). */
int gptq_dequant(const gptq_layer_t *layer, void *W_out, void *stream);

/* dX[M, K] (+)= dY[M, N] . W^T, W = gptq_dequant(layer) exactly; dY / dX in the layer dtype, row-major, on the layer's device.
 * The layer's epilogue is ignored: dY is the gradient of the product BEFORE any epilogue ([M, N], N = layer->N).  accumulate = 1 adds to dX.
 * Caller's stream, no allocation, no workspace, capturable in a graph.  GPTQ_ERR_NULL / _SHAPE / _UNSUPPORTED as for gptq_forward
 * (dy and dx must also be 16-byte aligned).  Products and sums in fp32, one rounding at the store (accumulate: dX + the sum in fp32, one rounding). */
int gptq_grad_input(const gptq_layer_t *layer, const void *dy, void *dx, int M, int accumulate, void *stream);

/* LoRA adapters beside a quantized layer (the reference's GPTQLoraLinear, auto_gptq/utils/peft_utils.py:58-123, whose merge() must refuse: W is int4 on a
 * fixed grid, so W + s B A has no packed form and every call pays the adapter branch at run time).  For each adapter i of a call:
 *   down:  u_i[m, j]   = T(sum_k x[m, k] * A_i[j, k])                                      fp32 products and sums, one rounding
 *   up:    out_i[m, n] = T(float(out_i[m, n]) + scale_i * sum_j float(u_i[m, j]) * float(B_i[n, j]))   in place on the base layer's output, one rounding
 * A is peft's lora_A.weight [r, K], B its lora_B.weight [N, r], both in the layer dtype T (fp16 / bf16), row-major.  n = 1..GPTQ_LORA_MAX adapters of one
 * call share x, K and dtype (q|k|v, gate|up) and run as ONE launch per direction; adapter i's result is bit-identical to a call of its own.  u_i is a
 * caller tensor [M, r_i] (no workspace); x, u_i, out_i dense row-major and 16-byte aligned.  Caller's stream, no allocation, no atomics, fixed summation
 * order (bit-reproducible), legal inside hipGraph capture; M = 0 launches nothing.  Declined with GPTQ_ERR_UNSUPPORTED and the reason in
 * gptq_last_error() (the caller composes the branch itself): fp32, r outside {8, 16, .., 64}, K % 32, N % 16, misaligned pointers, n > GPTQ_LORA_MAX,
 * adapters of one call that differ in K or dtype. */
#define GPTQ_LORA_MAX 4
typedef struct gptq_lora_t {
    const void *A;          /* [r, K] dtype, row-major, 16-byte aligned */
    const void *B;          /* [N, r] dtype, row-major, 16-byte aligned */
    int32_t K, N, r, dtype; /* r % 8 == 0, 8 <= r <= 64; K % 32 == 0; N % 16 == 0; GPTQ_F16 / GPTQ_BF16 */
    float   scale;          /* lora_alpha / r */
    int32_t reserved;       /* 0 */
} gptq_lora_t;
int gptq_lora_down (const gptq_lora_t *const *loras, int n, const void *x, void *const *u, int M, void *stream);
int gptq_lora_up   (const gptq_lora_t *const *loras, int n, const void *const *u, void *const *outs, int M, void *stream);
int gptq_lora_apply(const gptq_lora_t *const *loras, int n, const void *x, void *const *u, void *const *outs, int M, void *stream); /* down + up */
/* Host-only: "path=lora rows=gemv|mfma wg_down=... wg_up=... launches=2" (rows: the VALU forms up to 8 rows, the matrix-core forms above) or
 * "path=none reason=...".  GPTQ_OK either way (GPTQ_ERR_NULL for a NULL out). */
int gptq_describe_lora_plan(const gptq_lora_t *const *loras, int n, int M, char *out, size_t out_bytes);

/* The adapters' backward.  For each adapter i of a call (T the layer dtype, s = loras[i]->scale, K / N / r of loras[i]; loras[i]->A and ->B are NOT read):
 *   1. du_i[m, j] = T(sum_n dY_i[m, n] * Bt_i[j, n])                      gptq_lora_down with A := Bt [r, N], K := N: bit-identical to that call
 *   2. dA_i[j, k] = s * sum_m float(du_i[m, j]) * float(x[m, k])          fp32 [r, K], overwritten
 *   3. dB_i[n, j] = s * sum_m float(dY_i[m, n]) * float(u_i[m, j])        fp32 [N, r], overwritten; u_i is the forward's u
 *   4. dX[m, k]   = T(float(dX[m, k]) + s * sum_j du_i[m, j] * At_i[k, j])  gptq_lora_up with B := At [K, r], N := K, in place on ONE dX shared by all
 *                                                                          adapters, i = 0 .. n-1 in that order (one launch each); the caller passes
 *                                                                          zeros or a gradient to add to
 * At = A^T [K, r] and Bt = B^T [r, N] are copies in T the caller makes.  dA or dB NULL skips that output; dX NULL skips step 4.  Steps 2 and 3 of all
 * adapters are ONE launch (csrc/adapter_grad.hip): a unit is one 64-wide block of K (or N) x all of r x one slice of M, the row index is the summed one.
 * The slice count of one output [P, Q] ({r, K} or {N, r}) is a function of (M, P, Q) alone, the same on every device:
 *     steps = ceil(M / 32), blocks = ceil(max(P, Q) / 64), S0 = min(64, max(1, steps / 4), ceil(512 / blocks)),
 *     steps_per_slice = ceil(steps / S0), S = ceil(steps / steps_per_slice)          (a slice is 32 steps_per_slice rows, the last may be short)
 * S = 1 writes s * sum straight to the output; S > 1 writes fp32 partials [S, P, Q] to the workspace and a second launch adds them in ascending slice order
 * and applies s.  No atomics, fixed orders: bit-reproducible, and adapter i's results in a call of n are bit-identical to a call of its own.
 * Workspace: sum over the adapters and their two outputs of (S > 1 ? a256(4 S P Q) : 0), a256 = round up to 256; it does not depend on which outputs are
 * NULL, and may be NULL when that is 0.  Caller's stream, no allocation, no sync, legal inside hipGraph capture; M = 0 launches nothing.
 * Declined with GPTQ_ERR_UNSUPPORTED and the reason in gptq_last_error(), before any launch: fp32, r outside {8, 16, .., 64}, K % 32, N % 32 (stricter than
 * the forward: N is a summed length of step 1), n > GPTQ_LORA_MAX, adapters that differ in K or dtype, any pointer not 16-byte aligned.
 * GPTQ_ERR_WORKSPACE for a workspace that is too small, GPTQ_ERR_NULL for a NULL At / Bt / u / dY / du / x. */
typedef struct gptq_lora_grad_t {
    const void *At;         /* [K, r] dtype: lora_A.weight^T */
    const void *Bt;         /* [r, N] dtype: lora_B.weight^T */
    const void *u;          /* [M, r] dtype: the forward's u */
    const void *dY;         /* [M, N] dtype */
    void       *du;         /* [M, r] dtype, written */
    float      *dA;         /* [r, K] fp32, overwritten; NULL: skipped */
    float      *dB;         /* [N, r] fp32, overwritten; NULL: skipped */
} gptq_lora_grad_t;
size_t gptq_lora_backward_workspace_bytes(const gptq_lora_t *const *loras, int n, int M);  /* 0 when the call is declined */
int gptq_lora_backward(const gptq_lora_t *const *loras, const gptq_lora_grad_t *const *grads, int n, const void *x, void *dX, int M,
                       void *workspace, size_t workspace_bytes, void *stream);
/* Host-only: "path=lora_backward S_dA=a,b,.. S_dB=a,b,.. wg_down=... wg_wgrad=... wg_sum=... wg_up=... workspace=... launches=..." for a call that asks
 * for every output (per-adapter slice counts; launches = n + 1 + (any S > 1) + n) or "path=none reason=...".  GPTQ_OK either way. */
int gptq_describe_lora_backward_plan(const gptq_lora_t *const *loras, int n, int M, char *out, size_t out_bytes);

/* Per-row adapter banks: a batch whose rows belong to different fine-tunes of one GPTQ base.  Row m carries a slot ids[m] (int64, device memory); a bank
 * holds `slots` adapters of ONE layer: A [slots][r][K] and B [slots][N][r] in the layer dtype T (fp16 / bf16), scales [slots] fp32, all device memory.
 *   row m with a = ids[m] in [0, slots):
 *     u_m[j]    = T(sum_k x[m, k] * A[a][j, k])                                              fp32 products and sums, one rounding
 *     out[m, n] = T(float(out[m, n]) + scales[a] * sum_j float(u_m[j]) * float(B[a][n, j]))   in place on the base layer's output, one rounding
 *   any other id (-1 is the documented "no adapter") leaves out[m] untouched, bit for bit.
 * The bits of row m depend on x[m], its slot and the bank alone: not on the other rows, their ids, or where row m sits in the batch.  No atomics, no
 * workgroup waits on another, fixed summation order.  ids is read on the device only: all three launches (routing, down, up) are legal inside hipGraph
 * capture and a replay follows the ids then in memory.
 *   routing: rows sorted by slot into tiles of up to 16 rows of one slot, written to `route` (a caller buffer of the size the _bytes query names for
 *            (M, slots), 16-byte aligned; the library owns its layout).  One routing serves every layer of a model step -- the ids are the same for all.
 *   apply:   n = 1..GPTQ_LORA_MAX banks that share x, K, dtype, slots and the routing (q|k|v, gate|up) run as ONE down and ONE up launch; bank i's
 *            result is bit-identical to a call of its own.  u[i] is a caller tensor [M, r_i] (no workspace): the routed rows' u in SORTED-row order
 *            (routed rows ordered by slot, the rows of one slot by ascending m), the rest is not written.  The caller passes the M the route was built with, and banks of the slots it was
 *            built with: the apply call cannot verify either.
 * M = 0 returns GPTQ_OK, launches nothing and dereferences nothing.  Declined with GPTQ_ERR_UNSUPPORTED and the reason in the last-error string, before
 * any launch: fp32, r outside {8, 16, .., 64}, K % 32, N % 16, slots outside 1..256, n > GPTQ_LORA_MAX, banks of one call that differ in K, dtype or
 * slots, any of x, A, B, u[i], outs[i], route not 16-byte aligned, a route_bytes that is too small. */
typedef struct gptq_adapter_bank_t {
    const void  *A;         /* [slots, r, K] dtype, row-major, 16-byte aligned */
    const void  *B;         /* [slots, N, r] dtype, row-major, 16-byte aligned */
    const float *scales;    /* [slots] fp32: lora_alpha / rank of each slot */
    int32_t K, N, r, slots, dtype, reserved; /* r % 8 == 0, 8 <= r <= 64; K % 32 == 0; N % 16 == 0; 1 <= slots <= 256; GPTQ_F16 / GPTQ_BF16; 0 */
} gptq_adapter_bank_t;
size_t gptq_adapter_route_bytes(int M, int slots);  /* 0 for M < 0 or slots outside 1..256 */
int gptq_adapter_route(const int64_t *ids, int M, int slots, void *route, size_t route_bytes, void *stream);
int gptq_adapter_rows_apply(const gptq_adapter_bank_t *const *banks, int n, const void *x, void *const *u, void *const *outs,
                            const void *route, int M, void *stream);
/* Host-only: "path=adapter_rows tiles=... wg_down=... wg_up=... launches=2" (tiles: the grid's bound M / 16 + min(slots, M); workgroups past the routed
 * count return at once) or "path=none reason=...".  GPTQ_OK either way (GPTQ_ERR_NULL for a NULL out). */
int gptq_describe_adapter_rows_plan(const gptq_adapter_bank_t *const *banks, int n, int M, char *out, size_t out_bytes);

/* Routed mixture-of-experts layer (the experts of a Mixtral block: auto_gptq/modeling/mixtral.py, block_sparse_moe.experts.{e}.w1 / w3 / w2).  E experts,
 * each three plain layers: gate (w1) and up (w3) [H -> I], down (w2) [I -> H].  For token t and its topk assignments (t, j) to experts
 * e = topk_idx[t, j] (int64, the dtype of torch.topk; values outside [0, E) are dropped):
 *   h = T(silu(x_t . W1_e) * (x_t . W3_e))   fp32 sums and silu, one rounding;   out[t] = T(sum_j topk_w[t, j] * (h . W2_e))   fp32, ascending j, one rounding
 * (a token with no valid expert gets 0).  Every W is gptq_dequant of its layer, bit for bit.  Grouped path: 4- or 8-bit fp16 / bf16 experts, group_size a
 * multiple of 32 (or >= K), plain or act-order with qweight_seq / perm (re-sequenced rows), H and I multiples of 64, no bias, no epilogue, E <= 256,
 * topk <= 8; all experts of one projection share K, N, bits, group_size, dtype and zero_mode, and gate / up share them too.  Anything else:
 * GPTQ_ERR_UNSUPPORTED with the reason (the caller composes the layer from per-expert gptq_forward calls instead).
 * flags: 0, or GPTQ_MOE_LOW_BIT: the grouped path (gptq_moe_build_table / gptq_moe_forward, gptq_moe_build_grad_table / gptq_moe_backward and their
 * describe / workspace twins) also takes 2- and 3-bit experts -- same contract, same workspace; gate and up still share their width, down may have
 * another (3-bit gate | up with 4-bit down is legal).  The decode and the batch path decline 2 / 3 bits whatever this flag says.
 * GPTQ_MOE_LOW_BIT_DECODE (independent of GPTQ_MOE_LOW_BIT; the two may be or-ed): the DECODE path (gptq_moe_build_decode_table /
 * gptq_moe_decode_forward and their describe / workspace twins, T <= 4) also takes 2- and 3-bit experts with a decode copy -- same contract, same
 * workspace, same plan keys; gate, up and down share one width there as at 4 / 8 bits.  The grouped and the backward entry points ignore it (flags 8 / 9
 * behave as 0 / 1); the batch, the prefill and the fused shared-expert entry points decline 2 / 3 bits whatever these two flags say.  Without the flag every
 * entry point answers as it did.  Unknown flag bits (2 and 4 among them): GPTQ_ERR_UNSUPPORTED from the grouped and the backward entry points.
 * GPTQ_MOE_LOW_BIT_BATCH (independent of the other two; they may be or-ed): the BATCH path (gptq_moe_batch_forward and its describe / workspace twins,
 * T <= 64) also takes 2- and 3-bit experts with a decode copy -- same contract, same launches, the workspace of the 4-bit set of the same (T, topk, E, H, I);
 * gptq_moe_build_decode_table then builds their table with this flag alone as well (the batch path's own checks apply: H and I multiples of 128, its group
 * sizes).  The decode, prefill and fused shared-expert entry points ignore the bit.  The grouped and the backward entry points keep refusing it with their
 * unknown-flag-bits message, as they did before it had a meaning: a caller that runs both paths on such experts keeps two gptq_moe_t over the same layer
 * arrays, one with the bit for the batch path (and its table build), one without for the rest (autogptq_amd/moe.py does).
 * GPTQ_MOE_LOW_BIT_PREFILL (independent of the other three; they may be or-ed): the PREFILL path (gptq_moe_prefill_forward and its describe / workspace
 * twins, any T up to GPTQ_MOE_PREFILL_MAX_ROWS routed rows) also takes 2- and 3-bit experts with a decode copy -- same contract, same launches
 * (moe_panel_lowbit_kernel), the workspace of the 4-bit set of the same (T, topk, E, H, I), the same plan keys and a trailing "bits=N";
 * gptq_moe_build_decode_table builds their table with this flag alone as well (without GPTQ_MOE_LOW_BIT_DECODE the check in front of the table is that of
 * the first copy path whose flag is set: batch, then prefill).  The decode, batch and fused shared-expert entry points ignore the bit; the grouped and the
 * backward entry points refuse it as an unknown flag bit, exactly as they do GPTQ_MOE_LOW_BIT_BATCH: the second gptq_moe_t of such a caller carries
 * whichever of the two copy-path bits are on. */
#define GPTQ_MOE_LOW_BIT 1
#define GPTQ_MOE_LOW_BIT_DECODE 8
#define GPTQ_MOE_LOW_BIT_BATCH 0x10
#define GPTQ_MOE_LOW_BIT_PREFILL 0x20
typedef struct gptq_moe_t {
    int32_t E;
    int32_t flags;                     /* 0 | GPTQ_MOE_LOW_BIT | GPTQ_MOE_LOW_BIT_DECODE | GPTQ_MOE_LOW_BIT_BATCH | GPTQ_MOE_LOW_BIT_PREFILL (the field was `reserved`, 0, before: a zeroed struct means what it meant) */
    const gptq_layer_t *const *gate;   /* [E] */
    const gptq_layer_t *const *up;     /* [E] */
    const gptq_layer_t *const *down;   /* [E] */
} gptq_moe_t;
/* The device table of per-expert pointers the kernels read (the launch arguments cannot hold E x 12 pointers): built once (post_init) into
 * gptq_moe_table_bytes(E) caller-owned device bytes; it synchronises `stream` (not capturable).  Rebuild it whenever a layer's buffers move. */
size_t gptq_moe_table_bytes(int E);
int gptq_moe_build_table(const gptq_moe_t *moe, void *table, void *stream);
/* Workspace of one call with T tokens:  GPTQ_WORKSPACE_HEADER_BYTES (left untouched: a workspace shared with the other entry points keeps its header)
 *   + a256(4 (E + 1)) + 256 + a256(16 tiles) + 2 a256(4 T topk) + a256(T topk I sizeof(T)) + a256(4 ksplit T topk H),   a256 = round up to 256;
 * tiles = floor(T topk / bm) + min(E, T topk) and bm / ksplit as gptq_describe_moe_plan reports them.  0 when the call is declined. */
size_t gptq_moe_workspace_bytes(const gptq_moe_t *moe, int T, int topk);
/* out[T, H] (layer dtype).  x [T, H] layer dtype, topk_idx [T, topk] int64, topk_w [T, topk] fp32, all contiguous, 16-byte aligned, on the experts' device.
 * h_out (optional, for tests): the sorted intermediate H_sorted [T topk, I] (layer dtype; rows grouped by expert in ascending order, each expert's rows in
 * the order of their assignments t topk + j) followed by pos [T, topk] int32 (the row of assignment (t, j), or -1), copied in stream order.
 * Four launches on the caller's stream, no allocation, no synchronisation, legal inside hipGraph capture; T = 0 launches nothing. */
int gptq_moe_forward(const gptq_moe_t *moe, const void *table, const void *x, const int64_t *topk_idx, const float *topk_w, int T, int topk, void *out,
                     void *h_out, void *workspace, size_t workspace_bytes, void *stream);
/* Host-only: "path=grouped bm=16 bn=64 tiles=2 ksplit=4 launches=4" or "path=per_expert reason=...", for (moe, T, topk).  GPTQ_OK either way
 * (GPTQ_ERR_NULL for a NULL out). */
int gptq_describe_moe_plan(const gptq_moe_t *moe, int T, int topk, char *out, size_t out_bytes);

/* The same layer at DECODE row counts, T <= 4, on the experts' decode copy (ABI 8): every expert layer carries qweight_tiled / qconst_tiled
 * (gptq_prepack_decode; act-order experts: built from qweight_seq, with perm), and the call runs on streaming kernels of the dense decode kernel's kind.
 *   ARITHMETIC: that of the dense decode-copy kernel, NOT "every W bit-exact to gptq_dequant" as on the grouped path: w - z exact in the layer dtype,
 *   products x (w - z) exact in fp32, fp32 sums over the 32 (8 bits: 16) consecutive k a lane holds, the group's scale applied to that fp32 sum; W is never
 *   rounded to the layer dtype.  silu and the product on the fp32 sums, h rounded once; out[t] = T(sum_j topk_w[t, j] (h_(t,j) . W2_e)) in fp32, ascending j,
 *   0 for a token with no valid expert.  Bit-reproducible; the row of token t does not depend on the other tokens of the call.
 *   TWO launches (gate|up + silu * mul; down + combine), no routing launch: every workgroup reads its expert from topk_idx and that expert's entry from the
 *   device table, so a captured graph replays with new routing.
 * Takes 4- and 8-bit fp16 / bf16 experts (2- and 3-bit ones with GPTQ_MOE_LOW_BIT_DECODE in moe->flags: same launches, workspace and plan), every group size the decode copy takes, plain and act-order (gate and up may have different activation orders:
 * each is gathered through its own perm; equal perm pointers -> one gather), T <= 4, topk <= 8, E <= 256, H and I multiples of 64, no bias.  Anything
 * else: GPTQ_ERR_UNSUPPORTED with the reason, and the caller keeps gptq_moe_forward / the per-expert composition.
 * Table: [3 projections][E] entries of 32 bytes {qweight_tiled, qconst_tiled, perm or NULL, 0}; gptq_moe_build_decode_table fills
 * gptq_moe_decode_table_bytes(E) = 3 E 32 caller-owned device bytes, synchronises `stream` (not capturable); rebuild it whenever a layer's buffers move. */
size_t gptq_moe_decode_table_bytes(int E);
int gptq_moe_build_decode_table(const gptq_moe_t *moe, void *table, void *stream);
/* GPTQ_WORKSPACE_HEADER_BYTES (left untouched) + a256(T topk I sizeof(T)) + a256(4 T topk): the h rows and pos.  0 when the call is declined. */
size_t gptq_moe_decode_workspace_bytes(const gptq_moe_t *moe, int T, int topk);
/* Arguments as gptq_moe_forward.  h_out (optional, for tests): H [T topk, I] in ASSIGNMENT order (row t topk + j; rows of dropped assignments are not
 * written) followed by pos [T, topk] int32 = that row, or -1 for a dropped assignment -- H[pos[t, j]] reads as with the grouped path.
 * Caller's stream, no allocation, no synchronisation, legal inside hipGraph capture (gptq_init() first: long act-order rows need its LDS grant);
 * T = 0 launches nothing. */
int gptq_moe_decode_forward(const gptq_moe_t *moe, const void *table, const void *x, const int64_t *topk_idx, const float *topk_w, int T, int topk, void *out,
                            void *h_out, void *workspace, size_t workspace_bytes, void *stream);
/* Host-only: "path=decode launches=2 wg_pair=1792 wg_down=256 waves_pair=8 waves_down=16 lds_pair=... lds_down=..." (workgroups, waves per workgroup and
 * dynamic LDS bytes of the two launches) or "path=none reason=..." (experts without a decode copy, T > 4, 2- / 3-bit without GPTQ_MOE_LOW_BIT_DECODE, fp32, topk > 8, ...).  GPTQ_OK either way. */
int gptq_describe_moe_decode_plan(const gptq_moe_t *moe, int T, int topk, char *out, size_t out_bytes);

/* The SHARED EXPERT of a Qwen-MoE block next to its routed experts (additive in ABI 8; transformers' Qwen2MoeSparseMoeBlock.forward):
 *   out[t] = T( sum_j topk_w[t, j] (h_(t,j) . W2_e)  +  s_t (hs_t . W2_s) ),   hs_t = T(silu(x_t . W1_s) * (x_t . W3_s)),   s_t = sigmoid(l_t),
 *   l_t = T(sum_k x_t[k] w_g[k]): fp32 products and sums in an order that depends on H alone (the router kernel's: lane l of one wave takes the 16-byte
 *   pieces l, l + 64, .. in ascending order, then a butterfly), rounded ONCE to the layer dtype as gptq_moe_router rounds its logits; the sigmoid is
 *   1 / (1 + exp(-l_t)) in fp32.  gate_w == NULL: s_t = 1 (the DeepSeek form of a shared expert).
 * gate / up are [H -> I_s], down is [I_s -> H]; every token takes them.
 *
 * gptq_moe_shared_decode_forward, T <= 4: the TWO launches of gptq_moe_decode_forward in their shared form, with that call's arithmetic contract (w - z
 * exact, products exact in fp32, per-run fp32 sums on the matrix core, the scale applied to the sum, W never rounded; no atomics, no K slices;
 * bit-reproducible, row t independent of the other tokens, capturable).
 *   launch 1  the routed grid plus, per token, ceil(I_s / I) grid rows of I / 16 workgroups: row q, column c serves strip q (I / 16) + c of I_s (strips
 *             past I_s / 16 leave at once); the shared workgroup of strip 0 also writes s_t from the row of x it has staged.
 *   launch 2  grid (H / 16, T) as before; behind the token's topk routed assignments (ascending j) the workgroup adds s_t (hs_t . W2_s) to the same fp32
 *             register and rounds once.  The routed terms are summed exactly as gptq_moe_decode_forward sums them.  A token with no valid routed
 *             expert gets T(s_t (hs_t . W2_s)).
 * Takes what gptq_moe_decode_forward takes for `moe` at 4 and 8 bits (2- / 3-bit routed experts are declined whatever moe->flags says), and shared layers with a decode copy, 4 or 8 bits, fp16 / bf16, plain or act-order.  Declined with
 * GPTQ_ERR_UNSUPPORTED and the reason: shared gate / up (down) that differ from the routed gate / up (down) in bits or dtype, I_s % 64 != 0, a bias or an
 * epilogue on a shared layer, a shared layer without a decode copy or with a group size the copy does not take, shared gate and up of different group
 * sizes, either launch's LDS layout above 160 KiB, gate_w not 16-byte aligned, flags or reserved != 0. */
typedef struct gptq_moe_shared_t {
    const gptq_layer_t *gate, *up, *down;   /* [H -> I_s], [H -> I_s], [I_s -> H], with decode copies */
    const void *gate_w;                     /* [H] layer dtype, 16-byte aligned, or NULL (s = 1) */
    int32_t flags, reserved;                /* 0 */
} gptq_moe_shared_t;
/* gptq_moe_decode_workspace_bytes(moe, T, topk) + a256(T I_s sizeof(T)) + a256(4 T): the decode path's h rows and pos, then hs [T, I_s] and s [T] fp32.
 * The GPTQ_WORKSPACE_HEADER_BYTES in front are left untouched.  0 when the call is declined. */
size_t gptq_moe_shared_decode_workspace_bytes(const gptq_moe_t *moe, const gptq_moe_shared_t *shared, int T, int topk);
/* Arguments as gptq_moe_decode_forward (decode_table: gptq_moe_build_decode_table of `moe`; the shared layers need no table).  h_out (optional, for
 * tests), at byte offsets  0: H [T topk, I] in assignment order;  T topk I sizeof(T): pos [T, topk] int32;  + 4 T topk: Hs [T, I_s];
 * + T I_s sizeof(T): s [T] fp32 -- copied in stream order.  Caller's stream, no allocation, no synchronisation, legal inside hipGraph capture
 * (gptq_init() first); T = 0 launches nothing. */
int gptq_moe_shared_decode_forward(const gptq_moe_t *moe, const gptq_moe_shared_t *shared, const void *decode_table, const void *x, const int64_t *topk_idx,
                                   const float *topk_w, int T, int topk, void *out, void *h_out, void *workspace, size_t workspace_bytes, void *stream);
/* Host-only: "path=decode_shared launches=2 wg_pair=... wg_down=... waves_pair=... waves_down=... lds_pair=... lds_down=..." (wg_pair =
 * T topk (I / 16) + T (I_s / 16): the workgroups that do work) or "path=none reason=...".  GPTQ_OK either way (GPTQ_ERR_NULL for a NULL out). */
int gptq_describe_moe_shared_decode_plan(const gptq_moe_t *moe, const gptq_moe_shared_t *shared, int T, int topk, char *out, size_t out_bytes);
/* The same tail at ANY token count, in place on the routed output: out[t, :] = T(float(out[t, :]) + s_t float(ys[t, :])), s_t as above from x [T, H] and
 * gate_w [H] (NULL: s_t = 1, x is not read), ys [T, H] the shared expert's output; all in `dtype` (GPTQ_F16 / GPTQ_BF16), contiguous, 16-byte aligned.
 * ONE launch, one workgroup per token, H % 8 == 0, no workspace, no atomics, bit-reproducible, legal inside hipGraph capture; T = 0 launches nothing. */
int gptq_moe_shared_combine(const void *x, const void *gate_w, const void *ys, void *out, int T, int H, int dtype, void *stream);

/* The same layer at BATCHED-DECODE row counts, 1 <= T <= 64 (additive in ABI 8), on the experts' decode copy: the arithmetic of gptq_moe_forward (every W
 * bit-exact to gptq_dequant, fp32 products and sums on the matrix core, h rounded once, out[t] = T(sum_j topk_w[t, j] y_(t, j)) in ascending j), on kernels
 * of the dense batched-decode kind: a workgroup = one tile of up to 16 rows of one expert x 4 strip-chunks x the whole K, no K slices, no atomics --
 * bit-reproducible, and the row of token t does not depend on the other tokens of the call.
 *   Launches: routing (bm = 16), gate|up + silu * mul, down, combine: FOUR; sets with act-order experts add one row gather through perm in front of either
 *   GEMM (five or six).  No host round trip; the grid is a bound from (T, topk, E), so a captured graph replays with new routing.
 * Takes 4- and 8-bit fp16 / bf16 experts (2- and 3-bit ones with GPTQ_MOE_LOW_BIT_BATCH in moe->flags: same launches and workspace; moe_rows_lowbit_kernel
 * reads their copy in place), plain or act-order (gate and up may have different activation orders), group_size 32, 64, 128 2^n or one group,
 * H and I multiples of 128, E <= 256, topk <= 8, no bias, every expert with its decode copy.  Anything else: GPTQ_ERR_UNSUPPORTED with the reason.
 * `table` is the DECODE table (gptq_moe_build_decode_table): there is no table of its own.
 * Workspace of one call:  GPTQ_WORKSPACE_HEADER_BYTES (left untouched)
 *   + a256(4 (E + 1)) + 256 + a256(16 tiles) + 2 a256(4 T topk) + a256(T topk I sizeof(T)) + a256(4 T topk H) + a256(2 T topk H sizeof(T)) + a256(T topk I sizeof(T)),
 * a256 = round up to 256, tiles = floor(T topk / 16) + min(E, T topk): offsets, tile count, tiles, pos, sorted rows, H_sorted, Y, and the two gathered
 * operands of act-order sets (reserved for every set: the size depends on (T, topk, E, H, I) alone).  0 when the call is declined. */
size_t gptq_moe_batch_workspace_bytes(const gptq_moe_t *moe, int T, int topk);
/* Arguments as gptq_moe_forward, except that `table` is the decode table.  h_out (optional, for tests): H_sorted [T topk, I] (rows grouped by expert, as on
 * the grouped path) followed by pos [T, topk] int32.  Caller's stream, no allocation, no synchronisation, legal inside hipGraph capture (gptq_init() first:
 * act-order sets need its LDS grant); T = 0 launches nothing. */
int gptq_moe_batch_forward(const gptq_moe_t *moe, const void *table, const void *x, const int64_t *topk_idx, const float *topk_w, int T, int topk, void *out,
                           void *h_out, void *workspace, size_t workspace_bytes, void *stream);
/* Host-only: "path=batch bm=16 s=4 tiles=10 launches=4 waves_pair=8 waves_down=8 lds_pair=... lds_down=..." (s: strip-chunks per wave and chunk -- the pair
 * form runs 2 strips of W1 and of W3, the down form 4 of W2; 2- / 3-bit experts taken under GPTQ_MOE_LOW_BIT_BATCH: the same keys and a trailing "bits=3")
 * or "path=none reason=..." (no decode copy, T > 64, 2- / 3-bit without GPTQ_MOE_LOW_BIT_BATCH, fp32, ...).  GPTQ_OK either way. */
int gptq_describe_moe_batch_plan(const gptq_moe_t *moe, int T, int topk, char *out, size_t out_bytes);

/* PREFILL path of the routed layer (additive in ABI 8): the same formulas and arithmetic contract on the experts' DECODE COPY at ANY token count (the Python
 * layer uses it from 65 tokens on), on kernels of the dense panel kind: a workgroup = one tile of up to 64 rows of one expert x a column tile x the whole K;
 * its waves are K parts that meet once in LDS in wave order; no K slices, no atomics, nothing exchanged between workgroups -- bit-reproducible, and the row
 * of token t does not depend on the other tokens of the call (the K split is a function of the layers alone).
 *   Launches: routing (bm = 64), x into sorted order (act-order sets: through W1's and W3's perm, two planes), gate|up + silu * mul, down, combine: FIVE;
 *   sets with act-order down projections add the gather of H_sorted through W2's perm (six).  No host round trip; the grid is a bound from (T, topk, E),
 *   so a captured graph replays with new routing.
 * Takes 4- and 8-bit fp16 / bf16 experts (2- and 3-bit ones with GPTQ_MOE_LOW_BIT_PREFILL in moe->flags: same launches and workspace;
 * moe_panel_lowbit_kernel reads the copy's 8- / 12-byte lanes in place), plain or act-order, group_size 64 2^n or one group, H and I multiples of 128, E <= 256, topk <= 8,
 * T topk <= 65535, no bias, every expert with its 16-byte aligned decode copy.  Anything else: GPTQ_ERR_UNSUPPORTED with the reason.
 * `table` is the DECODE table (gptq_moe_build_decode_table).
 * Workspace of one call:  GPTQ_WORKSPACE_HEADER_BYTES (left untouched)
 *   + a256(4 (E + 1)) + 256 + a256(16 tiles) + 2 a256(4 T topk) + a256(planes T topk H sizeof(T)) + a256(T topk I sizeof(T)) + a256(4 T topk H)
 *   [+ a256(T topk I sizeof(T)) for act-order down projections],
 * a256 = round up to 256, tiles = floor(T topk / 64) + min(E, T topk), planes = 2 for act-order gate / up layers, else 1: offsets, tile count, tiles, pos,
 * sorted rows, x_sorted, H_sorted, Y, gathered H.  0 when the call is declined. */
size_t gptq_moe_prefill_workspace_bytes(const gptq_moe_t *moe, int T, int topk);
/* Arguments and status codes as gptq_moe_batch_forward.  h_out (optional, for tests): H_sorted [T topk, I] (rows grouped by expert) followed by pos
 * [T, topk] int32.  Caller's stream, no allocation, no synchronisation, legal inside hipGraph capture (gptq_init() first: the kernels need its LDS grant);
 * T = 0 launches nothing. */
int gptq_moe_prefill_forward(const gptq_moe_t *moe, const void *table, const void *x, const int64_t *topk_idx, const float *topk_w, int T, int topk, void *out,
                             void *h_out, void *workspace, size_t workspace_bytes, void *stream);
/* Host-only: "path=prefill bm=64 launches=5 tiles=72 nt_pair=2 nt_down=4 waves=8 waves_pair=8 spw_pair=8 spw_down=28 lds=131072" (nt: 32-column blocks per
 * workgroup -- the pair form runs nt_pair blocks of W1 and of W3, the down form nt_down of W2; waves_pair = 4 for act-order gate / up layers; spw: 64-deep
 * steps per wave; 2- / 3-bit experts taken under GPTQ_MOE_LOW_BIT_PREFILL: the same keys and a trailing "bits=3") or "path=none reason=..." (no decode
 * copy, 2- / 3-bit without GPTQ_MOE_LOW_BIT_PREFILL, fp32, 32-wide groups, ...).  GPTQ_OK either way. */
int gptq_describe_moe_prefill_plan(const gptq_moe_t *moe, int T, int topk, char *out, size_t out_bytes);

/* BACKWARD of the routed layer (additive in ABI 8): the gradients of gptq_moe_forward's formulas with respect to x and topk_w, from the packed weights.
 * Given dout [T, H] in the experts' dtype T, for every valid assignment r = (t, j) with expert e:
 *   d_r     = dout[t] . W2_e^T                          fp32 sums over H, every W bit-exact to gptq_dequant
 *   dw[t,j] = sum_i d_r[i] h_r[i]                       fp32, fixed order; h_r = T(silu(g_r) u_r)
 *   dg_r    = T(w[t,j] d_r u_r silu'(g_r))              silu'(g) = s (1 + g (1 - s)), s = 1 / (1 + exp(-g)), on fp32, one rounding
 *   du_r    = T(w[t,j] d_r silu(g_r))
 *   dx[t]   = T(sum_j (dg_r . W1_e^T + du_r . W3_e^T))  fp32, ascending j, one rounding
 * Nothing is saved by the forward: g_r = T(x_t . W1_e), u_r = T(x_t . W3_e) are recomputed (the grouped GEMM's fp32 sums, rounded once).  Dropped
 * assignments give dw = 0 and contribute nothing; a token without a valid expert gets a zero dx row.  No atomics, fixed summation orders: bit-reproducible
 * and independent of the tiling.  Takes exactly what gptq_moe_forward takes; anything else is GPTQ_ERR_UNSUPPORTED with the reason.
 *   Launches: routing (64-row tiles), recompute of g / u (the forward's grouped GEMM, reading `table`), down stage (d, dg, du, dw partials), up stage
 *   (fp32 rows of dx per assignment), combine: FIVE (four when dx is NULL).  The down and up stages read the CHECKPOINT rows (qweight with g_idx, as
 *   gptq_grad_input does) through a table of their own: [3 projections][E] entries of 32 bytes {qweight, qzeros, scales, g_idx or NULL};
 *   gptq_moe_build_grad_table fills gptq_moe_grad_table_bytes(E) = 3 E 32 caller-owned device bytes, synchronises `stream` (not capturable); rebuild it
 *   whenever a layer's buffers move. */
size_t gptq_moe_grad_table_bytes(int E);
int gptq_moe_build_grad_table(const gptq_moe_t *moe, void *table, void *stream);
/* Workspace of one call:  GPTQ_WORKSPACE_HEADER_BYTES (left untouched)
 *   + a256(4 (E + 1)) + 256 + a256(16 tiles) + 2 a256(4 T topk) + 2 a256(T topk I sizeof(T)) + a256(4 T topk ceil(I / 128)) + a256(4 T topk H),
 * a256 = round up to 256, tiles = floor(T topk / 64) + min(E, T topk): offsets, tile count, tiles, pos, sorted rows, G and U (overwritten by dg and du),
 * the dw partials, and the fp32 dx rows per assignment.  0 when the call is declined. */
size_t gptq_moe_backward_workspace_bytes(const gptq_moe_t *moe, int T, int topk);
/* dx [T, H] (layer dtype) or NULL, dw [T, topk] fp32 or NULL (both NULL: GPTQ_ERR_NULL).  x, topk_idx, topk_w as gptq_moe_forward took them, dout [T, H]
 * layer dtype; x, dout, dx and the workspace 16-byte aligned.  `table` is the forward table (gptq_moe_build_table), `grad_table` the one above.
 * dgu_out (optional, for tests): the kernel's dg rows [T topk, I], then its du rows [T topk, I] (layer dtype, rows grouped by expert as H_sorted), then
 * pos [T, topk] int32, copied in stream order.  Caller's stream, no allocation, no synchronisation, legal inside hipGraph capture; the grids are bounds
 * from (T, topk, E) alone, so a captured graph replays with new routing.  T = 0 launches nothing. */
int gptq_moe_backward(const gptq_moe_t *moe, const void *table, const void *grad_table, const void *x, const int64_t *topk_idx, const float *topk_w,
                      const void *dout, int T, int topk, void *dx, float *dw, void *dgu_out, void *workspace, size_t workspace_bytes, void *stream);
/* Host-only: "path=grouped_backward tiles=3 launches=5 wg_recompute=... wg_down=... wg_up=..." or "path=per_expert reason=...", for (moe, T, topk).
 * GPTQ_OK either way (GPTQ_ERR_NULL for a NULL out). */
int gptq_describe_moe_backward_plan(const gptq_moe_t *moe, int T, int topk, char *out, size_t out_bytes);

/* The ROUTER in front of the routed layer (additive in ABI 8): logits, softmax and top-k of a softmax-then-top-k router (Mixtral, Qwen2-MoE, Qwen3-MoE) in
 * ONE launch.  The router weight is not quantized (auto_gptq/modeling/mixtral.py lists only w1 / w2 / w3 and the attention projections): a dense kernel.
 * For x [T, H] and w [E, H] in the layer dtype D (fp16 or bf16):
 *   Logits.     l[t, e] = D(sum_k x[t, k] w[e, k]): fp32 products and sums in a fixed order, one rounding to D -- F.linear in D up to summation order.
 *               Everything below is a function of these rounded logits alone.
 *   Selection.  topk times, take the largest remaining logit; equal logits go to the LOWER expert index.  topk_idx [T, topk] (int64) is in that order:
 *               descending logit, then ascending index (sorted=True).  -0 equals +0 and a NaN ranks above every number, as in torch.sort.  Indices are
 *               always distinct and inside [0, E), whatever the input holds (NaN or Inf rows included).  These are the experts torch.topk on the fp32
 *               probabilities picks, except where that call's own tie order is undefined (equal logits, or probabilities that round to the same fp32).
 *   Weights.    p_e = exp(l_e - max_e l) / sum_e exp(l_e - max_e l) in fp32, fixed summation order; topk_w[t, j] = p_sel(j).  With GPTQ_ROUTER_RENORM,
 *               topk_w[t, j] = p_sel(j) / sum_j p_sel(j), summed in ascending j.  fp32 [T, topk]: the layout gptq_moe_*forward takes.
 *   logits_out  [T, E] in D, the rounded logits (the auxiliary loss and output_router_logits need them), or NULL.
 * No workspace, no atomics, no exchange between workgroups: bit-reproducible and legal inside hipGraph capture.  A workgroup owns its tokens' whole rows
 * of logits; softmax and selection run in its epilogue.  Two launch-uniform row regimes: 9+ tokens, 16 tokens x all experts per workgroup on
 * v_mfma_f32_16x16x32 (8 waves split the k-steps and meet in LDS in wave order); 1..8 tokens, one token per workgroup (x staged in LDS, waves take experts
 * round robin).  Within a regime a token's bits depend on nothing but its own row; the regimes sum in different orders.
 * Takes D in {fp16, bf16} (the same for x and w), 1 <= E <= 256, 1 <= topk <= min(E, 8), H % 64 == 0 (and a staged row within 64 KiB of LDS), all pointers
 * 16-byte aligned and contiguous.  Anything else: GPTQ_ERR_UNSUPPORTED with the reason, nothing launched.  Unknown flag bits: GPTQ_ERR_UNSUPPORTED.
 * GPTQ_ERR_NULL for a NULL x / w / topk_idx / topk_w.  T = 0 launches nothing. */
#define GPTQ_ROUTER_RENORM 1
int gptq_moe_router(const void *x, const void *w, int T, int H, int E, int topk, int dtype, int flags, void *logits_out, int64_t *topk_idx, float *topk_w,
                    void *stream);
/* Host-only: "path=router form=rows|tiles wg=... waves=8 lds=... launches=1" or "path=none reason=...".  GPTQ_OK either way (GPTQ_ERR_NULL for a NULL out). */
int gptq_describe_moe_router_plan(int T, int H, int E, int topk, int dtype, int flags, char *out, size_t out_bytes);

/* The GROUPED-SIGMOID form of the router (additive in ABI 8): the router of DeepSeek-V3 / R1 and GLM-4.5 / 4.6 MoE blocks (transformers'
 * DeepseekV3TopkRouter / Glm4MoeTopkRouter: fp32 linear, sigmoid, correction bias, group-limited top-k, gather, renormalise, scale) in ONE launch of the
 * same kernels.  For x [T, H] and w [E, H] in D (fp16 or bf16), bias [E] fp32 or NULL, G = n_group, kg = topk_group, Eg = E / G:
 *   Logits.     l[t, e] = sum_k x[t, k] w[e, k]: fp32 products and sums in the fixed orders of the two row regimes, NOT rounded to D (the reference
 *               casts x and w to fp32 first).
 *   Scores.     s_e = 1 / (1 + expf(-l_e)) in fp32; c_e = s_e + bias_e, one fp32 add (NULL bias: c_e = s_e).
 *   Groups.     Only when G > 1: group g holds the experts [g Eg, (g + 1) Eg); its score is the fp32 sum of its two largest c (one add: largest plus
 *               second largest).  The kg groups with the largest score stay; equal scores go to the LOWER group index.
 *   Selection.  Among the experts of the groups that stay, topk times the largest remaining c; equal c goes to the LOWER expert index.  topk_idx [T, topk]
 *               (int64) is in that order: descending c, then ascending index.  -0 equals +0 and a NaN ranks above every number, for c and for the group
 *               scores alike.  Indices are always distinct, inside [0, E) and inside the groups that stay, whatever the input holds.
 *   Weights.    topk_w[t, j] = s_sel(j): the score WITHOUT the bias, as in the reference.  With GPTQ_ROUTER_RENORM divided by
 *               (sum_j s_sel(j), in ascending j) + 1e-20.  Then multiplied by scale, the routed scaling factor (1.0 for none).  fp32 [T, topk].
 *   logits_out  fp32 [T, E], the logits, or NULL.      scores_out  fp32 [T, E], s, or NULL.
 * Given s, everything after the sigmoid is single fp32 adds and comparisons: a host can reproduce the selection bit for bit.
 * As gptq_moe_router: no workspace, no atomics, no exchange between workgroups; bit-reproducible, legal inside hipGraph capture; the same two row regimes
 * (1..8 tokens: one token per workgroup; 9+: 16 tokens x all experts on v_mfma_f32_16x16x32), within which a token's bits depend on its own row only.
 * Takes D in {fp16, bf16}, H % 64 == 0 (and a staged row within 64 KiB of LDS), 1 <= E <= 256, 1 <= topk <= 8, 1 <= kg <= G <= 32, E % G == 0, Eg >= 2
 * when G > 1, topk <= kg Eg, flags within {0, GPTQ_ROUTER_RENORM}, a finite scale; x, w and the outputs 16-byte aligned and contiguous, bias 4-byte
 * aligned.  Anything else: GPTQ_ERR_UNSUPPORTED with the reason, nothing launched.  GPTQ_ERR_NULL for a NULL x / w / topk_idx / topk_w; T < 0 is
 * GPTQ_ERR_SHAPE; T = 0 validates and launches nothing. */
int gptq_moe_router_grouped(const void *x, const void *w, const float *bias, int T, int H, int E, int topk, int n_group, int topk_group, float scale,
                            int dtype, int flags, float *logits_out, float *scores_out, int64_t *topk_idx, float *topk_w, void *stream);
/* Host-only: "path=router_grouped form=rows|tiles wg=... waves=8 lds=... groups=... launches=1" or "path=none reason=...".  GPTQ_OK either way
 * (GPTQ_ERR_NULL for a NULL out). */
int gptq_describe_moe_router_grouped_plan(int T, int H, int E, int topk, int n_group, int topk_group, int dtype, int flags, char *out, size_t out_bytes);

/* Integer unpack (bit-exact targets). w_out uint8 [K,N]; z_out int32 [G,N] (zero-point as used). */
int gptq_unpack_weights(const uint32_t *qweight, int K, int N, int bits, uint8_t *w_out, void *stream);
int gptq_unpack_zeros(const uint32_t *qzeros, int G, int N, int bits, int zero_mode, int32_t *z_out, void *stream);

/* Device pack(): intweight[k,n] = round((W[n,k] + zero[g,n]*scale[g,n]) / scale_cast[g,n]) packed
 * along K exactly like the reference (fields OR-ed unmasked).  W is [N,K] in w_dtype; scale_in /
 * zero_in are [G,N] in qparam_dtype (already transposed); scales_out [G,N] in w_dtype receives the
 * cast scales.  g_idx NULL = sequential. */
int gptq_pack_weights(const void *W, const void *scale_in, const void *zero_in, const int32_t *g_idx,
                      int K, int N, int bits, int group_size, int w_dtype, int qparam_dtype,
                      uint32_t *qweight_out, void *scales_out, void *stream);
int gptq_pack_zeros(const void *zero_in, int G, int N, int bits, int qparam_dtype,
                    uint32_t *qzeros_out, void *stream);

/* Act-order support.  HOST function: stable counting sort of k by g_idx (host pointers).
 * perm_out[i] = original k at sorted position i.  *uniform_out = 1 iff sorted position i has
 * group i / group_size for every i (then the fast kernels can use qweight_seq + perm). */
int gptq_make_sequential(const int32_t *g_idx_host, int K, int group_size,
                         int32_t *perm_out_host, int *uniform_out);
/* HOST function: every g_idx[k] must name an existing group, 0 <= g_idx[k] < G (G = rows of scales / qzeros).  The kernels
 * index scales / qzeros with raw g_idx values on act-order layers; the reference's torch indexing raises on a bad index
 * (qlinear_cuda.py:302 `self.scales[self.g_idx.long()]`), this is the same check for a C caller.  GPTQ_ERR_SHAPE on violation. */
int gptq_validate_g_idx(const int32_t *g_idx_host, int K, int G);
/* qweight_seq[row-order = perm] from qweight; device pointers. */
int gptq_resequence_qweight(const uint32_t *qweight, const int32_t *perm, int K, int N, int bits,
                            uint32_t *qweight_seq_out, void *stream);
/* The decode copy of a 2-, 3-, 4- or 8-bit layer (layouts: gptq_layer_t.qweight_tiled / qconst_tiled): exact integer re-arrangements of the packed fields, the
 * scales (bit copies) and the zero-points (the value the kernels subtract, zero_mode applied), written to caller-owned buffers of
 * gptq_prepack_decode_bytes() bytes.  Source: layer->qweight_seq when present, else layer->qweight; layer->qweight_tiled / qconst_tiled / tiled_cols
 * are ignored.  Needs bits 2 / 3 / 4 / 8 (2 bits: no fused epilogue), fp16 / bf16, group_size = KPL times a power of two (or group_size >= K), K % 32 == 0, N % 16 == 0, no raw act-order;
 * otherwise GPTQ_ERR_UNSUPPORTED (and sizes 0).  The role of the reference's load-time re-layouts -- exllamav2 shuffle_kernel
 * (exllamav2/cuda/q_matrix.cu:19-42, called :149), exllama make_sequential (exllama/cuda_func/q4_matrix.cu:105-169), Marlin's repack kernel
 * (marlin/marlin_repack.cu:8-92) -- without touching the checkpoint tensors. */
int gptq_prepack_decode_bytes(const gptq_layer_t *layer, size_t *tiled_bytes, size_t *const_bytes);
int gptq_prepack_decode(const gptq_layer_t *layer, uint32_t *qweight_tiled_out, void *qconst_tiled_out, void *stream);
/* The exact inverse of the weights half (round 5): qweight_out [K/32*bits, N] = the packed rows the copy was made from (qweight, or qweight_seq of an act-order
 * layer), bit for bit.  What lets ONE copy of the weights stay on the device -- the reference's fast backends re-lay their weights IN PLACE
 * (exllama/cuda_func/q4_matrix.cu:160, exllamav2/cuda/q_matrix.cu:149) -- while state_dict() / a re-save / the kernels that read rows are still served:
 * QuantLinear.post_init(release_checkpoint_layout=True) moves qweight to host memory and rebuilds rows into a shared scratch only for calls that need them. */
int gptq_unprepack_decode(const uint32_t *qweight_tiled, int K, int N, int bits, uint32_t *qweight_out, void *stream);
/* x_out[m, i] = x[m, perm[i]] */
int gptq_permute_columns(const void *x, const int32_t *perm, int M, int K, int dtype, void *x_out, void *stream);

/* Host-only introspection: which kernel and launch geometry gptq_forward_ex would use for (layer, M, tuning), written as a
 * short "key=value ..." line into out (NUL-terminated, truncated to out_bytes).  No device work, no pointer is dereferenced
 * except the struct fields; returns GPTQ_OK or the validation status gptq_forward_ex would return.  Examples:
 *   "path=gemv kernel=mfma ln=4 waves=16 u=2 ksplit=1 mt=1 strips=256 pair=0 perm=0"
 *   "path=gemm kernel=tiled mt=4 bk=64 kg=2 ksplit=1 tiles=16x16 perm=1 dma=1"
 * (the reference's dispatch thresholds, SURVEY §8 a15, are constants in its sources; here they are queryable.) */
int gptq_describe_plan(const gptq_layer_t *layer, int M, const gptq_tuning_t *tuning, char *out, size_t out_bytes);
/* Host-only, beside gptq_describe_plan (whose line is pinned byte for byte by tests/test_forward_entry_contract.py and so does not grow): in how many steps the
 * decode-copy kernel ("kernel=strips") stages x and the constants for (layer, M, tuning) -- 2: a plain 4-bit fp16 launch without K slices that is deeper than one
 * pass of its workgroup (waves * u chunks) stages only that pass's part in front of the first weight burst and the rest behind it; 1: every other decode-copy
 * launch; 0: another kernel, or arguments gptq_describe_plan would refuse.  The Python wrapper reports it as "xstage" of describe_plan(). */
int gptq_describe_plan_xstage(const gptq_layer_t *layer, int M, const gptq_tuning_t *tuning);

/* ---- AWQ checkpoint ingest (4-bit only, as the reference: auto_gptq/modeling/_utils.py:525-701) ----------------
 * AWQ side: awq_qweight u32 [K, N/8] (nibble p of word c = column 8c + {0,2,4,6,1,3,5,7}[p]), awq_qzeros u32 [G, N/8]
 * (same order, raw zero-point, no -1), awq_scales fp16 [G, N] (= the GPTQ `scales` tensor, passed through unchanged).
 *
 * gptq_awq_unpack replaces unpack_awq (_utils.py:556-621): weight_kn_out fp16 [K, N] =
 *   half(w * s) - half(z * s)   (each product and the difference rounded to fp16 once, the reference's op order);
 *   the reference returns its transpose view [N, K].  zeros_out int8 [G, N] = the raw zero-points in natural column order.
 * gptq_awq_repack is unpack_awq + pack_from_tensors (_utils.py:624-701) as one integer pass: GPTQ qweight_out u32 [K/8, N]
 *   (nibble j of word r = w[8r + j, n]) and qzeros_out u32 [G, N/8] (field = (z - 1) & 15).  Identical to the reference's
 *   fp16 round trip whenever that round trip is faithful (finite, normal scales; tests/golden/awq_*.npz). */
int gptq_awq_unpack(const uint32_t *awq_qweight, const uint32_t *awq_qzeros, const void *awq_scales, int K, int N,
                    int group_size, void *weight_kn_out, int8_t *zeros_out, void *stream);
int gptq_awq_repack(const uint32_t *awq_qweight, const uint32_t *awq_qzeros, int K, int N, int group_size,
                    uint32_t *qweight_out, uint32_t *qzeros_out, void *stream);

/* ---- direct peer-store all-gather for out_features-parallel layers; experimental, off by default ----------
 * The reference runs a layer on one GPU only (tests/test_q4.py:1224-1226: `test_multigpu` is a TODO); the column split is the
 * property its fused q/k/v caller relies on (fused_llama_attn.py:171-186).  Rank r of T computes out[:, r*N/T : (r+1)*N/T]; the
 * exchange below replaces the ring all-gather behind it on a point-to-point fabric: every rank stores its [M, N/T] slice into the
 * exchange buffer of EVERY rank (one xGMI link per peer), raises a flag there, waits for the T flags of its own buffer and copies
 * the gathered [M, N] rows to `out`.
 *
 * The caller owns all memory: per rank two exchange buffers [rows_max, N] (they alternate by call parity), uint32
 * flags[GPTQ_PEER_MAX] and uint32 state[4], the last two zeroed once; the buffers and flags of the peers are mapped into the
 * caller's address space (hipIpcOpenMemHandle / the framework's IPC) and listed in gptq_peer_group_t in RANK order (entry `rank` =
 * the caller's own).  Across GPUs buffers and flags must be fine-grained allocations.  Calls are collective: every rank issues
 * the same sequence of gathers with the same M.  Two launches per gather, no host state per call (legal under hipGraph capture,
 * and a captured graph replays: the call epoch lives in state[0]).  state[3] != 0 afterwards = a wait gave up after
 * `max_spins` polls (a peer never arrived) and `out` is incomplete -- the kernels never spin unbounded. */
#define GPTQ_PEER_MAX 8
typedef struct gptq_peer_group_t {
    void     *xbuf[2][GPTQ_PEER_MAX];  /* xbuf[p][r]: exchange buffer of parity p of rank r, [rows_max, N] dtype */
    uint32_t *flags[GPTQ_PEER_MAX];    /* flags[r]: rank r's arrival flags, uint32[GPTQ_PEER_MAX] */
    uint32_t *state;                   /* this rank's uint32[4]: gathers completed, two tickets, timeout raised */
    int32_t world, rank;               /* 1 <= world <= GPTQ_PEER_MAX */
    int32_t rows_max, N;               /* geometry of the exchange buffers; N = out_features of the full layer */
} gptq_peer_group_t;

/* scatter: y_local [M, n_local] (n_local = N / world) -> columns [rank*n_local, (rank+1)*n_local) of every rank's exchange
 * buffer, then the arrival flags.  collect: wait for all ranks' slices of this call, copy [M, N] to `out`, advance the epoch.
 * gather = scatter + collect.  Independent work of the caller may be enqueued between scatter and collect -- ON THE SAME STREAM: every collect
 * (re-)publishes this rank's arrival flag of its epoch when it starts (that is what lets gptq_forward_scatter go without a flag of its own), which is only
 * correct behind the rank's payload stores in stream order.  A scatter on one stream and its collect on another -- or a collect enqueued first -- raises
 * the flag over an incomplete payload and the peers copy stale rows without any error. */
int gptq_peer_scatter(const gptq_peer_group_t *pg, const void *y_local, int M, int n_local, int dtype, void *stream);
int gptq_peer_collect(const gptq_peer_group_t *pg, void *out, int M, int dtype, uint32_t max_spins, void *stream);
int gptq_peer_gather(const gptq_peer_group_t *pg, const void *y_local, void *out, int M, int n_local, int dtype,
                     uint32_t max_spins, void *stream);
/* The scatter as the EPILOGUE of the rank's decode kernel (round 4): layer = this rank's column shard (layer->N = pg->N / world) carrying its decode copy,
 * M <= 4.  The strip owners of the decode-copy kernel store their [M][16] outputs straight into every rank's exchange buffer (16-byte system-scope
 * write-through stores) -- no y_local, no scatter launch: a tensor-parallel layer is the local kernel + ONE collect.  The rank's arrival flag is raised by
 * the first block of its gptq_peer_collect launch (every collect (re-)publishes the flag of its epoch before it waits: behind this kernel in stream order
 * the payload is complete); gptq_peer_publish raises it on its own -- needed only when several ranks share ONE stream (simulations: each rank's collect
 * would wait for flags that later launches of the same stream raise) or when unrelated work sits between the scatter and the collect.
 * workspace as for gptq_forward (gptq_workspace_bytes(layer, M)).  GPTQ_ERR_UNSUPPORTED when the layer / M does not qualify (then: gptq_forward +
 * gptq_peer_scatter).  gptq_forward_gather = gptq_forward_scatter + gptq_peer_collect.  Same collective contract as gptq_peer_gather. */
int gptq_forward_scatter(const gptq_layer_t *layer, const void *x, int M, const gptq_peer_group_t *pg, void *workspace, size_t workspace_bytes,
                         void *stream);
int gptq_forward_gather(const gptq_layer_t *layer, const void *x, void *out, int M, const gptq_peer_group_t *pg, uint32_t max_spins, void *workspace,
                        size_t workspace_bytes, void *stream);
int gptq_peer_publish(const gptq_peer_group_t *pg, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPTQ_MI355X_H */
