/*
 * woq_hip.h — C ABI of libwoq_hip.so, the MI355X (gfx950) replacement for the reference's
 * `qbits_py` operator module on the int4 weight-only-quantized linear path.
 *
 * Every entry point below replaces one function of the reference boundary
 *   intel_extension_for_transformers/qbits/qbits.cpp:192-206   (PYBIND11_MODULE qbits_py)
 * or, for the ops between the linears, one stock-HF module forward that the reference executes
 * on the CPU. The reference-side binding a maintainer would add is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; every `*_dev` / `const void*` tensor argument is a DEVICE pointer owned by
 *    the caller (torch allocates it); the library never frees or keeps caller memory, except the
 *    pointers stored in a woq_engine, which must outlive it (same rule as the reference's
 *    set_woq_workspace, bestla_weightonly_dispatcher.cpp:394-397).
 *  - `stream` is a hipStream_t passed as void* (0 = default stream). All work is asynchronous on
 *    that stream. The per-token calls (woq_linear with int4 blobs, fp32 activations and M <= 8, the
 *    woq_engine step) neither synchronise nor allocate and can be captured into a hipGraph; the
 *    prefill GEMM (M > 8), int8 blobs and 16-bit activations at M <= 8 need scratch: it comes from the
 *    caller's workspace (woq_set_workspace, the reference's set_woq_workspace contract) when that has
 *    room — then these calls do not allocate either and are capturable — and otherwise from
 *    stream-ordered allocation (hipMallocAsync / hipFreeAsync on `stream`) per call, like the reference's
 *    per-call amalloc (bestla_weightonly_dispatcher.cpp:108-118,179); the engine's prompt pass owns its scratch.
 *  - return value: 0 on success, non-zero on error; woq_last_error() returns a thread-local
 *    message that starts with "QBits:" like the reference's TORCH_CHECK strings
 *    (bestla_weightonly_dispatcher.cpp:289,368; qbits.cpp:35,150). The Python shim raises
 *    RuntimeError with it, which is what c10::Error becomes in the reference.
 *  - dtype codes: enum woq_dtype in woq_blob.h (0 fp32, 1 bf16, 2 fp16).
 */
#ifndef WOQ_HIP_H_
#define WOQ_HIP_H_

#include <stddef.h>
#include <stdint.h>

#include "woq_blob.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WOQ_API __attribute__((visibility("default")))

WOQ_API const char* woq_last_error(void);
/* ABI revision of this header: 1 = rounds 1-3; 2 = round 4; 3 = round 5; 4 = round 6: FROZEN to what the boundary
 * needs (the qbits operator functions, the ops between the linears, the decode engine, the tensor-
 * parallel exchange). Every lab switch and measurement hook left it — the persistent launch and the token-long
 * prefetcher left the library altogether (tools/rejected/, both measured slower), the timing / probe entry points
 * live in woq_hip_experimental.h, which is NOT covered by this number. A client checks woq_abi_version() against
 * WOQ_ABI_VERSION at load time. */
#define WOQ_ABI_VERSION 4
WOQ_API int woq_abi_version(void);
/* number of visible HIP devices (0 when there is no GPU); never fails. */
WOQ_API int woq_device_count(void);

/* How the decode GEMVs read a 4-bit table weight type (nf4 / fp4_e2m1 / fp4_e2m1_bnb; no counterpart in the reference,
 * whose BesTLA kernels look the value up per weight): table[c] * S as `return value` balanced base-256 int8 digits —
 * planes[j][c >> 2] byte (c & 3) = digit j of code c — one v_mfma_i32_16x16x64_i8 per digit plane, and *wmul = 16 / S,
 * the factor that undoes S (and the 16 of the int4 kernels' 16 q operand). compute_type (enum woq_compute_type): nf4
 * takes three planes at fp32, two otherwise. Host-only (no device needed); 0 = not a table type. */
WOQ_API int woq_table_digit_planes(int weight_type, int compute_type, uint32_t planes[3][4], float* wmul);

/* ---- packed-weight management (load time) ---------------------------------------------------- */

/* replaces qbits.get_packed_weight_size (qbits.cpp:79-88). 0 = unsupported geometry. */
WOQ_API size_t woq_packed_weight_size(int K, int N, int blocksize, int weight_type, int scale_type, int asym,
                                      int act_shuffle);

/* replaces qbits.repack_quantized_weight (qbits.cpp:61-77 -> bestla_packq_impl.cpp:20-41).
 * weight_type (enum woq_weight_type): int4_clip — qweight int8 [K,N] holds int4 values in the signed domain
 * (modules.py:225-227); int3_clip / int2_clip — values in [-4, 3] / [-2, 1], kept in int4 storage with a header tag
 * (woq_blob.h narrow_bits: same bytes and kernels as int4; the name survives acquire_packed_weight_info);
 * int8 — full int8 values (stored as a composite of two int4 blobs, woq_blob.h); nf4 /
 * fp4_e2m1 / fp4_e2m1_bnb — table codes 0..15, no zero points; fp8_e4m3 / fp8_e5m2 — code bytes (as int8), no zero
 * points, scale_type may be WOQ_SCALE_FP8_E8M0 (power-of-two scales, stored as bf16). scale fp32 [G,N],
 * zp int8 [G,N] or NULL (sym), g_idx int32 [K] = GPTQ act-order group id of every K row (each group exactly
 * `blocksize` rows) or NULL; like BesTLA, repack converts it to activation shuffle indices
 * (qbits_ut/test_packq.py:22-28,59-64) and the blob keeps those. blob_dev: caller-allocated,
 * woq_packed_weight_size() bytes, 256-B aligned. Layout transform only; device-side. */
WOQ_API int woq_repack_quantized_weight(const int8_t* qweight_dev, const float* scale_dev, const int8_t* zp_dev,
                                        const int32_t* g_idx_dev, int K, int N, int blocksize, int weight_type,
                                        int scale_type, int compute_type, void* blob_dev, size_t blob_bytes,
                                        void* stream);

/* replaces qbits.quantize_to_packed_weight (qbits.cpp:90-100): RTN of an fp32 weight straight into a
 * blob. transpose != 0: weight is [N,K] (nn.Linear layout). Rounding rule: DESIGN.md (parity unpinned). */
WOQ_API int woq_quantize_to_packed_weight(const float* weight_dev, int transpose, int K, int N, int blocksize,
                                          int weight_type, int scale_type, int compute_type, int asym,
                                          void* blob_dev, size_t blob_bytes, void* stream);

/* the sequential sweep of GPTQ calibration over one block of B <= 128 consecutive input features, c0 <= j < c0 + B
 * (no reference counterpart: the reference hands GPTQ to neural_compressor; algorithm and layout: csrc/woq_gptq.hip,
 * DESIGN.md "GPTQ"). w fp32 [K,N] in working order (Linear.weight.T), modified in place; u fp32 [K,K] upper triangular
 * with H^-1 = U^T U. Per column, j ascending: at a group start the RTN parameters (woq_quantize_to_packed_weight's rule;
 * bits 2 | 3 | 4 | 8, sym or asym) of the current rows of the group go to scale fp32 [G,N] / zp int8 [G,N]; q int8 [K,N]
 * row j = the code (scale, zp and q in the domain woq_repack_quantized_weight takes); err fp32 [B,N] row j - c0 =
 * (w[j] - dequantised) / u[j][j]; the block's later rows take -err * u[j][k]; w[j] = the dequantised value. The rows
 * after the block are the caller's: w[c0+B:] -= u[c0:c0+B, c0+B:]^T err. group <= 0 or > K = one group per column.
 * params_given != 0 (static groups): scale / zp are read, not computed. col_group int32 [K] or NULL: the group of every
 * working row (after an act-order permutation), NULL = j / group. Computing parameters needs c0 and group to be
 * multiples of 32 (or one group per column). Asynchronous on `stream`; allocates nothing. */
WOQ_API int woq_gptq_sweep(float* w_dev, const float* u_dev, int K, int N, int c0, int B, int group, int bits, int asym,
                           int params_given, const int32_t* col_group_dev, int8_t* q_dev, float* scale_dev,
                           int8_t* zp_dev, float* err_dev, void* stream);

/* the two searches of AWQ calibration (no reference counterpart: the reference hands AWQ to neural_compressor; algorithm
 * and layout: csrc/woq_awq.hip, DESIGN.md "AWQ"). w fp32 [K,N] in working order (Linear.weight.T); Q = the RTN rule of
 * woq_quantize_to_packed_weight at bits 2 | 3 | 4 | 8, sym or asym, groups of `group` rows (the last may be short).
 * Both are asynchronous on `stream`, allocate nothing and modify no input.
 *
 * woq_awq_scale_delta: d_out fp32 [K,N] = diag(1/s) Q(diag(s) W) - W for one candidate s fp32 [K] (every s[k] nonzero)
 * of the scale search; each product, quotient and difference is rounded on its own. group <= 0 or > K = one group per
 * column. The loss tr(D^T H D) is the caller's GEMM. */
WOQ_API int woq_awq_scale_delta(const float* w_dev, const float* s_dev, int K, int N, int group, int bits, int asym,
                                float* d_out_dev, void* stream);

/* woq_awq_clip_search: per column n and group g, candidates c_j = 1 - j / n_grid, j < n_cand <= n_grid: the group is
 * clamped to +-c_j max|w| (sym) or [c_j min(min w, 0), c_j max(max w, 0)] (asym), d = Q(clamped) - w,
 * losses fp32 [n_cand,G,N][j][g][n] = d^T G d with G the group's diagonal block of h fp32 [K,K] (symmetric; row stride
 * ldh >= K, in elements); best int32 [G,N] = the first minimum; w_out fp32 [K,N] = w clamped by it. group: 32, 64 or 128. */
WOQ_API int woq_awq_clip_search(const float* w_dev, const float* h_dev, int ldh, int K, int N, int group, int bits,
                                int asym, int n_grid, int n_cand, int32_t* best_dev, float* losses_dev,
                                float* w_out_dev, void* stream);

/* the quantiser of AutoRound calibration (no reference counterpart: the reference hands AutoRound to neural_compressor /
 * auto-round; rule, gradients and layout: csrc/woq_autoround.hip, DESIGN.md "AutoRound"). w fp32 [K,N] in working order
 * (Linear.weight.T); v fp32 [K,N] the rounding offset in [-0.5, 0.5]; alpha, beta fp32 [G,N] the range factors in
 * [0, 1]; groups of `group` rows (the last may be short; group <= 0 or > K = one group per column); bits 2 | 3 | 4 | 8,
 * sym or asym. v = 0, alpha = beta = 1 is woq_quantize_to_packed_weight's RTN rule, bit for bit. Dtypes are
 * woq_dtype codes (fp32, bf16, fp16). All three are asynchronous on `stream` and allocate nothing.
 *
 * woq_autoround_forward: out [K,N] of out_dtype = the fake-quantised weight W~, the fp32 value rounded once. */
WOQ_API int woq_autoround_forward(const float* w_dev, const float* v_dev, const float* alpha_dev,
                                  const float* beta_dev, int K, int N, int group, int bits, int asym, void* out_dev,
                                  int out_dtype, void* stream);

/* woq_autoround_step: recomputes the forward, forms dL/dv, dL/dalpha, dL/dbeta from g = dL/dW~ [K,N] of g_dtype
 * (rounding straight-through, clips passing inside their range) and applies p <- clamp(p - lr sign(grad)) to v (lr_v)
 * and to alpha, beta (lr_minmax) in place; dL/dv is never stored. dalpha_out / dbeta_out: fp32 [G,N] or NULL, the raw
 * gradients. No floating-point atomics: the same inputs give the same bits. */
WOQ_API int woq_autoround_step(const float* w_dev, float* v_dev, float* alpha_dev, float* beta_dev, const void* g_dev,
                               int g_dtype, int K, int N, int group, int bits, int asym, float lr_v, float lr_minmax,
                               float* dalpha_out_dev, float* dbeta_out_dev, void* stream);

/* woq_autoround_codes: q int8 [K,N], scale fp32 [G,N], zp int8 [G,N] (NULL when sym) in the domain
 * woq_repack_quantized_weight takes. */
WOQ_API int woq_autoround_codes(const float* w_dev, const float* v_dev, const float* alpha_dev, const float* beta_dev,
                                int K, int N, int group, int bits, int asym, int8_t* q_dev, float* scale_dev,
                                int8_t* zp_dev, void* stream);

/* the quantiser of TEQ calibration (no reference counterpart: the reference hands TEQ to neural_compressor; rule,
 * gradient and layout: csrc/woq_teq.hip, DESIGN.md "TEQ"). w fp32 [K,N] in working order (Linear.weight.T); a fp32 [K]
 * the trainable per-input-channel scale, positive; groups of `group` rows (the last may be short; group <= 0 or > K =
 * one group per column); bits 2 | 3 | 4 | 8, sym or asym. u = w[k,n] a[k] goes through woq_quantize_to_packed_weight's
 * RTN rule and W~ = dequantised / a[k], each step rounded on its own: a = 1 is that rule bit for bit. Dtypes are
 * woq_dtype codes (fp32, bf16, fp16). Both are asynchronous on `stream` and modify no input.
 *
 * woq_teq_forward: out [K,N] of out_dtype = W~, the fp32 value rounded once. Allocates nothing. */
WOQ_API int woq_teq_forward(const float* w_dev, const float* a_dev, int K, int N, int group, int bits, int asym,
                            void* out_dev, int out_dtype, void* stream);

/* woq_teq_grad: da fp32 [K] (overwritten) = dL/da from g = dL/dW~ [K,N] of g_dtype: the forward is recomputed, rounding
 * is straight-through, clips pass inside their range, a group's max / min pass to the row that attains them. No
 * floating-point atomics and a summation order the layout fixes: the same inputs give the same bytes. Takes
 * K * ceil(N / 64) floats of scratch (woq_set_workspace, else a stream-ordered allocation). */
WOQ_API int woq_teq_grad(const float* w_dev, const float* a_dev, const void* g_dev, int g_dtype, int K, int N,
                         int group, int bits, int asym, float* da_dev, void* stream);

/* ---- backward of the linear with respect to its activations (reference: autograd/functions.py:163-179, which
 * dequantises the whole weight and calls a matmul; new entry points only, WOQ_ABI_VERSION stays 4) -------------------
 * dX[m][k] = sum_n dY[m][n] w[k][n], w as woq_dequantize_packed_weight defines it; for an act-order blob w is indexed
 * by blob row j and the result is written to column shuffle[j]. grad_out [M, ldg >= N] and grad_in [M, ldo >= K]
 * (overwritten; columns at or beyond K are not touched) are fp32 | bf16 | fp16. One fp16 product per operand pair on
 * the matrix cores (dY with an exact power-of-two scale per row, w relative to the blob's largest scale), fp32
 * accumulation over all of N in a fixed order, no floating-point atomics: the same inputs give the same bytes; a 16-bit
 * output is the fp32 result rounded once (csrc/woq_linear_bwd.hip, DESIGN.md "QLoRA backward"). Weight types: int4 /
 * int3 / int2 sym and asym, int8, nf4, fp4_e2m1, fp4_e2m1_bnb, every group size and both scale modes; fp8 weights fail
 * with a "QBits:" message. Stream-ordered, allocates nothing and synchronises nothing: its scratch is
 * woq_linear_backward_workspace(M, hdr) bytes of the workspace (woq_set_workspace), and a workspace without that much
 * room fails with a message that names the size, launching nothing.
 *
 * woq_linear_backward_workspace: 2 * Mpad * Npad64 (the fp16 image of dY) + 4 * Mpad rounded up to 256 (row scales)
 * + 256 (one word: the blob's largest scale), Mpad = M rounded up to 128, Npad64 = N rounded up to 64. It holds no
 * image of W and does not grow with K * N. 0 for a bad header or M <= 0. */
WOQ_API int woq_linear_backward(const void* grad_out_dev, int grad_dtype, int ldg, const void* blob_dev,
                                const woq_blob_header* hdr, void* grad_in_dev, int out_dtype, int ldo, int M,
                                void* stream);
WOQ_API size_t woq_linear_backward_workspace(int M, const woq_blob_header* hdr);

/* replaces qbits.dequantize_packed_weight (qbits.cpp:102-111): blob -> fp32 [K,N] or [N,K]. The
 * geometry is passed by value (hdr = host copy of the blob header) so the call never reads device
 * memory from the host. */
WOQ_API int woq_dequantize_packed_weight(const void* blob_dev, const woq_blob_header* hdr, float* out_dev,
                                         int transpose, void* stream);

/* copy the 256-B header of a device blob to host memory (synchronises `stream`). Load-time only;
 * the Python module caches the result so the hot path never re-parses it (the reference re-parses
 * per call, bestla_weightonly_dispatcher.cpp:335). */
WOQ_API int woq_read_header(const void* blob_dev, woq_blob_header* hdr_out, void* stream);

/* replaces qbits.acquire_packed_weight_info for the tensor-valued selectors
 * (bestla_packq_impl.cpp:152-204): SCALE_TENSOR -> fp32 [G,N], ZP_TENSOR -> int8 [G,N] (signed
 * domain), G_IDX -> int32 [K]. Scalar / string selectors are answered from the cached header in
 * the Python shim. out_dev is caller-allocated. */
WOQ_API int woq_blob_extract(const void* blob_dev, const woq_blob_header* hdr, int what, void* out_dev,
                             void* stream);

/* replaces qbits.set_woq_workspace (qbits.cpp:142-144 -> bestla_weightonly_dispatcher.cpp:394-397): a raw pointer
 * into caller-owned device memory that must outlive every later call; woq_linear carves its scratch from it (int8
 * composite: M * N * 4 bytes; M > 8: the packed activation planes, about 2 * Mpad * Kpad * (1 or 2 planes) +
 * 8 * Mpad + 4 * Npad bytes; fp16 / bf16 activation rows at M <= 8 are read natively and need none). Process-wide like the reference's (calls from
 * several host threads are not safe with it). NULL / 0 removes it. */
WOQ_API int woq_set_workspace(void* workspace_dev, size_t bytes);

/* ---- the hot call ------------------------------------------------------------------------------ */

/* replaces qbits.woq_linear (qbits.cpp:113-140): out[M,N] = act[M,K] . W_deq[K,N] (+ bias).
 *   act: act_dtype [M, lda]; out: out_dtype [M, ldo], written in place; bias fp32 [N] or NULL
 *   (alpha = 1, beta = bias ? 1 : 0, bestla_customop.hpp:22-40). Activation shuffle (g_idx) is
 *   applied when the blob carries indices (autograd/functions.py:52-57).
 * Kernel selection by M: M <= 8 decode GEMV (int8-MFMA inner product over exact fixed-point activation limbs,
 * csrc/woq_gemv_i8.hip; the generic fp32-VALU kernel for shuffled / table / fp8 blobs), M > 8 MFMA GEMM
 * (csrc/woq_gemm_f16.hip; its K loop for the one-product form is scheduled by hand, csrc/woq_gemm_f16p.h). */
WOQ_API int woq_linear(const void* act_dev, int act_dtype, int lda, const void* blob_dev,
                       const woq_blob_header* hdr, const float* bias_dev, void* out_dev, int out_dtype, int ldo,
                       int M, void* stream);

/* ---- ops between the linears (replace stock-HF module forwards) -------------- */

/* The four calls below refuse, before any launch, a dtype code other than WOQ_F32, WOQ_F16 or WOQ_BF16, a null pointer
 * with a non-zero size and a negative size; rows / tokens / heads / n == 0 is a no-op. Results are computed in fp32 and
 * rounded once on store (nearest even; fp16 overflow goes to +-inf, nothing saturates). */

/* HF LlamaRMSNorm: out = x * rsqrt(mean(x^2) + eps) * weight ; x/out dtype [rows, d], weight fp32 [d].
 * dtype, out_dtype: WOQ_F32, WOQ_F16 or WOQ_BF16, each on its own; rows >= 0, d > 0; x, out contiguous [rows, d]. */
WOQ_API int woq_rmsnorm(const void* x_dev, int dtype, const float* weight_dev, float eps, int rows, int d,
                        void* out_dev, int out_dtype, void* stream);
/* HF apply_rotary_pos_emb (rotate_half) in place on x [tokens, heads, D]; cos/sin fp32 tables
 * [max_pos, D/2]; pos int32 [tokens] (device).
 * dtype: WOQ_F32, WOQ_F16 or WOQ_BF16; tokens, heads >= 0, D even; every pos[t] in [0, max_pos) (not checked). */
WOQ_API int woq_rope(void* x_dev, int dtype, const int32_t* pos_dev, const float* cos_dev, const float* sin_dev,
                     int tokens, int heads, int D, void* stream);
/* HF LlamaMLP elementwise part: out = silu(gate) * up, n elements.
 * dtype: WOQ_F32, WOQ_F16 or WOQ_BF16, shared by gate, up and out [n]; out may be gate or up. */
WOQ_API int woq_silu_mul(const void* gate_dev, const void* up_dev, int dtype, size_t n, void* out_dev, void* stream);
/* GeLU: approximate != 0 -> tanh form ("gelu_new", GPT-2), else erf form.
 * dtype: WOQ_F32, WOQ_F16 or WOQ_BF16, shared by x and out [n]; out may be x. */
WOQ_API int woq_gelu(const void* x_dev, int dtype, size_t n, int approximate, void* out_dev, void* stream);

/* ---- fused batch-1 decode engine (Llama-class decoder; the measured path of bench.py) ----------
 * A woq_engine owns no weights: it holds device pointers to the per-layer WQH1 blobs and norm
 * vectors plus its own activation scratch and KV cache, and launches the whole token step
 * (5 kernels per layer) from C++, optionally replayed as one hipGraph. */
typedef struct woq_engine woq_engine;

typedef struct woq_engine_config {
  int32_t hidden, inter, heads, kv_heads, head_dim, layers, vocab, max_ctx;
  float rms_eps, rope_theta;
  int32_t tp_rank, tp_size; /* tensor parallel: heads/inter are PER-RANK sizes when tp_size > 1 */
  int32_t kv_dtype;         /* WOQ_F16 | WOQ_BF16 | WOQ_FP8_E4M3 (unscaled e4m3fn, saturating at +-448) */
  int32_t reserved[3];      /* [0] = max_batch: sequences the KV cache holds for woq_engine_prefill (0 / 1 = one);
                             * [1] = attn_splits: context slices per head in the decode attention (0 = automatic:
                             *       1 up to max_ctx 4096, else 1024 / heads clamped to [2, 32]);
                             * [2] = sliding window (HF Mistral `sliding_window`): a query sees the last `window`
                             *       positions, itself included; 0 = full causal attention */
} woq_engine_config;

typedef struct woq_layer_weights {
  const void* qkv_blob;     /* [hidden -> (heads + 2 kv_heads) * head_dim] */
  const void* o_blob;       /* [heads*head_dim -> hidden] */
  const void* gate_up_blob; /* [hidden -> 2*inter], 16-column tiles interleaved gate/up */
  const void* down_blob;    /* [inter -> hidden] */
  const float* ln1;         /* input_layernorm weight fp32 [hidden] */
  const float* ln2;         /* post_attention_layernorm weight fp32 [hidden] */
  woq_blob_header qkv_hdr, o_hdr, gate_up_hdr, down_hdr;
} woq_layer_weights;

WOQ_API int woq_engine_create(const woq_engine_config* cfg, woq_engine** out);
WOQ_API void woq_engine_destroy(woq_engine* e);
/* Every check runs before the layer is stored: a refused call leaves the engine as it was. All layers of an engine are
 * of one kind (integer / 4-bit table blobs, or fp8 blobs of one type), in whichever order they are set; a step, capture,
 * phase or prompt pass is refused until every layer has been set. */
WOQ_API int woq_engine_set_layer(woq_engine* e, int layer, const woq_layer_weights* w);
/* embed: fp16/bf16 [vocab, hidden]; final norm fp32 [hidden]; lm_head fp16/bf16 [vocab_shard, hidden]
 * (NOT quantised, like the reference: utils/config.py:836-837 llm_int8_skip_modules). */
WOQ_API int woq_engine_set_head(woq_engine* e, const void* embed_dev, int embed_dtype, const float* final_norm_dev,
                                const void* lm_head_dev, int lm_head_dtype, const float* cos_dev,
                                const float* sin_dev);
/* optional: make the engine use caller-owned device buffers (e.g. torch tensors) for its I/O instead of
 * its own: token int32[1], pos int32[1], logits fp32[vocab], hidden fp32[hidden]. NULL keeps the internal one. */
WOQ_API int woq_engine_bind_io(woq_engine* e, void* token_dev, void* pos_dev, void* logits_dev, void* hidden_dev);
/* device buffers the caller reads/writes between steps */
WOQ_API void* woq_engine_token_ptr(woq_engine* e);  /* int32[1]: token fed to the next step */
/* int32[max_ctx + 1]: a greedy step that fed position p leaves its new token in slot p, so a host that replays k
 * steps back to back reads k tokens with ONE synchronisation (the reference's loop pays a host round trip per token,
 * transformers/generation: greedy_search.py:148-150,374-377) */
WOQ_API void* woq_engine_token_log_ptr(woq_engine* e);
WOQ_API void* woq_engine_pos_ptr(woq_engine* e);    /* int32[1]: its position */
WOQ_API void* woq_engine_logits_ptr(woq_engine* e); /* fp32[vocab] of the last step */
WOQ_API void* woq_engine_hidden_ptr(woq_engine* e); /* fp32[hidden] residual stream (TP all-reduce target) */
/* one decode step: embed(token) -> layers -> final norm -> lm_head -> logits; if greedy != 0 also
 * argmax -> token_ptr and pos_ptr += 1, so steps can be chained with no host round trip. */
WOQ_API int woq_engine_step(woq_engine* e, int greedy, void* stream);
/* prompt pass (what HF's first generate() forward does with the reference's linears at M = batch * T rows,
 * nn/modules.py:140-169): n_seq sequences x T new tokens each, tokens int32 [n_seq][T] on the device, at positions
 * start_pos .. start_pos + T - 1 (each sequence's cache must already hold [0, start_pos): chunked prefill = calls
 * with growing start_pos). Fills the KV caches; the last position's logits of every sequence go to
 * woq_engine_prefill_logits_ptr() (fp32 [n_seq][vocab]); sequence 0's also to logits_ptr / hidden_ptr, with
 * pos_ptr = start_pos + T - 1, and if greedy != 0 token_ptr = argmax and pos_ptr = start_pos + T so that
 * woq_engine_step continues sequence 0. Linears run on the fp16-operand MFMA GEMM whatever the blobs' compute_type;
 * q/k/v, attention output and MLP activations are fp16 between kernels, the residual stream fp32. */
WOQ_API int woq_engine_prefill(woq_engine* e, const int32_t* tokens_dev, int n_seq, int T, int start_pos, int greedy,
                               void* stream);
WOQ_API void* woq_engine_prefill_logits_ptr(woq_engine* e);
/* like woq_engine_prefill with n_seq == 1, and it also writes rows of the three logs of
 * woq_engine_logprob_ptr: row start_pos + t describes the raw distribution after position start_pos + t,
 * chosen = log-probability of targets_dev[t] (device int32 [T]: the id at position start_pos + t + 1).
 * greedy == 0: rows t = 0 .. T-1. greedy != 0: rows t = 0 .. T-2; row T-1 belongs to the chaining tail
 * exactly as today (its target is the token the tail picks; targets_dev[T-1] is not read).
 * Chunked scoring = calls with growing start_pos, a non-final chunk with greedy == 0 and the next chunk's first id as
 * its last target. A row is the record documented at woq_engine_set_logprobs (20 ids, NaN logits weigh 0, -1 / -inf
 * padding); a target outside [0, vocab) gives chosen = NaN, the row's 20 ids are written all the same. lm_head runs
 * over all rows on the matrix cores, the final-norm row as a hi + lo pair in lm_head's type, fp32 accumulation
 * (csrc/woq_score.hip), in blocks of 256 rows: the scratch (256 x vocab x 4 bytes of logits) is allocated on first use.
 * KV cache, token_ptr, pos_ptr, logits_ptr and prefill_logits_ptr end as after woq_engine_prefill(e, tokens, 1, T,
 * start_pos, greedy, stream). Fails with a "QBits:" message before the first woq_engine_set_logprobs(e, 1) (the logs
 * do not exist; recording need not be on), on a tensor-parallel engine, for a vocabulary the record does not cover and
 * for a hidden size that is no multiple of 8. */
WOQ_API int woq_engine_prefill_scored(woq_engine* e, const int32_t* tokens_dev, int T, int start_pos,
                                      const int32_t* targets_dev, int greedy, void* stream);
/* decode attention regime: 1 = one workgroup per head (fastest up to a few hundred cached positions), n > 1 = n
 * context slices per head + a combine launch (long contexts). Takes effect at the next step / capture; a graph
 * captured earlier keeps the regime it was captured with. */
WOQ_API int woq_engine_set_attn_splits(woq_engine* e, int splits);
WOQ_API int woq_engine_attn_splits(woq_engine* e);
/* sliced regime only: on = one workgroup per (kv head, slice) computing all the query heads of the group on the
 * matrix cores, so each K / V row is fetched once per group instead of once per query head (measured faster at
 * 8k cached positions, Mistral-7B shape; applies to head_dim 128 with 2 / 4 / 8 query heads per kv head and an fp16 or
 * fp8 cache — silently the per-query-head slices otherwise). Default off. Same capture rule as attn_splits. */
WOQ_API int woq_engine_set_attn_grouped(woq_engine* e, int on);
WOQ_API int woq_engine_attn_grouped(woq_engine* e);
/* decode step, XQ path: [RMSNorm + qkv GEMV] and [RoPE + KV append + attention] as ONE launch — the workgroup whose
 * column strip completes a head's q / k / v runs that head's attention (csrc/woq_gemv_attn.hip). Applies to multi-head
 * shapes (heads == kv_heads), head_dim 128, hidden 4096, one context slice, no sliding window; the two launches
 * otherwise. Default on (WOQ_ENGINE_FUSE_ATTN=0 turns it off). Same capture rule as attn_splits.
 * woq_engine_fuse_attn: 1 when the next step / capture will use it. */
WOQ_API int woq_engine_set_fuse_attn(woq_engine* e, int on);
WOQ_API int woq_engine_fuse_attn(woq_engine* e);
/* sticky device-side status of the decode step, 0 = fine; bit 0: an attention workgroup of the fused launch gave up
 * waiting for its head's q / k / v after its bound (its outputs are then wrong); bit 1: a step started with its
 * position at or beyond max_ctx — it ran at max_ctx - 1 instead (outputs meaningless, nothing written out of bounds;
 * woq_engine_step / _replay cannot check a position that lives on the device); bit 2: a greedy step found no
 * winning logit (all NaN) and fed token 0; bit 3: a sampled step found more than 1024 scores at or above the k-th
 * largest (ties) and kept the 1024 with the lowest ids among the tied — informational, the token stands; not set
 * when the tie is at -inf below a finite best score (fewer than k finite scores: those candidates weigh 0);
 * bit 4: a step with a token guide picked an id that the guide's state bans (a state with every id banned, which a
 * well-formed guide does not have) or whose entry names no state of the table — the state stayed where it was;
 * -1 = the read itself failed.
 * Synchronises `stream`. */
WOQ_API int woq_engine_status(woq_engine* e, void* stream);
/* resets the sticky status to 0 (stream-ordered): a caller that read a non-zero status, changed what caused it
 * (e.g. woq_engine_set_fuse_attn(e, 0)) and re-runs the request starts from a clean word. */
WOQ_API int woq_engine_clear_status(woq_engine* e, void* stream);
/* KV cache base pointers (which: 0 = K, 1 = V), layout [sequence][layer][position][kv_head][head_dim] in kv_dtype:
 * inspection / tests, and the seam for an external cache manager. */
WOQ_API void* woq_engine_kv_cache_ptr(woq_engine* e, int which);
/* 1 when the decode step hands activations between its kernels as XQ limb blocks (csrc/woq_xq.h; every layer's blobs
 * qualify, one GPU, WOQ_ENGINE_XQ != 0), 0 when it runs the fp32-activation kernels. */
WOQ_API int woq_engine_uses_xq(woq_engine* e);
/* capture one step into a hipGraph and replay it `n` times (greedy chaining). Round 5: a greedy capture also holds the
 * step chained 8 times as ONE graph (interior token boundaries: argmax + next embedding as one launch); replay(n) then issues n / 8 launches of it and n % 8 single steps — same kernels, same
 * tokens, +0.6 % tokens/s (each hipGraphLaunch costs the device a few us between tokens). */
WOQ_API int woq_engine_capture(woq_engine* e, int greedy, void* stream);
WOQ_API int woq_engine_replay(woq_engine* e, int n, void* stream);
/* `n` decode steps issued eagerly back to back (no graph, no host synchronisation; with greedy != 0 the token /
 * position chain on the device like a replayed graph). Same device time as woq_engine_replay on the same stream; costs
 * the host ~2.6 us per launch. (Round 4 note: graph replays looked ~1 us per kernel boundary slower until their launch
 * was moved off a stream that sat behind cross-stream event waits — profiles/r04ab_stream_mode_probe.txt.) */
WOQ_API int woq_engine_steps(woq_engine* e, int n, int greedy, void* stream);
/* ---- sampled token tail (added after the freeze of revision 4: new entry points only, nothing existing changed, so
 * WOQ_ABI_VERSION stays 4 — a client that needs them looks the symbols up) -----------------------------------------
 * With a sampler installed, every step that chains on the device (greedy != 0: woq_engine_step / _steps / _capture /
 * _replay and the prompt pass's tail) picks its next token with Hugging Face's logits processing instead of the plain
 * argmax, in one launch after the lm_head (csrc/woq_sample.hip), HF's order: RepetitionPenaltyLogitsProcessor over the
 * ids of the `seen` bit set (fp32, `s < 0 ? s * penalty : s / penalty`), then argmax (do_sample == 0, lowest id on
 * ties) or TemperatureLogitsWarper, TopKLogitsWarper (ties at the k-th value survive), TopPLogitsWarper
 * (min_tokens_to_keep 1) and an inverse-CDF draw with u = (x0 >> 8) * 2^-24, x0 = word 0 of Philox4x32-10 under counter
 * (position fed + discarded, 0, 0, 0) and key (seed_lo, seed_hi), `discarded` = the positions a rolling KV cache has
 * dropped (woq_engine_kv_shift; 0 for a request that never shifts, uint32 wrap): a token depends on (seed, absolute
 * position in the stream, logits) only, whatever the burst size or launch mode, and no draw repeats after a shift.
 * Covered: do_sample == 0; 1 <= top_k <= 1024 with any top_p; top_k == 0 with top_p == 1. */
typedef struct woq_sampler_config {
  int32_t do_sample;        /* 0 = argmax of the penalised scores */
  int32_t top_k;            /* 0 = whole vocabulary */
  float temperature, top_p, repetition_penalty;
  uint32_t seed_lo, seed_hi;
  uint32_t reserved;        /* 0 */
} woq_sampler_config;
/* cfg (host memory) is copied into a device struct the kernel reads: changing parameters needs no new capture, only
 * installing or removing (cfg == NULL) the sampler drops a captured graph. Synchronises the device. Fails with a
 * "QBits:" message on a tensor-parallel engine (vocab-sharded head) or for a combination that is not covered. */
WOQ_API int woq_engine_set_sampler(woq_engine* e, const woq_sampler_config* cfg);
/* history of the repetition penalty: uint32 [(vocab + 31) / 32] bit set owned by the engine. Marks tokens_dev[0..n)
 * (device int32; may be NULL with n == 0), after zeroing the set when clear != 0; stream-ordered. The sampled tail
 * marks every token it picks itself. */
WOQ_API int woq_engine_sampler_seen(woq_engine* e, const int32_t* tokens_dev, int n, int clear, void* stream);
WOQ_API void* woq_engine_sampler_seen_ptr(woq_engine* e);
/* ---- sampler controls: logit bias, presence / frequency penalty, min_p (new entry points only; WOQ_ABI_VERSION stays
 * 4 and woq_sampler_config stays 32 bytes) -----------------------------------------------------------------------------
 * With controls installed beside a sampler, the score of id i is built from the fp32 logit l by these fp32 operations,
 * each rounded on its own, in this order: s = l + bias[i] for ids with a bias entry (finite, or -inf = a ban; ahead of
 * the penalties like HF's SequenceBiasLogitsProcessor and vLLM's logit_bias); the repetition penalty over `seen` as
 * above; for ids GENERATED c[i] > 0 times in this request s = s - (frequency_penalty * (float)c[i]), then
 * s = s - presence_penalty (prompt tokens do not count — the vLLM convention; a host that wants otherwise preloads the
 * counts); then / temperature, top-k and top-p as above, and min_p (HF's MinPLogitsWarper, min_tokens_to_keep 1, after
 * top-p): a candidate stays iff expf(s_i - s_max) >= min_p. With do_sample == 0 the pick is the argmax of the
 * penalised scores. top_k == 0 with top_p == 1 and 0 < min_p <= 1 is covered. A pre-pass over the whole chip writes the
 * scores into an engine-owned scratch and the sampling launch reads that (csrc/woq_sample.hip): one more launch per
 * step, shapes by the vocabulary alone; the log-probability record keeps describing the raw logits. The tail also
 * counts every token it picks. */
typedef struct woq_sampler_controls {
  float presence_penalty, frequency_penalty; /* finite; 0 = off */
  float min_p;                               /* [0, 1]; 0 = off; > 0 needs do_sample */
  int32_t n_bias;                            /* entries of the two host arrays, 0..1024 */
  uint32_t reserved[4];                      /* 0 */
} woq_sampler_controls;
/* ctl (host memory) and the n_bias (token id, value) pairs are copied into device memory the kernels read: changing them
 * needs no new capture, installing or removing (ctl == NULL; also woq_engine_set_sampler(e, NULL)) the controls drops a
 * captured graph. Needs a sampler installed. Synchronises the device. Fails with a "QBits:" message for ids outside
 * [0, vocab), duplicate ids, n_bias > 1024, min_p outside [0, 1] or > 0 without do_sample, non-finite penalties and a
 * bias of +inf or NaN. */
WOQ_API int woq_engine_set_sampler_controls(woq_engine* e, const woq_sampler_controls* ctl, const int32_t* bias_ids_host,
                                            const float* bias_vals_host);
/* the generated-token counts: uint32 [vocab] owned by the engine. counts[tokens_dev[j]] += 1 for j in [0, n) (device
 * int32; may be NULL with n == 0) after zeroing the table when clear != 0; stream-ordered. */
WOQ_API int woq_engine_sampler_counts(woq_engine* e, const int32_t* tokens_dev, int n, int clear, void* stream);
WOQ_API void* woq_engine_sampler_count_ptr(woq_engine* e);
/* ---- token guide: constrained decoding (new entry points only; WOQ_ABI_VERSION stays 4, no struct changes) -----------
 * A guide is a deterministic automaton over token ids as a dense table next[n_states][vocab] of uint16_t: 0xFFFF = the
 * id is banned in that state, any other value = the state after that id; 1 <= n_states <= 65535. With one installed
 * beside a sampler, every chaining step builds its scores by the four steps of the sampler controls above (neutral
 * controls when none are installed) and then, as step 5, s = -inf where next[state][i] == 0xFFFF; the pick follows as
 * above, and a one-thread launch after it sets state = next[state][token]. Two more launches per step than the plain
 * sampled tail (the pre-pass and the advance), shapes by the vocabulary alone. The state lives on the device, so bursts
 * of steps and replayed graphs follow the guide with no host round trip. A well-formed guide has no state with every
 * id banned; the device does not check: such a state picks what the sampler picks among all -inf scores, stays, and
 * raises status bit 4. The log-probability record keeps describing the raw logits.
 * set_guide copies the table (DEVICE memory, n_states * vocab uint16_t) into memory the engine owns, grown when needed
 * and kept; the kernels read the table pointer and the state from a device struct, so installing another guide over
 * an installed one, or resetting the state, keeps a captured graph valid. Installing the first guide or removing it
 * (table_dev == NULL; also woq_engine_set_sampler(e, NULL)) drops a captured graph. Needs a sampler installed.
 * Synchronises the device. Fails with a "QBits:" message on a tensor-parallel engine, for n_states outside 1..65535
 * and for start_state outside [0, n_states). */
WOQ_API int woq_engine_set_guide(woq_engine* e, const void* table_dev, int n_states, int start_state);
/* state = `state`, stream-ordered (a request starts from its guide's start state, or from the state after its prompt) */
WOQ_API int woq_engine_guide_reset(woq_engine* e, int state, void* stream);
/* int32[1] on the device: the guide's current state; NULL before the first woq_engine_set_guide */
WOQ_API void* woq_engine_guide_state_ptr(woq_engine* e);
/* ---- per-token log-probabilities (new entry points only; WOQ_ABI_VERSION stays 4) ----------------------------------
 * With recording on, every step that chains on the device (greedy != 0: the prompt pass's tail, woq_engine_step /
 * _steps / _capture / _replay) writes, after its pick, one row of three device logs indexed like the token log (row p
 * = the step that fed position p), csrc/woq_logprob.hip. A row describes the RAW model distribution, log_softmax over
 * the fp32 lm_head logits of that step, before repetition penalty, temperature, top-k and top-p, whether the token came
 * from the argmax or from the sampler:
 *   chosen[p]          fp32   log-probability of the token the step picked
 *   top_id[p][0..20)   int32  the 20 ids with the largest logits, ordered by (logit descending, id ascending)
 *   top_lp[p][0..20)   fp32   their log-probabilities
 * Always 20 (fewer alternatives are a host-side slice). NaN logits weigh 0 and are never listed; fewer than 20 other
 * logits pad with id -1 / -inf; -inf logits are legal (log-probability -inf, listed last, ties by id); an all-NaN row
 * gives chosen = NaN and every id -1 (status bit 2 comes from the pick). A logits-only step (greedy == 0) writes
 * nothing. Two launches per step whose shape depends on the vocabulary alone; with recording off the step is unchanged.
 * set_logprobs allocates the logs, max_ctx + 1 rows each, on first use; switching on or off drops a captured graph.
 * Fails with a "QBits:" message on a tensor-parallel engine (vocab-sharded head). */
WOQ_API int woq_engine_set_logprobs(woq_engine* e, int on);
WOQ_API int woq_engine_logprobs(woq_engine* e); /* 1 when recording */
/* which: 0 chosen, 1 top_id, 2 top_lp; NULL before the first woq_engine_set_logprobs(e, 1) */
WOQ_API void* woq_engine_logprob_ptr(woq_engine* e, int which);
/* ---- rolling KV cache (StreamingLLM, reference docs/streamingllm.md: n_keep sinks, n_discard dropped after them; new
 * entry points only, WOQ_ABI_VERSION stays 4, no struct changes) -------------------------------------------------------
 * Sequence `seq`'s cache holds positions [0, n_cached). The call drops positions [n_keep, n_keep + n_discard) and moves
 * every later row n_discard positions down, in place, in every layer (csrc/woq_kv_shift.hip): V rows are copied bit for
 * bit; K rows, which are stored rotated, are rotated back by the angle of n_discard with row n_discard of the tables
 * given to woq_engine_set_head (pairing d, d + D/2: a = K[p][d], b = K[p][d + D/2] -> a * cos + b * sin, b * cos -
 * a * sin, products and sum in fp64, the sum rounded to fp32) and stored with the cache type's rounding and saturation —
 * what the append kernels would have written at position p - n_discard, up to that rounding. Afterwards rows [0, n_keep) are bit-unchanged, rows
 * [n_keep, n_cached - n_discard) hold the shifted rows, rows [n_cached - n_discard, n_cached) are unspecified, rows at
 * or beyond n_cached and every other sequence are untouched. Every shift re-rounds the moved K rows to the cache type:
 * for fp16 / bf16 one more rounding of the size the row already carries, for e4m3 a 3-bit mantissa each time.
 * All geometry comes from the host, which counts its tokens: nothing is read back, nothing synchronises, nothing
 * allocates; the work is stream-ordered and capturable. move_pos != 0 (seq == 0 only) also does pos -= n_discard and
 * discarded += n_discard on the device in the same stream order, so a replayed graph or an eager burst issued next
 * feeds position n_cached - n_discard. n_keep + n_discard == n_cached is legal: no row moves, only the two words change.
 * Fails with a "QBits:" message, launching nothing: on a tensor-parallel engine, with a sliding window (reserved[2]),
 * for seq outside [0, max_batch), n_keep < 0, n_discard < 1, n_keep + n_discard > n_cached, n_cached > max_ctx, and
 * move_pos with seq != 0. */
WOQ_API int   woq_engine_kv_shift(woq_engine* e, int seq, int n_keep, int n_discard, int n_cached, int move_pos, void* stream);
WOQ_API void* woq_engine_discarded_ptr(woq_engine* e);                    /* int32[1] on the device */
WOQ_API int   woq_engine_discarded_set(woq_engine* e, int value, void* stream);
/* ---- per-layer extras of Llama-class variants: Qwen2's q / k / v biases, Qwen3's q / k norm (new entry point only,
 * WOQ_ABI_VERSION stays 4, no struct changes) ----------------------------------------------------------------------------
 * optional per-layer extras of Llama-class variants; every pointer may be NULL (= absent); fp32 on the device;
 * the engine keeps the pointers (the caller owns the memory), like woq_engine_set_layer:
 *   qkv_bias [(heads + 2 kv_heads) * head_dim]  added to the fused q|k|v projection (Qwen2)
 *   q_norm, k_norm [head_dim]                   RMSNorm over head_dim of every q / k head BEFORE RoPE,
 *                                               eps = cfg.rms_eps (Qwen3); both or neither
 * The bias is added in the projection's epilogue, after the input RMSNorm's factor, in the decode step (all three
 * forms: fused qkv + attention launch, XQ GEMV, fp32-activation GEMV) and in the prompt pass's GEMM. The norm is
 * x * rsqrt(mean(x^2) + eps) * w in fp32 (HF Qwen3RMSNorm), inside the decode attention (per-query-head and fused forms;
 * a layer with a norm never takes the grouped form) and the prompt pass's RoPE / append kernel, where q and k are
 * rounded once, after norm and rotation. The call comes after woq_engine_set_layer for that layer (which clears the
 * layer's extras); a call that changes which extras are present, or their pointers, drops captured graphs. Fails with a
 * "QBits:" message on a tensor-parallel engine (tp_size > 1, a communicator or an all-reduce callback), for a bias on
 * fp8-weight layers, for only one of q_norm / k_norm, and for a norm with head_dim not a multiple of 16. */
WOQ_API int woq_engine_set_layer_extras(woq_engine* e, int layer, const float* qkv_bias_dev,
                                        const float* q_norm_dev, const float* k_norm_dev);
/* ---- unmerged LoRA adapters on the engine (new entry points only, WOQ_ABI_VERSION stays 4, no struct changes) ---------
 * A targeted projection computes y = x . W_deq (+ bias) + scaling * (x . A^T) . B^T with A [r][K], B [N][r] in fp32 and
 * fp32 accumulation (the reference's QuantizedLoraLinearQBits.forward at inference: dropout is the identity); x is the
 * projection's own input (the RMSNorm output for q / k / v and gate / up, the attention output for o_proj,
 * SiLU(gate) * up for down_proj). Targets: 0 q_proj, 1 k_proj, 2 v_proj, 3 o_proj, 4 gate_proj, 5 up_proj, 6 down_proj;
 * any subset, ranks may differ per target, 1 <= r <= 64. One adapter per target at a time.
 *   lora_reserve  once per engine: the per-layer A / B tables of all seven targets at rank r_max, the device descriptors
 *                 the kernels read ranks and scalings from, and the decode step's four delta buffers. Changes no step.
 *   set_lora      copies one target's tables in (a_dev: fp32 [r][K], b_dev: fp32 [N][r], dense, device memory; the
 *                 caller's tensors are free afterwards); r == 0 removes the target. Synchronises the device.
 *   clear_lora    removes every target.   lora_on: the number of (layer, fused projection) pairs that carry an adapter.
 * Decode step: in front of every fused projection (q|k|v, o, gate/up, down) with at least one installed part ONE launch
 * (csrc/woq_lora.hip) writes static bias + scaling * B . (A . x) per output column, which the projection's GEMV takes
 * through its bias slot: after the RMSNorm factor, before SiLU * mul, the residual add and the XQ output; all forms
 * (XQ GEMV, fused qkv + attention, fp32-activation GEMV). Prompt pass: two launches per such projection on the f32-input
 * matrix cores; q / k / v and gate / up are rounded to fp16 once more than without an adapter. A projection
 * without an installed part keeps exactly the calls it has without adapters, and an engine without adapters issues no
 * new launch. Captured graphs: a call that changes WHICH (layer, fused projection) pairs carry an adapter drops them;
 * other values, or another adapter of the same targets and ranks up to r_max, keep them (tables, descriptors and launch
 * geometry do not move; ranks are device data). Every refusal is checked before any state changes: a tensor-parallel
 * engine (tp_size > 1, a communicator or an all-reduce callback), fp8-weight layers, r > r_max, set before reserve, a
 * layer that is not set, a second reserve, shapes whose rows / columns are no multiples of 16. */
WOQ_API int woq_engine_lora_reserve(woq_engine* e, int r_max);
WOQ_API int woq_engine_set_lora(woq_engine* e, int layer, int target, const float* a_dev, const float* b_dev, int r,
                                float scaling);
WOQ_API int woq_engine_clear_lora(woq_engine* e);
WOQ_API int woq_engine_lora_on(woq_engine* e);
/* tensor-parallel seam: when set, the engine calls `fn(user, buf_dev, count_f32, stream)` after
 * o_proj and after down_proj (row-parallel partial sums -> sum over ranks). The Python host binds it
 * to RCCL via torch.distributed. NULL = single GPU. */
typedef int (*woq_allreduce_fn)(void* user, void* buf_dev, size_t count, void* stream);
WOQ_API int woq_engine_set_allreduce(woq_engine* e, woq_allreduce_fn fn, void* user);
/* ---- device-side tensor-parallel exchange (one process per GPU) ----------------------------------
 * The reference has no counterpart (its multi-device inference is DeepSpeed AutoTP on fp models,
 * neural_chat/models/model_utils.py:238-311); this is the exchange step the sharded int4 path needs: the sum over ranks
 * of the row-parallel [hidden] partials after o_proj and down_proj, and the greedy-token pick over a vocab-sharded
 * lm_head. Both are kernels on the caller's stream (capturable): every rank stores 8-byte {fp32, tag} granules straight
 * into every peer's inbox over xGMI (hipIpc-mapped) and sums what arrives in its own, rank order 0..W-1 (bit-identical
 * results on all ranks). Set-up, per rank: create -> handle (64 bytes, exchanged by the host, e.g. torch.distributed
 * all_gather) -> connect(all handles, device ordinal of every rank). All ranks must issue the same sequence of
 * collectives. A peer that does not show up within the timeout (default 2 s) sets a sticky status instead of hanging. */
typedef struct woq_comm woq_comm;
WOQ_API int woq_comm_create(int rank, int world, size_t max_elems, woq_comm** out);
WOQ_API int woq_comm_handle(woq_comm* c, void* handle_out, size_t bytes);
WOQ_API int woq_comm_connect(woq_comm* c, const void* handles, const int* peer_devices);
/* in-place sum over ranks of buf[0..n) fp32, n <= max_elems */
WOQ_API int woq_comm_allreduce_f32(woq_comm* c, float* buf_dev, size_t n, void* stream);
/* synchronises `stream`; *status_out: 0 = every collective so far completed, bit 0 / 1 = an all-reduce / a token
 * exchange timed out (results after that are undefined) */
WOQ_API int woq_comm_status(woq_comm* c, void* stream, int* status_out);
WOQ_API int woq_comm_set_timeout_ms(woq_comm* c, int ms);
WOQ_API void woq_comm_destroy(woq_comm* c);
/* make the engine's decode step issue the exchange itself (after o_proj and down_proj, and for the greedy token:
 * token id = vocab_offset + local argmax of this rank's lm_head rows), so woq_engine_capture / replay cover a whole
 * tensor-parallel token. The comm must outlive the engine's use of it. NULL = back to the callback / single GPU. */
WOQ_API int woq_engine_set_comm(woq_engine* e, woq_comm* comm, int vocab_offset);
/* tensor-parallel decode step with a bound device communicator. xq (default on, WOQ_TP_XQ=0 off): the ranks run the
 * XQ decode kernels (csrc/woq_gemv_xqs.h) and the all-reduce kernel emits the next GEMV's XQ vector itself; off = the
 * fp32-activation kernels. fused_push (default on, WOQ_TP_FUSED_PUSH=0 off; XQ path only): the row-parallel GEMVs
 * (o_proj, down_proj) store their partial sums into the peers' inboxes from their own epilogue, so the fabric flight runs
 * under the kernel boundary and the all-reduce kernel only pulls and sums; off = the all-reduce kernel pushes (the A/B
 * twin; results are bit-identical). Takes effect at the next step / capture. */
WOQ_API int woq_engine_set_tp_options(woq_engine* e, int xq, int fused_push);
/* run only the kernels of one sub-block, for TP where the collective is issued by the host
 * between them: phase 0 = embed + attention block up to o_proj partial, 1 = MLP block up to
 * down partial, 2 = head. layer ignored for phase 2. */
WOQ_API int woq_engine_phase(woq_engine* e, int layer, int phase, int greedy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WOQ_HIP_H_ */
