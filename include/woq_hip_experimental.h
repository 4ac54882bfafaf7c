/*
 * woq_hip_experimental.h — measurement hooks and lab switches of libwoq_hip.so.
 *
 * NOT part of the drop-in boundary (include/woq_hip.h) and NOT covered by WOQ_ABI_VERSION: these entry points exist
 * for bench.py's `roofline` / `prefill.dominant_gemm` objects, the A/B records under profiles/ and the GPU tests that
 * pin an experiment's results. They may change or disappear between rounds. No reference counterpart (the reference
 * has no timing hooks on qbits.cpp:113-140's path).
 */
#ifndef WOQ_HIP_EXPERIMENTAL_H_
#define WOQ_HIP_EXPERIMENTAL_H_

#include "woq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* grouped form only: `chunk` > 0 (a multiple of 32) = position-independent slice geometry — slice s owns the absolute
 * cached positions [s * chunk, (s + 1) * chunk) (the last slice also whatever lies beyond), so its K / V rows are
 * requested before the device-side position is read; 0 = slices cut evenly from the current span (the default; always
 * used with a sliding window). Pick splits >= ceil(positions / chunk). Same capture rule as attn_splits. */
WOQ_API int woq_engine_set_attn_chunk(woq_engine* e, int chunk);
WOQ_API int woq_engine_attn_chunk(woq_engine* e);
/* time the dominant kernel (int4 GEMV) alone over all layers with HIP events on `stream`: one pass = every layer's 4
 * GEMV launches in the forms the decode step uses (same kernels, epilogues, XQ outputs, residual chaining), captured
 * into a hipGraph and replayed `reps` times between one event pair (after an untimed replay); returns total ms, the
 * algorithmic bytes of one pass and its launch count (average launch duration = total_ms / (reps * launches_per_pass),
 * boundaries included). Overwrites the residual stream / XQ vectors (the next step's embedding rewrites them). */
WOQ_API int woq_engine_time_gemv(woq_engine* e, int reps, void* stream, float* total_ms, double* bytes_per_pass,
                                 int* launches_per_pass);
/* the same with a pass restricted to some of the layer's projections (mask bit 0 qkv, 1 o, 2 gate/up, 3 down): the
 * per-instantiation numbers rocprofv3's kernel stats list separately (bench.py roofline.by_projection) */
WOQ_API int woq_engine_time_gemv_mask(woq_engine* e, int mask, int reps, void* stream, float* total_ms,
                                      double* bytes_per_pass, int* launches_per_pass);
/* the same four launches per layer with the arithmetic taken out, timed the same way (`reps` passes after a warm-up
 * pass, total milliseconds): mode 0 = load-only twins (same grids, waves, K slices, non-temporal 16-byte requests over
 * the engine's own blobs: what this launch structure reaches as a pure stream), mode 1 = empty kernels on the same
 * grids (what the launches cost before they do anything). bench.py reports both as roofline.ceiling. */
WOQ_API int woq_engine_time_twin(woq_engine* e, int mode, int reps, void* stream, float* total_ms);
/* how woq_engine_time_gemv / _gemv_mask / _twin issue their timed passes: on != 0 (default) eagerly back to back on
 * the stream — the way decode bursts run by default since round 4 — else as replays of a captured graph. */
WOQ_API int woq_engine_set_time_eager(woq_engine* e, int on);
/* the prompt pass's dominant GEMM in place: the engine's own gate/up call of `layer` over n_rows rows of the residual
 * stream a preceding woq_engine_prefill left (RMSNorm pack pass + MFMA GEMM + SiLU * mul epilogue), the MEDIAN of `reps`
 * calls after a warm-up one: gemm_ms = the GEMM kernel alone (HIP events on the launch stream right around its launch),
 * call_ms = pack pass + GEMM. */
WOQ_API int woq_engine_time_prefill_gemm(woq_engine* e, int layer, int n_rows, int reps, void* stream, float* gemm_ms,
                                         float* call_ms);
/* forms of the most recent prefill-GEMM launches (launch_gemm_f16), oldest first, process-wide, at most 64 kept:
 * copies min(n, cap) of them into forms[], returns n, and empties the log (forms == NULL / cap == 0: just empties).
 * Each form is a bit set (mirrored in _lib.py GEMM_FORM_*): 1 fragment-image kernel (nf4 / fp4 / fp8 weights), 2 K slices
 * (split-K), 4 three-product fp32-class form, 8 hand-scheduled K loop, 16 half-tile ring layout, 32 256-row tiles,
 * 64 raw-A rows. Lets a test assert which kernel its shape ran. */
WOQ_API int woq_gemm_form_log(int* forms, int cap);
/* What launch_gemm_f16 would decide for one call, without touching a device (tests/test_gemm_plan_cpu.py): the header
 * is built with woq_header_init from (K, N, group, the woq_blob.h type codes, asym, act_shuffle); M rows of act_dtype
 * with row stride lda, `aligned` = the activation pointer is 16-byte aligned, has_norm = an RMSNorm weight is passed,
 * compute_type fp32 = the fp32-class form. fp8 != 0: the call of an fp8 weight (the header is then the HI plane's int4
 * one, weight_type is ignored). tall / tall_raw: the WOQ_GEMM_TALL / WOQ_GEMM_TALL_RAW switches (defaults 1 / 0).
 * out8 = {form bits, K slices, pack pass writes half-tile images, row blocks of the pack pass (0 = raw-A), workspace
 * bytes of this call, workspace bytes the caller-side sizing function answers for it, bytes of split-K partials, the
 * share the sizing reserves for them}. */
WOQ_API int woq_probe_gemm_plan(int K, int N, int group, int weight_type, int scale_type, int compute_type, int asym,
                                int act_shuffle, int M, int act_dtype, int lda, int aligned, int has_norm, int fp8,
                                int tall, int tall_raw, long long* out8);
/* one prompt-pass projection (tests/test_gpu_prefill_gemm_epilogues.py): forwards to launch_gemm_f16 unchanged, on
 * caller-owned device buffers and with the arguments the engine fixes left open. act [M][lda] in act_dtype, blob a packed
 * weight on the device (its header is read back, which synchronises the stream), norm_w fp32 [K] (nullable) with eps =
 * RMSNorm fused into the pack pass, epi 1 = SiLU(gate) * up over a fuse_gate_up blob (out [M][N / 2]; N % 32 != 0 is the
 * launcher's error), bias fp32 [N] (nullable), residual fp32 [M][ld_res] (nullable, may alias out), out [M][ldo] in
 * out_dtype, fp32_class != 0 = the three-product form. ws (nullable) / ws_bytes = a caller workspace: a fragment-image
 * call (nf4 / fp4 / fp8 weights) uses it only when ws_bytes covers the plan's bytes, else per-call scratch; any other
 * call must bring at least what the engine's sizing function asks for. An fp8 composite blob is split like woq_linear
 * splits it; an int8 composite (two chained calls) is refused. woq_gemm_form_log reports the form that ran. */
WOQ_API int woq_probe_gemm_f16(const void* act, int act_dtype, int lda, int M, const void* blob, const float* norm_w,
                               float eps, int epi, const float* bias, const float* residual, int ld_res, void* out,
                               int out_dtype, int ldo, int fp32_class, void* ws, size_t ws_bytes, void* stream);
/* Test entry points: the attention launches of the engine on caller-owned buffers, each forwarding to the engine's own
 * launcher unchanged (tests/test_gpu_attention_kernels.py). Caches [sequence][position][kv head][head_dim] in kv_dtype
 * (WOQ_F16 | WOQ_BF16 | WOQ_FP8_E4M3), `seq_stride_elems` elements between sequences; cos / sin fp32 [position][head_dim / 2].
 * rope_append: qkv fp16 [n_seq * T][(heads + 2 kv_heads) * head_dim], q rotated in place, rotated k and v appended at
 * positions start .. start + T - 1. attn_prefill: causal attention of the chunk's q rows over cache positions
 * [0, start + row], `window` > 0 = sliding window; out fp16 [n_seq * T][heads * head_dim]. */
WOQ_API int woq_probe_rope_append(void* qkv, int n_seq, int T, int start, int heads, int kv_heads, int head_dim,
                                  const float* cos_dev, const float* sin_dev, void* kcache, void* vcache, int kv_dtype,
                                  size_t seq_stride_elems, void* stream);
WOQ_API int woq_probe_attn_prefill(const void* qkv, int n_seq, int T, int start, int heads, int kv_heads, int head_dim,
                                   const void* kcache, const void* vcache, int kv_dtype, size_t seq_stride_elems,
                                   void* out, int window, void* stream);
/* one decode step's attention: qkv fp32 [(heads + 2 kv_heads) * head_dim] un-rotated, `pos_dev` = device int32 position
 * of the new token (k / v appended there), caches [max_ctx][kv_heads][head_dim], out fp32 [heads * head_dim].
 * splits > 1: context slices merged by the combine launch (merge 0) or by the last slice to arrive (merge 1, zeroed
 * counters); grouped != 0: the grouped-query matrix-core form where it applies, chunk_fixed as in
 * woq_engine_set_attn_chunk. The partial buffer and counters are allocated and freed on `stream`; no state is kept. */
WOQ_API int woq_probe_attn_decode(const float* qkv, void* kcache, void* vcache, int kv_dtype, const int32_t* pos_dev,
                                  const float* cos_dev, const float* sin_dev, int heads, int kv_heads, int head_dim,
                                  int max_ctx, int window, int splits, int grouped, int merge, int chunk_fixed,
                                  float* out, void* stream);
/* woq_probe_rope_append / woq_probe_attn_decode with the per-head q / k RMSNorm of woq_engine_set_layer_extras in front
 * of the rotation (tests/test_gpu_qknorm_kernels.py): q_norm_dev / k_norm_dev fp32 [head_dim], both required; the decode
 * probe runs the per-query-head form (the grouped form does not carry the norm). */
WOQ_API int woq_probe_rope_append_qknorm(void* qkv, int n_seq, int T, int start, int heads, int kv_heads, int head_dim,
                                         const float* cos_dev, const float* sin_dev, void* kcache, void* vcache,
                                         int kv_dtype, size_t seq_stride_elems, const float* q_norm_dev,
                                         const float* k_norm_dev, float eps, void* stream);
WOQ_API int woq_probe_attn_decode_qknorm(const float* qkv, void* kcache, void* vcache, int kv_dtype,
                                         const int32_t* pos_dev, const float* cos_dev, const float* sin_dev, int heads,
                                         int kv_heads, int head_dim, int max_ctx, int window, int splits, int merge,
                                         const float* q_norm_dev, const float* k_norm_dev, float eps, float* out,
                                         void* stream);
/* What plan_attn_decode (csrc/woq_attn_decode.hip) decides for one decode step's attention, without touching a device
 * (tests/test_attn_plan_cpu.py). in23 = {heads, kv_heads, head_dim, kv_dtype, max_ctx, window | splits, grouped, fold,
 * chunk_fixed, fuse_attn, fuse_sliced, grouped_a2a | xq step, granule buffers present, layers, slots (resident
 * workgroups of the grouped kernel, 0 = not covered) | the qkv blob as woq_header_init builds its header: K (0 = no
 * blob), group, weight_type, scale_type, asym, act_shuffle}; N is (heads + 2 kv_heads) * head_dim.
 * out11 = {form (0 fused into the qkv launch, 1 per query head, 2 grouped), merge (0 none, 1 combine launch, 2 arrival
 * counters, 3 among the slices), slices, effective chunk_fixed, span, positions per wave, LDS bytes, grid x, grid y,
 * launches of qkv projection + attention, refused}. Where the launch would fail: refused = 1, form and slices still say
 * what was tried, and the call returns non-zero with the launcher's error text. */
WOQ_API int woq_probe_attn_decode_plan(const int* in23, long long* out11);
/* the plan the engine's next step would follow for layer 0, as out11 above; splits > 0 / grouped >= 0 evaluate it at
 * that slice count / grouped request instead of the engine's own. The engine is not changed. A plan the launch would
 * refuse is an answer, not a failure of this call: it returns 0 with refused = 1 and the reason in woq_last_error. */
WOQ_API int woq_engine_attn_plan(woq_engine* e, int splits, int grouped, long long* out11);
/* the sampled token tail alone (tests/test_gpu_sampler_kernel.py), forwarding to the engine's own launcher unchanged:
 * logits fp32 [vocab], seen uint32 [(vocab + 31) / 32] (read for the penalty, the picked token's bit set), cfg in HOST
 * memory, u_or_null = device fp32 uniform that overrides Philox, pos_dev = device int32 position (the Philox counter;
 * not advanced), token_out device int32, philox_out4 (nullable) device uint32 [4], status (nullable) device int. */
WOQ_API int woq_probe_sample(const float* logits, int vocab, uint32_t* seen, const woq_sampler_config* cfg,
                             const float* u_or_null, const int32_t* pos_dev, int32_t* token_out, uint32_t* philox_out4,
                             int* status, void* stream);
/* woq_probe_sample with the word a rolling KV cache keeps (woq_engine_discarded_ptr, or any device int32; NULL = 0): the
 * Philox counter is *pos_dev + *discarded_dev with uint32 wrap (tests/test_gpu_streaming_engine.py). */
WOQ_API int woq_probe_sample_stream(const float* logits, int vocab, uint32_t* seen, const woq_sampler_config* cfg,
                                    const float* u_or_null, const int32_t* pos_dev, const int32_t* discarded_dev,
                                    int32_t* token_out, uint32_t* philox_out4, int* status, void* stream);
/* the token tail with sampler controls alone (tests/test_gpu_sampler_controls_kernel.py), forwarding to the engine's own
 * launcher: as woq_probe_sample, plus counts uint32 [vocab] (read by the pre-pass, the picked token's entry + 1), ctl
 * and its n_bias (id, value) pairs in HOST memory, adjusted_out = device fp32 [vocab] that receives the pre-pass's
 * scores (bias, repetition / frequency / presence penalty; before the temperature), kept_out (nullable) = device uint32
 * that a sampled draw sets to the number of ids it was over (after top-k, top-p and min_p). A refused configuration
 * returns non-zero before anything is launched. */
WOQ_API int woq_probe_sample_controls(const float* logits, int vocab, uint32_t* seen, uint32_t* counts,
                                      const woq_sampler_config* cfg, const woq_sampler_controls* ctl,
                                      const int32_t* bias_ids_host, const float* bias_vals_host, const float* u_or_null,
                                      const int32_t* pos_dev, int32_t* token_out, float* adjusted_out,
                                      uint32_t* kept_out, int* status, void* stream);
/* the token tail with a token guide alone (tests/test_gpu_guide_kernel.py), forwarding to the engine's own launchers:
 * as woq_probe_sample_controls, plus table_dev = device uint16_t [n_states][vocab], `state` = the state whose row masks
 * the scores, `advance_state` = the state the advance starts from (< 0: `state`; another one lets a test hand the
 * advance a pick that its row bans), state_out = device int32 that receives the state after the advance. status bit 4:
 * the pick was banned in the advance's row (the state stayed). */
WOQ_API int woq_probe_guide(const float* logits, int vocab, uint32_t* seen, uint32_t* counts,
                            const woq_sampler_config* cfg, const woq_sampler_controls* ctl,
                            const int32_t* bias_ids_host, const float* bias_vals_host, const uint16_t* table_dev,
                            int n_states, int state, int advance_state, const float* u_or_null, const int32_t* pos_dev,
                            int32_t* token_out, float* adjusted_out, int32_t* state_out, int* status, void* stream);
/* the log-probability record alone (tests/test_gpu_logprob_kernel.py), forwarding to the engine's own launcher
 * unchanged: logits fp32 [vocab], token_dev = device int32 id whose log-probability goes to chosen_out[0];
 * top_id_out20 / top_lp_out20 = device int32 / fp32 [20]. Scratch is allocated and freed on `stream`. */
WOQ_API int woq_probe_logprobs(const float* logits, int vocab, const int32_t* token_dev, float* chosen_out,
                               int32_t* top_id_out20, float* top_lp_out20, void* stream);
/* the scored head alone (tests/test_gpu_score_kernel.py), forwarding to the engine's own launcher unchanged (csrc/
 * woq_score.hip): hidden_rows fp32 [M][hidden], norm_w fp32 [hidden], W = dense lm_head [vocab][hidden] in w_dtype
 * (WOQ_F16 | WOQ_BF16), targets = device int32 [M]; row r's record goes to chosen_out[r], top_id_out[r][0..20),
 * top_lp_out[r][0..20). Scratch is allocated and freed on `stream`. */
WOQ_API int woq_probe_score_rows(const float* hidden_rows, const float* norm_w, float eps, const void* W, int w_dtype,
                                 int hidden, int vocab, const int32_t* targets, int M, float* chosen_out,
                                 int32_t* top_id_out, float* top_lp_out, void* stream);
/* The XQ decode GEMV and the greedy token tail alone (tests/test_gpu_xq_gemv_kernel.py, tests/test_gpu_token_tail_kernel.py),
 * each forwarding to the engine's own launcher unchanged. An XQ vector of K values (csrc/woq_xq.h) is three device
 * buffers: limbs (((K / 16 * 48 + 1023) / 1024 + 1) * 1024 bytes, [K / 16][3][16] int8 used), u and sx fp32 [K / 16].
 * xq_from_f32: x fp32 [K] (times norm_w when given), K % 16 == 0; ssq_out (nullable) fp32 [K / 16] = the blocks' sums
 * of squares of x. */
WOQ_API int woq_probe_xq_from_f32(const float* x, const float* norm_w, int K, void* limbs_out, float* u_out,
                                  float* sx_out, float* ssq_out, void* stream);
/* one batch-1 projection: x fp32 [K] is converted (times in_norm_w when given) to an XQ vector in scratch allocated and
 * freed on `stream`, then the GEMV runs over `blob` (device memory; its header is read back, which synchronises the
 * stream): out fp32 [N] (epi 1, a fuse_gate_up blob: SiLU(gate) * up, [N / 2]) = x . W (* rsqrt(mean(x^2) + eps) exactly
 * when in_norm_w is given) (+ bias [N]) (+ residual); xo_* (nullable together) = the result times next_norm_w (nullable)
 * as an XQ vector of Npad (epi 1: Npad / 2) values, ssq_out (nullable) its blocks' sums of squares. out may be null when
 * xo is given. Returns the library's error when the GEMV refuses the call. */
WOQ_API int woq_probe_gemv_xq(const float* x, const float* in_norm_w, float eps, const void* blob, int epi,
                              const float* bias, const float* residual, const float* next_norm_w, float* out,
                              void* xo_limbs, float* xo_u, float* xo_sx, float* ssq_out, void* stream);
/* The LoRA adapter kernels alone (csrc/woq_lora.hip; tests/test_gpu_lora_kernel.py), each forwarding to the engine's own
 * launcher unchanged. A projection's adapter is given as host arrays of n_parts (1..3) entries: a_dev[p] = device fp32
 * A_p [ranks[p]][K], b_dev[p] = device fp32 B_p [cols[p]][ranks[p]], scalings[p] = lora_alpha / r; ranks[p] == 0 = the
 * part has no adapter (its pointers are not read); cols[p] % 16 == 0 and their sum is N. interleave != 0 (two parts,
 * gate and up): the N blob columns alternate gate / up in 16-column tiles (runtime.fuse_gate_up).
 * delta, the decode step's launch: out fp32 [N] = base_bias (nullable = 0) + s_p * B_p . (inv * A_p . x).
 *   form 0: x / xq_u / xq_sx = an XQ vector of K values (woq_probe_xq_from_f32), aux = its K / 16 sums of squares
 *           (nullable; given: inv = 1 / sqrt(sum(aux) / K + eps), else 1)
 *   form 1: x fp32 [K], aux = a norm weight fp32 [K] (nullable; given: x * aux and inv = 1 / sqrt(mean(x^2) + eps))
 * shrink, the prompt pass's first launch: T fp32 [M][ldt], columns 0 .. sum(ranks) = inv_m * A_p . (X[m] * norm_w) over the
 *   stacked rows of the parts; X fp32 [M][ldx] (norm_w nullable) or fp16 (x_dtype WOQ_F16, norm_w NULL).
 * expand, its second: mode 0 out fp32 [M][ldo] += s_p * T[m] . B_p^T, mode 1 the same on fp16, mode 2 (interleave, gu =
 *   fp16 [M][ld_gu] gate/up rows in blob column order) out fp16 [M][ldo], N / 2 columns, = SiLU(gate + D) * (up + D). */
WOQ_API int woq_probe_lora_delta(int form, const void* x, const float* xq_u, const float* xq_sx, const float* aux,
                                 float eps, int K, int N, int n_parts, int interleave, const void* const* a_dev,
                                 const void* const* b_dev, const int* ranks, const int* cols, const float* scalings,
                                 const float* base_bias, float* out, void* stream);
WOQ_API int woq_probe_lora_shrink(const void* X, int x_dtype, int ldx, int M, int K, const float* norm_w, float eps,
                                  int n_parts, const void* const* a_dev, const int* ranks, float* T, int ldt,
                                  void* stream);
WOQ_API int woq_probe_lora_expand(int mode, const float* T, int ldt, int M, int N, int n_parts,
                                  const void* const* b_dev, const int* ranks, const int* cols, const float* scalings,
                                  void* out, int ldo, const void* gu, int ld_gu, void* stream);
/* The tensor-parallel exchange alone (tests/test_gpu_tp_kernels.py), each forwarding to the engine's own launcher
 * unchanged. Every rank of a connected communicator issues the same chain of collectives.
 * gemv_xq_tp: woq_probe_gemv_xq whose last chained launch also pushes its live output columns, this rank's partial sums,
 * into the peers' inboxes under the sequence number of the all-reduce that must follow with pushed != 0. */
WOQ_API int woq_probe_gemv_xq_tp(const float* x, const float* in_norm_w, float eps, const void* blob, int epi,
                                 const float* bias, const float* residual, const float* next_norm_w, float* out,
                                 void* xo_limbs, float* xo_u, float* xo_sx, float* ssq_out, void* stream,
                                 woq_comm* comm);
/* in-place sum over ranks of buf[0..n) in rank order from 0.f (woq_comm_launch_allreduce_ex): pushed != 0 = the
 * contribution is already in the peers' inboxes (woq_probe_gemv_xq_tp); xo_* (nullable together; n % 16 == 0) = the sum
 * times norm_w (nullable) as an XQ vector, ssq_out (nullable) fp32 [n / 16] = the blocks' sums of squares of the sum. */
WOQ_API int woq_probe_comm_allreduce(woq_comm* comm, float* buf, size_t n, int pushed, const float* norm_w,
                                     void* xo_limbs, float* xo_u, float* xo_sx, float* ssq_out, void* stream);
/* the greedy pick over a vocab-sharded lm_head's (max, local index) pairs (woq_comm_launch_greedy): token[0] = the
 * global index of the highest value over all ranks, lowest index on ties, log[pos[0]] = token (log nullable), pos[0] += 1;
 * no pair won on any rank: token 0 and status (nullable, device int) |= 4. */
WOQ_API int woq_probe_comm_greedy(woq_comm* comm, const float* pmax, const int32_t* pidx, int n_pairs, int vocab_offset,
                                  int32_t* token, int32_t* pos, int32_t* log, int* status, void* stream);
/* sets the sequence number of the next collective (never 0), stream-ordered. Test only: every rank calls it with the
 * same value while no collective of any rank is in flight (synchronise and meet first — a peer still pulling from the
 * buffer the new parity selects would lose its data), and on an inbox that holds none of the tags the sequence will
 * reach (the same tag on a stale granule reads as arrived). */
WOQ_API int woq_probe_comm_set_seq(woq_comm* comm, unsigned int seq, void* stream);
/* lm_head_kernel: hidden_in / norm_w fp32 [hidden] (hidden % 8 == 0), W dense [vocab][hidden] in w_dtype (WOQ_F16 |
 * WOQ_BF16), logits fp32 [vocab]; pmax / pidx (nullable together) fp32 / int32 [(vocab + 15) / 16]: each 16-row
 * workgroup's (max logit, lowest index of it). */
WOQ_API int woq_probe_lm_head(const float* hidden_in, const float* norm_w, float eps, const void* W, int w_dtype,
                              int hidden, int vocab, float* logits, float* pmax, int32_t* pidx, void* stream);
/* the greedy tails: mode 0 = argmax over logits [vocab] (the prompt pass's), mode 1 = argmax over the lm_head's
 * (vocab + 15) / 16 pairs (the eager step's), mode 2 = the same fused with the next step's embedding (chained steps).
 * All write token[0], pos[0] += 1; modes 1 and 2 also log[old pos] = token (log nullable) and status |= 4 when no pair
 * won (token 0). Modes 0 and 1 read none of the arguments from `embed` on. Mode 2: embed [rows][hidden] in embed_dtype,
 * out fp32 [hidden] = the token's row; with norm_w the row times norm_w also leaves as the XQ vector xo_* with ssq_out;
 * step_seq (nullable) += 1; a position that reaches max_ctx is clamped to max_ctx - 1 and status |= 2. */
WOQ_API int woq_probe_greedy_tail(int mode, const float* logits, int vocab, const float* pmax, const int32_t* pidx,
                                  int32_t* token, int32_t* pos, int32_t* log, const void* embed, int embed_dtype,
                                  int hidden, float* out, const float* norm_w, void* xo_limbs, float* xo_u, float* xo_sx,
                                  float* ssq_out, unsigned int* step_seq, int max_ctx, int* status, void* stream);
/* embed_kernel, the head of a decode step: the same outputs as mode 2 for the row of token[0]; pos (nullable) is only
 * guarded (pos >= max_ctx: clamped, status |= 2), step_seq (nullable) += 1. */
WOQ_API int woq_probe_embed(const void* embed, int embed_dtype, const int32_t* token, int hidden, float* out,
                            const float* norm_w, void* xo_limbs, float* xo_u, float* xo_sx, float* ssq_out,
                            unsigned int* step_seq, int32_t* pos, int max_ctx, int* status, void* stream);
/* one projection of the fp32-activation decode step (tests/test_gpu_f32_gemv_kernel.py), run exactly as the engine runs
 * it but on caller-owned device buffers and with the arguments the engine fixes left open: x [M][lda] in x_dtype, blob a
 * packed weight on the device (its header is read back, which synchronises the stream), norm_w fp32 [K] (nullable) with
 * eps = the fused RMSNorm, epi 1 = SiLU(gate) * up over a fuse_gate_up blob (out [M][N / 2]), bias fp32 [N] (nullable),
 * residual fp32 [M][ld_res] (nullable, may alias out), out [M][ldo] in out_dtype. An fp8 composite blob is split like
 * woq_linear splits it and goes to the engine's fp8 launcher, which takes M = 1, fp32 rows and no bias (anything else is
 * an error); its epi 1 form needs gu_tmp = fp32 [N] of device scratch, without it the lookup kernel runs. Every other
 * blob goes to the small-M dispatch. form_out (host, nullable) = {kernel, chained launches, waves, tiles per wave} of the
 * launch, from the predicates the launchers themselves call: kernel 0 = generic / lookup (one launch, 4 waves, tiles per
 * wave 0), 1 = the int8-MFMA tile kernel, 2 = the fp8 matrix-core kernel; waves and tiles per wave are those of the first
 * chained launch. */
WOQ_API int woq_probe_gemv_f32(const void* x, int x_dtype, int lda, int M, const void* blob, const float* norm_w,
                               float eps, int epi, const float* bias, const float* residual, int ld_res, void* out,
                               int out_dtype, int ldo, float* gu_tmp, int* form_out, void* stream);
/* fp32 [rows][hidden]: the residual stream the last prompt pass left (before the final norm), valid until the next
 * prompt pass; NULL before the first one. For tests. */
WOQ_API void* woq_engine_prefill_rows_ptr(woq_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* WOQ_HIP_EXPERIMENTAL_H_ */
