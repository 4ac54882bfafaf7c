// woq_host.h — the host functions the library's translation units call across files, declared once, default arguments
// included; every defining file includes it too. Declarations only: no device code (error / scratch plumbing: woq_launch.h).
#pragma once
#include "woq_comm_dev.h"
#include "woq_launch.h"
#include "woq_xq.h"

namespace woq {
struct LutArgs;    // woq_gemv_common.h
struct KPlan;      // woq_gemv_launch.h

// ---- woq_gemv.hip: small-M dispatch ------------------------------------------------------------------------------
// Shared by woq_linear and the decode engine: rows in chunks through the i8 tile kernel when the call qualifies,
// through the generic kernel otherwise.
int launch_gemv_from_header(const void* act, int act_dtype, int lda, const void* blob, const woq_blob_header& h,
                            const float* bias, void* out, int out_dtype, int ldo, int M, const float* norm_w,
                            float eps, const float* residual, int ld_res, int epi, hipStream_t st);
// fp8 weights at decode row counts: the fp8-MFMA kernel (woq_gemv_fp8.hip: code bytes straight into the matrix cores,
// activations as base-16 digits; round 4) where it takes the call, rows in chunks of 8; otherwise (per-32 / per-64 /
// per-256 scales, g_idx, misaligned rows, K beyond 8192) the lookup kernel reading both nibble planes, rows in chunks of GEN_MAXM.
// `hi` = the HI plane's header (scales, shuffle), `lo_q` = the LO plane's qdata.
int launch_gemv_fp8(const void* act, int act_dtype, int lda, const void* hi_blob, const woq_blob_header& hi,
                    const void* lo_q, uint32_t fp8_type, const float* bias, void* out, int out_dtype, int ldo, int M,
                    hipStream_t st);
// One batch-1 projection of an fp8-weight layer inside the decode engine (round 6): fp32 activation row in, fp32 out,
// with the engine's fused prologue / epilogues — RMSNorm (norm_w, eps), residual add, and for the fused gate/up
// projection (epi 1) SiLU(gate) * up. The fp8 matrix-core kernel (woq_gemv_fp8.hip) carries the norm and the residual
// itself; its gate/up call writes the 2 * inter interleaved columns to `gu_tmp` and a small launch pairs them. Blobs it
// does not take (g_idx, groups of 256, K beyond 12288) run the lookup kernel, which has all three built in.
int launch_gemv_fp8_engine(const float* act, int lda, const void* hi_blob, const woq_blob_header& hi, const void* lo_q,
                           uint32_t fp8_type, float* out, int ldo, const float* norm_w, float eps, const float* residual,
                           int ld_res, int epi, float* gu_tmp, hipStream_t st);

// ---- woq_gemv_i8.hip: the tile GEMV -------------------------------------------------------------------------------
// the digit planes of a table weight type; returns NDIG (1 | 2 | 3), 0 = not a table. compute_type (woq_blob.h):
// nf4 takes three planes for fp32 compute and two (table held to 2^-16 of its largest entry — finer than the bf16 / fp16
// operands those modes ask for) otherwise
int lut_args_for(uint32_t weight_type, uint32_t compute_type, LutArgs& L);
// geometry pick: nw waves x tpw tiles cover tiles_k (8 tiles = 8 KiB per wave per column tile; 4 for short K so
// that a workgroup still has a few waves). Returns false when this kernel does not take the shape (K > 16384).
bool gemv_tile_geometry(int tiles_k, int cb, int smode, int& nw, int& tpw);
// the chained launches of one call (woq_gemv_launch.h KPlan: chunks, tiles per chunk, nw x tpw of every chunk; K ranges
// one launch cannot hold are split only for linear epilogues — epi 0, no norm, fp32 out); chunks == 0 = not covered
KPlan gemv_tile_k_plan(const woq_blob_header& h, const float* norm_w, int epi, int out_dtype);
// largest M the tile kernel takes for this call (LDS budget), 0 if it is not covered: the kernel wants unshuffled
// activation rows, fp32 and 16-B aligned (what the decode engine feeds it and what the reference's qbits boundary
// always holds, modules.py:152-154) or fp16 / bf16 and 8-B aligned; anything else goes to the generic kernel in
// woq_gemv.hip.
int gemv_tile_max_rows(const void* act, int act_dtype, int lda, const woq_blob_header& h, const float* norm_w,
                       int epi, int out_dtype);
// rows 0..M-1 (M <= gemv_tile_max_rows). x: [M, lda]; out: [M, ldo]; residual: [M, ld_res] or null.
int launch_gemv_tile(const void* act, int act_dtype, int lda, int M, const void* blob, const woq_blob_header& h,
                     const float* bias, void* out, int out_dtype, int ldo, const float* norm_w, float eps,
                     const float* residual, int ld_res, int epi, hipStream_t st);

// ---- woq_gemv_fp8.hip: the fp8 matrix-core GEMV -------------------------------------------------------------------
// Does the fp8-MFMA kernel take this call? `hi` = the HI plane's header (scales; the LO plane has the same geometry).
bool gemv_fp8_mfma_supported(const void* act, int act_dtype, int lda, const woq_blob_header& hi);
// its geometry: nw waves x tpw tiles of both planes cover tiles_k; false when it does not take the K (beyond 12288)
bool fp8_geometry(int tiles_k, int& nw, int& tpw);
// rows 0..M-1 (M <= 8) of an fp8 weight: act [M, lda], out [M, ldo]
int launch_gemv_fp8_mfma(const void* act, int act_dtype, int lda, int M, const void* hi_blob, const woq_blob_header& hi,
                         const void* lo_q, uint32_t fp8_type, const float* bias, void* out, int out_dtype, int ldo,
                         hipStream_t st, const float* norm_w = nullptr, float eps = 0.f, const float* residual = nullptr,
                         int ld_res = 0);
// act[p * 16 + i] = SiLU(gu[(2 p) * 16 + i]) * gu[(2 p + 1) * 16 + i] (silu_mul_tiles_kernel)
void launch_silu_mul_tiles(const float* gu, int inter, float* act, hipStream_t st);

// ---- woq_gemv_xq.hip: batch-1 GEMV over an XQ activation vector ---------------------------------------------------
// does the XQ kernel take this blob as a batch-1 projection? epi 1 = fused gate/up (SiLU * mul)
bool gemv_xq_supported(const woq_blob_header& h, int epi);
// out[N] (fp32, may be null when only the XQ output is wanted) = xin . W_deq (* rsqrt(mean(x^2) + eps) when ssq_in)
// (+ bias) (+ residual), SiLU(gate) * up for epi 1; xo (optional): the result as the next kernel's XQ vector, after
// multiplying by next_norm_w (optional), with its per-block sums of squares in ssq_out (optional).
int launch_gemv_xq(const XqPtrs& xin, const void* blob, const woq_blob_header& h, const float* bias, float* out,
                   const float* ssq_in, float eps, const float* residual, int epi, const XqPtrs& xo,
                   const float* next_norm_w, float* ssq_out, hipStream_t st, const CommDev* tp);
// fp32 x[K] (times norm_w when given; K % 16 == 0) -> XQ vector xo, ssq_out (nullable) = per-block sums of squares of x
void launch_xq_from_f32(const float* x, const float* norm_w, int K, const XqPtrs& xo, float* ssq_out, hipStream_t st);
// mode 0: load-only twin of the batch-1 GEMV of this blob; mode 1: an empty kernel on the same grid and block
int launch_gemv_twin(const void* blob, const woq_blob_header& h, int epi, int mode, unsigned int* sink, hipStream_t st);

// ---- woq_attn_decode.hip: a decode step's attention — the plan and the separate launches --------------------------
// A step's attention runs in one of three forms — FUSED: attention workgroups behind the qkv GEMV's strips, one launch
// (woq_gemv_attn.hip); PER_HEAD / GROUPED: qkv GEMV, then one workgroup per (query head, slice) / one matrix-core
// workgroup per (kv head, slice) — and its context slices merge in one of three ways: a COMBINE launch, the last slice
// workgroup to arrive (COUNTER) or the slices among themselves through tagged granules (A2A; both woq_attn_merge.h).
enum AttnForm { ATTN_FUSED = 0, ATTN_PER_HEAD = 1, ATTN_GROUPED = 2 };
enum AttnMergeMode { ATTN_MERGE_NONE = 0, ATTN_MERGE_COMBINE = 1, ATTN_MERGE_COUNTER = 2, ATTN_MERGE_A2A = 3 };
struct AttnShape { int heads, kv_heads, head_dim, kv_dtype, max_ctx, window; };
struct AttnOptions {  // what is asked for; the plan says what runs
  int splits = 1;        // context slices per head (<= 1: none)
  bool grouped = false;  // the grouped form, where it applies
  bool fold = false;     // merge by arrival counters (WOQ_ATTN_FOLD=1; measured slower than the combine launch)
  int chunk_fixed = 0;   // grouped form: positions per slice of the position-independent geometry, 0 = adaptive
  bool fuse_attn = true, fuse_sliced = true;  // the fused launch where the shape allows; context slices in it as well
  bool grouped_a2a = true;  // grouped slices merge among themselves where the whole grid is resident
};
struct AttnFacts {  // what the engine is
  bool xq, granules;  // the XQ step (the fp32-activation one never fuses, never merges A2A); the granule buffers exist
  int layers;         // hand-off tags are (step << 6) | layer: at most 64 layers
  const woq_blob_header* qkv_hdr;  // the layer's qkv blob (nullable = no fused launch)
  int slots;          // attn_decode_mfma_slots for this shape, 0 = not covered
  bool qk_norm = false;  // the layer has a per-head q / k RMSNorm: the grouped form does not carry it (falls to per-head)
};
struct AttnDecodePlan {
  AttnShape shape;
  AttnForm form;
  AttnMergeMode merge;
  int slices, chunk_fixed;  // >= 1; GROUPED: the geometry that runs (no multiple of 32 -> 0, adaptive)
  int span, spw;            // FUSED / PER_HEAD: positions a workgroup / a wave may hold scores for (woq_attn_decode.h)
  size_t lds;               // dynamic LDS bytes of an attention workgroup
  unsigned grid_x, grid_y;  // of the launch that holds the attention workgroups
  int launches;             // qkv projection and attention together
  const char* error;        // null, or why launch_attn_decode will refuse (the other fields then mean nothing)
};
// Decides once how the attention of a step runs. Pure host arithmetic: no HIP call, no environment, no statics.
AttnDecodePlan plan_attn_decode(const AttnShape& s, const AttnOptions& o, const AttnFacts& f);
// a plan as the probes report it: {form, merge, slices, chunk_fixed, span, spw, LDS bytes, grid x, grid y, launches,
// refused}; refused = 1: launch_attn_decode would fail, and the error text (woq_last_error) is set to the reason
void attn_plan_report(const AttnDecodePlan& p, long long* out11);
// the device buffers of one layer's attention; which of them a launch touches follows from the plan
struct AttnDecodeIO {
  const float* qkv;       // fp32 [(heads + 2 kv_heads) * D] un-rotated projections (the separate launches' input)
  void *kcache, *vcache;  // [max_ctx][kv_heads][D]; the new k / v are appended at *pos
  const int32_t* pos;
  const float *cs, *sn;
  float* out;             // fp32 [heads * D], and `xo` its XQ form for the o_proj GEMV (or all null)
  XqPtrs xo;
  float* part;            // fp32 partials of the slices (layout: woq_attn_merge.h)
  unsigned int* counters; // COUNTER: [heads] words, zero between launches
  unsigned long long* part_g;  // A2A: {tag, fp32} partial granules [heads][64][D + 2]
  const unsigned int* seq;     // FUSED / A2A: device-side step counter, tag = seq << 6 | layer
  int layer;
  int* status;            // sticky give-up flag
  // per-head RMSNorm of q and of the new k over D BEFORE the rotation (Qwen3): fp32 [D] weights, both or neither
  const float *q_norm = nullptr, *k_norm = nullptr;
  float qk_eps = 0.f;
};
// the attention launch(es) of a PER_HEAD or GROUPED plan; a plan with an error text fails with it
int launch_attn_decode(const AttnDecodePlan& plan, const AttnDecodeIO& io, hipStream_t st);
// workgroups of the grouped decode attention kernel the chip holds at once (0 = shape not covered): the all-to-all
// merge needs the whole grid resident. Asks the device once per (cache type, group size) and remembers.
int attn_decode_mfma_slots(int kv_dtype, int rep);

// ---- woq_gemv_attn.hip: [RMSNorm + qkv GEMV] + [RoPE + KV append + attention] in one launch -----------------------
// A FUSED plan's launch. qkv_g ({tag, fp32} granules [(heads + 2 kv_heads) * 128]) = xin . W_qkv_deq *
// rsqrt(mean(x^2) + eps); per head, as its granules arrive: RoPE, KV append at *io.pos, attention over the cache ->
// io.out (+ io.xo). plan.slices > 1: context slices per head; they merge among themselves through io.part_g and write
// io.out / io.xo — no combine launch.
// bias (nullable): fp32 [N], added in the strips' epilogue after the RMSNorm factor (Qwen2's q / k / v biases)
int launch_gemv_xq_attn(const AttnDecodePlan& plan, const AttnDecodeIO& io, const XqPtrs& xin, const void* blob,
                        const woq_blob_header& h, unsigned long long* qkv_g, const float* ssq_in, float eps,
                        hipStream_t st, const float* bias = nullptr);

// ---- woq_ops.hip: the decode step's other launches ----------------------------------------------------------------
void launch_embed(const void* embed, int dtype, const int32_t* token, int hidden, float* out, const float* norm_w,
                  const XqPtrs& xo, float* ssq_out, unsigned int* step_seq, int32_t* pos, int max_ctx, int* status,
                  hipStream_t st);
// pmax / pidx (nullable): per-workgroup (max logit, its index), (vocab + 15) / 16 entries each
void launch_lm_head(const float* hidden_in, const float* norm_w, float eps, const void* W, int w_dtype, int hidden,
                    int vocab, float* logits, float* pmax, int32_t* pidx, hipStream_t st);
void launch_argmax(const float* logits, int vocab, int32_t* token, int32_t* pos, hipStream_t st);
// greedy token from the (max, index) pairs of launch_lm_head; no pair won (every logit NaN or -inf): token 0 and
// status (nullable) |= 4, the rule of launch_argmax_embed
void launch_argmax_pairs(const float* pmax, const int32_t* pidx, int n, int32_t* token, int32_t* pos, int32_t* log,
                         int* status, hipStream_t st);
// greedy token of the step that just ran its lm_head + embedding row of the NEXT step, one launch (argmax_embed_kernel)
void launch_argmax_embed(const float* pmax, const int32_t* pidx, int n, int32_t* token, int32_t* pos, int32_t* log,
                         const void* embed, int dtype, int hidden, float* out, const float* norm_w, const XqPtrs& xo,
                         float* ssq_out, unsigned int* step_seq, int max_ctx, int* status, hipStream_t st);

// ---- woq_sample.hip: the sampled token tail -----------------------------------------------------------------------
// A token guide (include/woq_hip.h woq_engine_set_guide): a dense table next[n_states][vocab] of uint16, GUIDE_BANNED =
// the id is banned in that state, anything else = the state after that id. The kernels read the table pointer and the
// state from this device struct, so another table or another state needs no new capture.
constexpr uint16_t GUIDE_BANNED = 0xFFFFu;
struct GuideState {
  const uint16_t* table;
  int32_t n_states;
  int32_t state;
};
// The device buffers of one sampled pick; which of them are set decides what launch_sample_tail runs.
//  - `adj` null: next token from the fp32 `logits` under the device-resident `cfg` (repetition penalty over the `seen`
//    bit set, then argmax or temperature / top-k / top-p / draw), one launch of one workgroup (sample_kernel<false>).
//  - `adj` set (sampler controls): a pre-pass over the whole chip (score_adjust_kernel<false>) writes adj[i] = the score
//    of id i after the logit bias (dense table `bias`, NaN = no entry), the repetition penalty and the frequency /
//    presence penalties over `counts` (uint32 [vocab], times generated), then the sampling workgroup runs over `adj`
//    (sample_kernel<true>: min_p from `ctl`) and also does counts[token] += 1. Two launches whose shapes depend on the
//    vocabulary alone; `logits` is only read.
//  - `guide` set as well: the pre-pass (score_adjust_kernel<true>) ends on adj[i] = -inf where
//    table[state * vocab + i] == GUIDE_BANNED (the row offset in 64 bits). The state is only read.
// pos_advance (the engine's chain): the Philox counter is *pos_advance + *discarded, log[*pos_advance] = token (`log`
// nullable), then *pos_advance += 1; else pos_fixed is only read. `discarded` (nullable = 0): the positions a rolling KV
// cache has dropped so far (woq_engine_kv_shift), which makes the counter the token's absolute index in the stream, with
// uint32 wrap. Sets the token's bit in `seen`; status |= 4 (every score NaN: token 0), 8 (more than 1024 candidates
// tied in).
struct SampleTail {
  const float* logits = nullptr; int vocab = 0; uint32_t* seen = nullptr; const woq_sampler_config* cfg = nullptr;
  // the controls' memory, all four or none; a guide needs it
  uint32_t* counts = nullptr; const float* bias = nullptr; const woq_sampler_controls* ctl = nullptr; float* adj = nullptr;
  const GuideState* guide = nullptr;
  int32_t *token = nullptr, *pos_advance = nullptr, *log = nullptr; const int32_t* pos_fixed = nullptr; int* status = nullptr;
  const int32_t* discarded = nullptr;
  // the probes' (null in the engine): u overrides the Philox uniform, philox_out receives the four Philox words,
  // kept_out (controls) the number of ids a sampled draw was over
  const float* u = nullptr; uint32_t *philox_out = nullptr, *kept_out = nullptr;
};
int launch_sample_tail(const SampleTail& t, hipStream_t st);  // non-zero (message set): the slots contradict each other
// seen |= bits of tokens[0..n) (ids outside [0, vocab) are ignored)
void launch_sampler_seen(uint32_t* seen, int vocab, const int32_t* tokens, int n, hipStream_t st);
// *dst = cfg, stream-ordered (the struct travels as a kernel argument)
void launch_sampler_config_store(const woq_sampler_config& cfg, woq_sampler_config* dst, hipStream_t st);
// null when the native sampler takes this combination, else the "QBits: ..." reason
const char* sampler_config_problem(const woq_sampler_config& cfg);
// counts[tokens[j]] += 1 for j in [0, n) (ids outside [0, vocab) are ignored)
void launch_sampler_counts(uint32_t* counts, int vocab, const int32_t* tokens, int n, hipStream_t st);
// bias[0..vocab) = NaN ("no entry"), then bias[ids_dev[j]] = vals_dev[j] for j in [0, n); stream-ordered
int launch_sampler_bias_store(float* bias, int vocab, const int32_t* ids_dev, const float* vals_dev, int n, hipStream_t st);
void launch_sampler_controls_store(const woq_sampler_controls& ctl, woq_sampler_controls* dst, hipStream_t st);
// null when the controls are acceptable beside `cfg` (ids / vals: ctl.n_bias host entries), else the "QBits: ..." reason
const char* sampler_controls_problem(const woq_sampler_controls& ctl, const woq_sampler_config& cfg, int vocab,
                                     const int32_t* ids, const float* vals);
// after a guided pick, one thread: state <- table[state * vocab + token[0]], or, where that is GUIDE_BANNED (or no state of
// the table), the state stays and status |= 16
void launch_guide_advance(GuideState* guide_dev, int vocab, const int32_t* token, int* status, hipStream_t st);
void launch_guide_state_store(GuideState* guide_dev, int32_t state, hipStream_t st);  // stream-ordered, capturable
// null when (n_states, start_state) describe a table the guide takes, else the "QBits: ..." reason
const char* guide_problem(int n_states, int start_state);

// ---- woq_kv_shift.hip: the rolling KV cache's shift ---------------------------------------------------------------
// One sequence's caches kseq / vseq ([layers][max_ctx][kv_heads * D] in kv_dtype), in place: for p in
// [n_keep + n_discard, n_cached) V[p - n_discard] = V[p] and K[p - n_discard] = K[p] rotated back by row n_discard of the
// fp32 tables cs / sn ([max_ctx][D / 2]; the row is read only when rows move). Each thread owns columns and walks the
// positions in ascending order, so the overlapping ranges need no order between workgroups. One launch, capturable.
// Non-zero (message set) for a geometry outside 0 <= n_keep, 1 <= n_discard, n_keep + n_discard <= n_cached <= max_ctx.
int launch_kv_shift(void* kseq, void* vseq, int kv_dtype, int layers, int kv_heads, int D, int max_ctx, const float* cs,
                    const float* sn, int n_keep, int n_discard, int n_cached, hipStream_t st);
// pos -= n_discard, discarded += n_discard (uint32 wrap), one thread, stream-ordered
void launch_kv_shift_words(int32_t* pos, int32_t* discarded, int n_discard, hipStream_t st);
void launch_i32_store(int32_t* dst, int32_t v, hipStream_t st);  // *dst = v, stream-ordered, capturable

// ---- woq_logprob.hip: the log-probability record of a chaining step ----------------------------------------------
// After the pick: row p = *pos - 1 of the three logs (pos null: row 0) <- log_softmax over the raw fp32 logits at
// token[0] (chosen [max_rows]) and at the 20 best ids by (logit descending, id ascending) (top_id / top_lp
// [max_rows][20], padded with -1 / -inf), NaN logits weighing 0. Two launches shaped by `vocab` alone (slices of 1024
// ids, then one merging workgroup); `ws` = logprob_workspace_bytes(vocab) bytes of device scratch, 8-byte aligned.
// Returns non-zero (message set) for a vocabulary the merge cannot hold; p outside [0, max_rows) writes nothing.
bool logprob_vocab_ok(int vocab);  // 1 .. 409 slices: what the merging workgroup holds in registers
size_t logprob_workspace_bytes(int vocab);
int launch_logprobs(const float* logits, int vocab, const int32_t* token, const int32_t* pos, int max_rows, void* ws,
                    float* chosen, int32_t* top_id, float* top_lp, hipStream_t st);
// The same two launches with a row dimension (the scored prompt pass): logits row r at logits + r * row_stride, its picked
// id targets[r], its record in log row row0 + r (rows outside [0, max_rows) write nothing). A target outside [0, vocab)
// gives chosen = NaN, the top 20 are written all the same. ws = rows * logprob_workspace_bytes(vocab); rows <= 65535.
int launch_logprob_rows(const float* logits, size_t row_stride, int vocab, int rows, const int32_t* targets, int row0,
                        int max_rows, void* ws, float* chosen, int32_t* top_id, float* top_lp, hipStream_t st);

// ---- woq_score.hip: log-probabilities of a supplied token sequence over the prompt pass's rows ---------------------
constexpr int SCORE_BLOCK_ROWS = 256;  // rows whose logits the scratch holds at once
// null when the scored head takes this shape, else the "QBits: ..." reason
const char* score_shape_problem(const void* W, int w_dtype, int hidden, int vocab);
// scratch of launch_score_rows: the hi + lo activation rows, the logits of one block of 256 rows (256 x vocab x 4
// bytes) and the record's partials for those rows
size_t score_workspace_bytes(int hidden, int vocab);
// rows r = 0 .. M-1 of fp32 `hidden_rows` [M][hidden]: final RMSNorm (norm_w, eps), logits over the dense fp16 / bf16
// W [vocab][hidden] on the matrix cores (activation as hi + lo in W's type, fp32 accumulation), then the record of
// launch_logprob_rows with targets[r] into log row row0 + r. In blocks of SCORE_BLOCK_ROWS rows: 4 launches a block.
int launch_score_rows(const float* hidden_rows, const float* norm_w, float eps, const void* W, int w_dtype, int hidden,
                      int vocab, const int32_t* targets, int M, int row0, int max_rows, void* ws, float* chosen,
                      int32_t* top_id, float* top_lp, hipStream_t st);

// ---- woq_prefill.hip: the prompt pass's launches outside its GEMMs -------------------------------------------------
void launch_embed_rows(const void* embed, int dtype, const int32_t* tokens, int M, int hidden, float* out,
                       hipStream_t st);
// q_norm / k_norm (fp32 [HD], both or neither; eps): RMSNorm of every q / k head over HD before the rotation
int launch_rope_append(_Float16* qkv, int n_seq, int T, int start, int heads, int kv_heads, int HD, const float* cs,
                       const float* sn, void* kcache, void* vcache, int kv_dtype, size_t seq_stride_elems,
                       hipStream_t st, const float* q_norm = nullptr, const float* k_norm = nullptr, float qk_eps = 0.f);
int launch_attn_prefill(const _Float16* qkv, int n_seq, int T, int start, int heads, int kv_heads, int HD,
                        const void* kcache, const void* vcache, int kv_dtype, size_t seq_stride_elems, _Float16* out,
                        int window, hipStream_t st);
// last row of every sequence -> dst fp32 [n_seq][hidden]
void launch_gather_last(const float* h, int n_seq, int T, int hidden, float* dst, hipStream_t st);

// ---- woq_lora.hip: unmerged LoRA adapters beside the packed projections -------------------------------------------
// One fused projection's adapter as the kernels read it from device memory: its parts in blob column order (q | k | v
// concatenated; gate / up with `interleave`: 16-column tiles alternate gate, up as runtime.fuse_gate_up lays them out;
// one part for o_proj and down_proj). Part p: A [r][K] and B [n][r] fp32, both dense, s = lora_alpha / r; r == 0 = the
// part carries no adapter. The stacked rows of all parts' A (at most LORA_MAX_ROWS) index the shrink's output columns.
constexpr int LORA_MAX_PARTS = 3, LORA_MAX_RANK = 64, LORA_MAX_ROWS = LORA_MAX_PARTS * LORA_MAX_RANK;
constexpr int LORA_DELTA_MAX_LDS = 160 * 1024;  // the delta launch stages its K input values in LDS
struct LoraPart { const float* A; const float* B; int32_t r, n; float s; int32_t reserved; };
struct LoraDesc { LoraPart part[LORA_MAX_PARTS]; int32_t n_parts, interleave; };
const char* lora_desc_problem(const LoraDesc& host_copy, int N);  // null, or the "QBits: ..." reason
// decode: out[n] (fp32 [N], blob column order) = base_bias[n] (nullable = 0) + s_p * sum_j B_p[n'][j] * t_p[j],
// t_p[j] = inv * sum_k A_p[j][k] * x[k]. XQ form: x = the decoded XQ vector, inv = 1 / sqrt(sum(ssq_in) / K + eps) when
// ssq_in (K / 16 partial sums of squares) is given, else 1. fp32 form: x = x[k] * norm_w[k] and inv from the kernel's own
// sum of squares of x when norm_w is given, else x as it stands and inv = 1. One launch whose geometry depends on K and N
// alone; columns of a part with r == 0 receive base_bias bit for bit. K % 16 == 0, K <= 40000.
int launch_lora_delta_xq(const LoraDesc* desc_dev, const XqPtrs& xin, const float* ssq_in, float eps, int K, int N,
                         const float* base_bias, float* out, hipStream_t st);
int launch_lora_delta_f32(const LoraDesc* desc_dev, const float* x, const float* norm_w, float eps, int K, int N,
                          const float* base_bias, float* out, hipStream_t st);
// prompt pass, shrink: T[m][j] (fp32 [M][ldt], j over the r_tot stacked rows) = inv_m * sum_k A[j][k] * g_k * X[m][k]; X
// fp32 [M][ldx] with norm_w (g = norm_w, inv_m = the row's RMSNorm factor) or without, or fp16 without. r_tot = the sum
// of the parts' ranks (the host's copy: it shapes the grid). K % 16 == 0, ldx % 4 == 0.
int launch_lora_shrink(const LoraDesc* desc_dev, int r_tot, const void* X, int x_dtype, int ldx, int M, int K,
                       const float* norm_w, float eps, float* T, int ldt, hipStream_t st);
// prompt pass, expand: D[m][n] = s_p * sum_j T[m][roff_p + j] * B_p[n'][j] over the N blob columns, stored as
//   ADD_F32  out fp32 [M][ldo] += D          ADD_F16  out fp16 [M][ldo] = fp16(out + D)
//   SILU     (gate / up, interleave) out fp16 [M][ldo] (N / 2 columns) = SiLU(gu_gate + D_gate) * (gu_up + D_up) in fp32,
//            gu = the base GEMM's fp16 [M][ld_gu] gate/up rows in blob column order
enum LoraExpandMode { LORA_EXPAND_ADD_F32 = 0, LORA_EXPAND_ADD_F16 = 1, LORA_EXPAND_SILU = 2 };
int launch_lora_expand(const LoraDesc* desc_dev, const float* T, int ldt, int M, int N, int mode, void* out, int ldo,
                       const _Float16* gu, int ld_gu, hipStream_t st);

// ---- woq_gemm_f16.hip: the prompt pass's MFMA GEMM ----------------------------------------------------------------
// workspace bytes of one blob's [M, K] x [K, N] call, fragment image of the float weight types included (4-8x the
// blob: what made table-type prompt passes allocate per call while the engine's workspace sat unused — ADVICE r04);
// fp8: the call passes an fp8 low plane (`h` = the HI plane's header, which does not say so)
size_t gemm_f16_workspace_bytes_blob(int M, const woq_blob_header& h, int planes, bool fp8);
// out[M,N] = act[M,K] . W_deq (+ bias) with fp16 operands. `ws` = caller workspace of gemm_f16_workspace_bytes_blob
// (`ws_bytes`: its size, which the fragment image of the float weight types is checked against) or
// null (stream-ordered allocation per call, like the reference's per-call amalloc,
// bestla_weightonly_dispatcher.cpp:108-118,179). norm_w/eps: RMSNorm fused into the pack pass (null = none);
// residual / epi: see GemmF16Args; fp32_class: the three-product hi + lo form (compute_dtype fp32).
int launch_gemm_f16(const void* act, int act_dtype, int lda, const void* blob, const woq_blob_header& h,
                    const float* bias, void* out, int out_dtype, int ldo, int M, const float* norm_w, float eps,
                    const float* residual, int ld_res, int epi, void* ws, int fp32_class, hipStream_t st,
                    const void* fp8_lo = nullptr, uint32_t fp8_type = 0, size_t ws_bytes = 0);
// events recorded on the launch stream right before / after the GEMM kernel of the next launch_gemm_f16 calls
// (null = off): lets bench.py time the dominant prefill kernel without its pack pass
void set_gemm_time_events(hipEvent_t before, hipEvent_t after);
}  // namespace woq

// ---- woq_comm.hip: device-side tensor-parallel exchange, the engine's internals -----------------------------------
size_t woq_comm_max_elems(woq_comm* c);  // floats one all-reduce launch can carry (the inbox size)
int woq_comm_launch_allreduce(woq_comm* c, float* buf, size_t n, hipStream_t st);
// the engine's form: `pushed` = the producing GEMV already stored this rank's contribution into the peers' inboxes
// (woq_comm_dev_ptr), `xo` (optional) = the summed vector also as an XQ vector (times norm_w, sums of squares in ssq_out)
int woq_comm_launch_allreduce_ex(woq_comm* c, float* buf, size_t n, int pushed, const float* norm_w,
                                 const woq::XqPtrs& xo, float* ssq_out, hipStream_t st);
// device-resident copy of the communicator record (peer inboxes, sequence word, rank / world), valid once connected
const woq::CommDev* woq_comm_dev_ptr(woq_comm* c);
// `status` (nullable) = the engine's status word: |= 4 when no pair won on any rank (token 0), like launch_argmax_pairs
int woq_comm_launch_greedy(woq_comm* c, const float* pmax, const int32_t* pidx, int n, int vocab_offset,
                           int32_t* token, int32_t* pos, int32_t* log, int* status, hipStream_t st);
