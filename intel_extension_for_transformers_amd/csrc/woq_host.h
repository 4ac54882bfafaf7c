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

// ---- woq_h2o.hip: H2O heavy-hitter eviction — score, select, compact ------------------------------------------------
// Device scratch of launch_h2o_score_decode: arrival counters (zero before the first launch; every launch leaves them
// zero), the slices' per-head (max, sum) and the logits of one layer.
size_t h2o_decode_scratch_bytes(int kv_heads, int max_ctx);
void launch_h2o_zero(void* p, size_t bytes, hipStream_t st);  // bytes (a multiple of 4) of zeros, a kernel: capturable
// One layer of a decode step, after its K row was appended at *pos: score[kvh][p] (fp32 [kv_heads][max_ctx]) += the
// probability row p <= *pos received from the kv group's query heads. q from the step's fp32 un-rotated qkv: q-norm
// (nullable weights) and RoPE at *pos as the decode attention does them. One launch whose grid depends on max_ctx alone.
int launch_h2o_score_decode(const float* qkv, const void* kcache, int kv_dtype, int heads, int kv_heads, int D, int max_ctx,
                            const int32_t* pos, const float* cs, const float* sn, const float* q_norm, float eps,
                            float* score, void* scratch, hipStream_t st);
// One layer of a prompt chunk of one sequence, after launch_rope_append: score += the column sums of the chunk's causal
// attention over cache rows [0, start + T). lse: fp32 [heads][T] scratch. Two launches.
int launch_h2o_score_prompt(const _Float16* qkv, int T, int start, int heads, int kv_heads, int D, const void* kcache,
                            int kv_dtype, int max_ctx, float* lse, float* score, hipStream_t st);
// dst[l][kvh][p] (int32 [layers][kv_heads][max_ctx], p < n_cached) = the row p moves to, -1 for the n_discard rows with the
// lowest score among [n_keep, n_cached - recent) (ties: the lower row goes)
int launch_h2o_select(const float* score, int32_t* dst, int layers, int kv_heads, int max_ctx, int n_keep, int n_discard,
                      int recent, int n_cached, hipStream_t st);
// the gather along dst, in place: V and score rows (nullable) copied, K rows rotated back by table row p - dst[p]; score
// rows [n_cached - n_discard, n_cached) are zeroed. One launch.
int launch_h2o_compact(void* kseq, void* vseq, float* score, const int32_t* dst, int kv_dtype, int layers, int kv_heads,
                       int D, int max_ctx, const float* cs, const float* sn, int n_keep, int n_discard, int n_cached,
                       hipStream_t st);

// ---- woq_moe.hip, woq_moe_prompt.hip: the routed expert block of a sparse mixture-of-experts layer, in two forms -------
// MOE_GROUPED (woq_moe.hip): few rows per expert, table blocks of 16 rows, on the int8 / fp8 MFMA: decode and short
// prompts. MOE_PROMPT (woq_moe_prompt.hip): many rows per expert, blocks of 128 rows, on the fp16 MFMA.
enum MoeForm { MOE_GROUPED = 0, MOE_PROMPT = 1 };
constexpr int MOE_BLOCK_ROWS = 16;      // rows of one block of the grouped plan's table: four MFMA row sets of four tokens
constexpr int MOE_PROMPT_ROWS = 128;    // rows of one block of the prompt plan's table: the row tile of its product
constexpr int MOE_MAX_EXPERTS = 1024;   // the plans' histograms live in LDS
constexpr int MOE_MAX_SLOTS = 8192;     // routed slots T * top_k of one grouped call: the plan keeps their ids in LDS
constexpr int MOE_PLAN_SEG = 1024;      // slots of one segment of the prompt plan = threads of a plan workgroup
constexpr int MOE_PROMPT_MAX_SLOTS = 65536;   // routed slots of one prompt call: 64 plan segments
constexpr int moe_max_slots(MoeForm form) { return form == MOE_PROMPT ? MOE_PROMPT_MAX_SLOTS : MOE_MAX_SLOTS; }
// rows of the module's `prompt_min_tokens`: from this many rows the engine's prompt pass takes the prompt form
constexpr int MOE_PROMPT_MIN_ROWS = 64;
// One call (include/woq_hip.h woq_moe_forward / woq_moe_prompt_forward, which check all of it): E blobs of each kind at
// a uniform stride under one header, the routing on the device, `workspace` of moe_workspace_bytes(form, ..) bytes.
struct MoeCall {
  const void* x; int x_dtype, ldx;
  const void* topk_idx; bool idx_is_int64; const float* topk_w;
  int T, top_k, E;
  const void* gate_up_blobs; const woq_blob_header* gate_up_hdr; size_t gate_up_stride;
  const void* down_blobs; const woq_blob_header* down_hdr; size_t down_stride;
  void* out; int out_dtype, ldo;
  void* workspace;
  // the engine's two variations (both off in the public entry points, whose launches and bytes stay as they were):
  // plan_ready: the plan tables already stand in `workspace` (woq_moe_route.hip's decode form wrote them), no plan launch;
  // residual: the last launch is launch_moe_combine_residual onto these rows instead of launch_moe_combine into `out`
  bool plan_ready = false;
  const struct MoeResidual* residual = nullptr;
};
// null when the products take expert blobs under this header at this stride, else the "QBits: ..." reason.
// `int4_only` (the decode engine's sparse layer) also refuses the table types, the int8 composite and the fp8 types,
// which woq_moe_forward / woq_moe_prompt_forward take.
const char* moe_header_problem(const woq_blob_header& h, size_t stride, bool int4_only = true);
// What both forms' products read of an expert blob, resolved on the host. MOE_W_INT4 and MOE_W_TABLE (nf4 / fp4: the
// nibble is a table code, symmetric) have one nibble plane, [0]. MOE_W_INT8 is the composite of woq_int8_headers: the HI
// plane [0] and the LO plane [1], q8 - zp8 = 16 (hi - zhi) + (lo - zlo); off_scale = the LO plane's scales s, which both
// share; off_zp[1] always stands, off_zp[0] only under an asymmetric blob. An absent zero-point section is offset 0.
// MOE_W_FP8 (fp8_e4m3 / fp8_e5m2) is the composite of woq_fp8_headers: the same two planes holding the nibbles of the code
// byte (hi << 4) | (lo ^ 8), off_scale = the LO plane's scales, symmetric: no zero point is read.
enum MoeWeightKind { MOE_W_INT4 = 0, MOE_W_TABLE = 1, MOE_W_INT8 = 2, MOE_W_FP8 = 3 };
struct MoePlanes {
  MoeWeightKind kind;
  size_t off_q[2], off_scale, off_zp[2];
};
MoePlanes moe_blob_planes(const woq_blob_header& h);  // h has passed moe_header_problem
// a row of a plan's block table: `rows` sorted slots of one expert from sorted position `first`
struct MoeBlock { int32_t expert, first, rows, pad; };
// Where the sections of a form's workspace lie (byte offsets). The plan tables come first: blocks[0 .. *nblocks) cover
// the sorted positions [0, valid slots) without a gap, in order; max_blocks sizes the grids (a workgroup past *nblocks
// returns). counts (nseg segments of E words) is the prompt plan's own scratch, empty in the grouped form. Then the
// fp32 rows h [sorted slot][inter] and y [sorted slot][hidden].
struct MoeLayout {
  size_t sorted, pos_of, blocks, nblocks, counts, h, y, total;
  int max_blocks, nseg;
};
MoeLayout moe_layout(MoeForm form, int T, int top_k, int E, int hidden, int inter);
// MoeLayout::total, or 0 for a shape outside the form's limits: woq_moe_workspace / woq_moe_prompt_workspace
size_t moe_workspace_bytes(MoeForm form, int T, int top_k, int E, int hidden, int inter);
// the prompt form's plan tables alone, which the backward (woq_moe_bwd.hip) puts at the front of its workspace
size_t moe_prompt_plan_bytes(int T, int top_k, int E);
// the plan tables of a form's workspace, as pointers
struct MoeRoutePlan {
  int32_t* sorted; int32_t* pos_of; MoeBlock* blocks; int32_t* nblocks; int32_t* counts;
  int max_blocks, nseg;
};
MoeRoutePlan moe_plan_tables(MoeForm form, void* workspace, int T, int top_k, int E);
// the prompt form's plan over the S = T * top_k ids — count, scan, scatter: three launches
void launch_moe_prompt_plan(const void* topk_idx, bool idx_is_int64, int S, int E, const MoeRoutePlan& p, hipStream_t st);
// One product of a form over a plan. MOE_GATE_UP: out[sorted slot][I] = SiLU(g) * u of the rows m.x gathered by token;
// MOE_GATE_UP_RAW (the prompt form only, for the backward; fp8 blobs are refused): out[sorted slot][2 I] fp32 = [g | u],
// no SiLU; MOE_DOWN: out[sorted slot][H] = h[sorted slot][I] through the down blobs.
enum MoeRole { MOE_GATE_UP, MOE_GATE_UP_RAW, MOE_DOWN };
int launch_moe_prompt_product(MoeRole role, const MoeCall& m, const MoeRoutePlan& p, const float* h, float* out,
                              hipStream_t st);
// plan (one launch, or the prompt form's three; none under plan_ready), gate/up, down, combine: launches shaped by
// (T, top_k, E, hidden, inter) alone, no host synchronisation
int launch_moe_forward(const MoeCall& m, MoeForm form, hipStream_t st);
// out[t][n] = sum_j topk_w[t][j] * y[pos_of[t k + j]][n] (fp32 y [sorted slot][H]), j ascending, a dropped slot (-1)
// contributing zero, rounded once to out_dtype: the last launch of both forms
void launch_moe_combine(const float* y, const int32_t* pos_of, const float* topk_w, int T, int top_k, int H, void* out,
                        int out_dtype, int ldo, hipStream_t st);
// The checks woq_moe_forward, woq_moe_prompt_forward and woq_moe_backward share, over the call as they received it: the
// headers, the [K, N] relation, the dtypes, then — past a call of no rows — the limits, null pointers, leading
// dimensions, alignment and the workspace size. What differs between them: the names inside the messages, the limits
// (`workspace` returns 0 outside them) and the workspace's alignment.
struct MoeEntry {
  const char* fn;
  size_t (*workspace)(int T, int top_k, int E, int hidden, int inter);
  const char* workspace_fn;
  int max_slots;
  size_t workspace_align;
};
// 0: sound, go on | 1: refused, woq_last_error says why | -1: no rows, nothing to do
int moe_entry_checks(const MoeEntry& e, const MoeCall& m, size_t workspace_bytes);

// ---- woq_moe_bwd.hip: backward of the routed expert block with respect to its rows and its routing weights ---------
// rows of one call: what woq_moe_backward takes (the plan's limit)
constexpr int MOE_BACKWARD_MAX_SLOTS = MOE_PROMPT_MAX_SLOTS;

// ---- woq_moe_route.hip: the router of a sparse layer -----------------------------------------------------------------
// include/woq_hip_experimental.h woq_moe_route, which this is: checks (a "QBits:" message, nothing launched), then
// one launch — the decode form for T == 1 (scratch: woq_moe_route_scratch_bytes, its ticket word zero), the MFMA
// form otherwise. plan (T == 1, all four tables or none): the row's routing as woq_moe.hip's plan kernel would write it
// from idx — sorted[top_k], pos_of[top_k], blocks[top_k] and their count — so that the grouped products can follow
// without a plan launch
int launch_moe_route(const float* x, int ldx, const float* norm_w, float eps, const void* router_w, int router_dtype,
                     int T, int H, int E, int top_k, int renorm, float* xn, int32_t* idx, float* w, void* scratch,
                     const MoeRoutePlan& plan, hipStream_t st);
// The combine of a sparse layer inside the engine, onto the fp32 residual stream:
//   hidden[t][n] += sum_j w[t][j] * y[pos_of[t k + j]][n], j ascending, a dropped slot contributing zero.
// xo (one row only, H % 16 == 0): the new row also leaves as the next layer's XQ input, times next_norm_w, with the
// per-block sums of squares of the raw values in ssq_out — what the dense layer's down_proj epilogue emits
struct MoeResidual { float* hidden; int ldh; XqPtrs xo; const float* next_norm_w; float* ssq_out; };
int launch_moe_combine_residual(const float* y, const int32_t* pos_of, const float* topk_w, int T, int top_k, int H,
                                const MoeResidual& r, hipStream_t st);

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
