// woq_engine.hip — native batch-1 decode engine for a Llama-class decoder over WQH1 blobs.
//
// What it replaces: in the reference a decode step is HF's LlamaDecoderLayer.forward running stock
// PyTorch CPU ops, with every nn.Linear swapped for QuantizedLinearQBits.forward
// (transformers/llm/quantization/nn/modules.py:140-169) -> matmul_kbit -> qbits.woq_linear: 7 Python ->
// pybind crossings per layer with the GIL held, a fresh torch.zeros output and a .float() up-cast
// per call. Here one token step is 5 kernel launches per layer issued from C++
// with no allocation and no host round trip, and the whole step is replayed as one hipGraph:
//     [RMSNorm + qkv GEMV] -> [RoPE + KV append + attention] -> [o GEMV + residual]
//  -> [RMSNorm + gate/up GEMV + SiLU*mul] -> [down GEMV + residual]
// The fused-op boundary mirrors ipex.optimize_transformers, the reference's own precedent for
// swapping HF's norm/rope/MLP for device kernels after from_pretrained (docs/weightonlyquant.md:199-202).
// Residual stream and the GEMV I/O stay fp32 (the reference up-casts every activation to fp32 at the
// qbits boundary, modules.py:152-154); the KV cache is fp16/bf16.
#include <algorithm>
#include <tuple>
#include <vector>

#include "woq_device.h"
#include "woq_host.h"
#include "../../include/woq_hip_experimental.h"

using woq::XqPtrs;

// a layer's four projections in launch order, and the epilogue each runs with (1 = SiLU(gate) * up)
enum Proj { P_QKV, P_O, P_GATE_UP, P_DOWN, P_COUNT };
constexpr int kProjEpi[P_COUNT] = {0, 0, 1, 0};
// the engine's own form of woq_layer_weights (woq_engine_set_layer converts). fp8-weight layers: blob / hdr are the HI
// nibble plane's (include/woq_blob.h woq_fp8_headers) and fp8_lo the LO plane's tile data; null for integer / table layers
struct EngineProj { const void* blob; woq_blob_header hdr; const void* fp8_lo; };
// what woq_engine_set_layer last committed for a layer: nothing yet, integer / 4-bit table blobs, fp8-weight blobs. A step
// needs every layer set and all of one kind (engine_layers_problem)
enum LayerKind { LAYER_UNSET, LAYER_INT, LAYER_FP8 };
// qkv_bias / q_norm / k_norm: the optional extras of woq_engine_set_layer_extras (null = absent)
struct EngineLayer {
  EngineProj p[P_COUNT];
  const float* ln1;
  const float* ln2;
  LayerKind kind = LAYER_UNSET;
  const float* qkv_bias = nullptr;
  const float* q_norm = nullptr;
  const float* k_norm = nullptr;
};
// the pick after an lm_head (woq_engine::tail decides, engine_tail issues); pairs: that lm_head emits (max, index) pairs
enum TailPick { PICK_NONE, PICK_SAMPLED, PICK_ARGMAX_FULL, PICK_ARGMAX_PAIRS, PICK_ARGMAX_EMBED, PICK_TP_GREEDY };
struct Tail { TailPick pick; bool pairs; };
// (sampler, controls, guide, logprobs): what a captured graph holds of the tail; a setter that changes it drops the graphs
using TailKey = std::tuple<bool, bool, bool, bool>;

struct woq_engine {
  woq_engine_config cfg;
  std::vector<EngineLayer> layers;
  const void* embed = nullptr;
  int embed_dtype = WOQ_F16;
  const float* final_norm = nullptr;
  const void* lm_head = nullptr;
  int lm_dtype = WOQ_F16;
  const float* cs = nullptr;
  const float* sn = nullptr;
  float* hidden = nullptr;
  float* qkv = nullptr;
  float* attn = nullptr;
  float* act = nullptr;
  float* logits = nullptr;
  int32_t* token = nullptr;
  int32_t* pos = nullptr;
  // positions a rolling KV cache has dropped in the running request (woq_engine_kv_shift; 0 otherwise): the sampled
  // tail's Philox counter is pos + discarded
  int32_t* discarded = nullptr;
  uint8_t* kcache = nullptr;
  uint8_t* vcache = nullptr;
  size_t kv_layer_bytes = 0;
  uint8_t* k_of(int l) const { return kcache + (size_t)l * kv_layer_bytes; }  // layer l's K / V cache (sequence 0)
  uint8_t* v_of(int l) const { return vcache + (size_t)l * kv_layer_bytes; }
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  // the same step captured `graph_unroll` times in a row (the token / position chain lives on the device, so k steps are
  // one valid graph): a burst of n replays launches n / k of these and n % k single steps. Each hipGraphLaunch costs the
  // device a few us between tokens (eager bursts read +0.6 % over one-step replays, profiles/r05z_*); 8 steps per launch
  // amortise it.
  hipGraph_t graph_k = nullptr;
  hipGraphExec_t exec_k = nullptr;
  static constexpr int graph_unroll = 8;
  woq_allreduce_fn allreduce = nullptr;
  void* allreduce_user = nullptr;
  // XQ decode path (woq_xq.h): activations travel between the step's kernels as limb blocks written by the
  // producing epilogue; on when every layer's blobs qualify (woq_engine_set_layer) and WOQ_ENGINE_XQ != 0
  bool xq_shapes_ok = true, xq_enabled = true;
  XqPtrs xq_hidden = {nullptr, nullptr, nullptr}, xq_attn = {nullptr, nullptr, nullptr},
         xq_act = {nullptr, nullptr, nullptr};
  float* ssq_part = nullptr;  // [hidden / 16] partial sums of squares of the residual stream
  // fused qkv + attention launch (woq_gemv_attn.hip): {tag, fp32} granules of q | k | v, the step counter the tags are
  // made of (advanced by the embedding kernel, the first of every step) and the sticky give-up flag
  unsigned long long* qkv_g = nullptr;
  unsigned int* step_seq = nullptr;
  int* fuse_status = nullptr;
  // fp8-weight layers (round 6; bestla_weightonly_dispatcher.hpp:62-72; EngineProj). Such engines run the
  // fp32-activation step (no XQ vectors): fp8 matrix-core GEMVs with RMSNorm / residual fused, 6 launches a layer
  uint32_t fp8_type = 0;  // 0 = integer / table layers; WOQ_W_FP8_E4M3 | WOQ_W_FP8_E5M2
  float* gu_tmp = nullptr;  // fp32 [2 * inter]: the fused gate/up projection's columns before SiLU * mul
  unsigned long long* attn_part_g = nullptr;  // the slices' partials as {tag, fp32} granules [heads][64][head_dim + 2]
  // tensor parallel ranks take the XQ path when the exchange runs on the device (its all-reduce kernel then emits the
  // next XQ vector itself); with a host-side transport they keep the fp32-activation kernels
  bool tp_xq = true, tp_fused_push = true;
  bool use_xq() const {
    return xq_shapes_ok && xq_hidden.limbs != nullptr &&
           (cfg.tp_size <= 1 ? xq_enabled : (tp_xq && comm != nullptr && allreduce == nullptr));
  }
  const woq::CommDev* tp_push() const;  // where the row-parallel GEMVs push their partial sums (null = nowhere)
  // residual input of a row-parallel projection (o_proj / down_proj) that adds onto `stream`: rank 0 carries the
  // residual so that the sum over ranks adds it exactly once
  const float* tp_residual(const float* stream) const { return cfg.tp_size <= 1 || cfg.tp_rank == 0 ? stream : nullptr; }
  woq_comm* comm = nullptr;  // device-side exchange: all-reduce kernels inside the (capturable) decode step
  int vocab_offset = 0;      // first vocabulary row of this rank's lm_head shard
  std::vector<void*> owned;  // everything hipMalloc'ed by create()
  // prompt pass: [n_seq * T] rows at a time; buffers grow on demand (never inside a captured graph)
  int32_t* tok_log = nullptr;   // [max_ctx + 1]: tok_log[p] = greedy token produced by the step that fed position p
  float* am_val = nullptr;      // per-workgroup (max logit, index) pairs of the lm_head launch, for the greedy argmax
  int32_t* am_idx = nullptr;
  int window = 0;               // sliding-window attention (HF Mistral sliding_window), 0 = full causal
  // decode attention: what is asked for (slices, grouped form, merge and fusion switches; woq_host.h AttnOptions). fold =
  // WOQ_ATTN_FOLD=1: built, parity-tested and measured SLOWER than the combine launch (+3..5 us per layer: three
  // dependent device-scope round trips on the launch's tail, profiles/r04d_*); opt-in, default off. fuse_sliced /
  // grouped_a2a = WOQ_FUSE_SLICED / WOQ_GROUPED_A2A (0: sliced contexts keep the separate launches / the combine launch)
  woq::AttnOptions attn_opt;
  // how layer l's attention runs under `o` (plan_attn_decode): decided per call, host arithmetic only
  woq::AttnDecodePlan attn_plan(int l, const woq::AttnOptions& o) const;
  woq::AttnDecodeIO attn_io(int l, const XqPtrs& xo) const;
  float* attn_part = nullptr;   // fp32 partials of the sliced decode attention (layout: woq_attn_merge.h)
  unsigned int* attn_cnt = nullptr;  // [heads] arrival counters of the slices' last-workgroup merge, zero between launches
  bool time_eager = true;       // woq_engine_time_gemv / _twin: passes issued eagerly (how bursts run by default) or as a
                                // replayed graph (round 3's measure; woq_engine_set_time_eager(e, 0))
  int max_batch = 1;
  size_t pf_rows = 0, pf_ws_bytes = 0;
  float* pf_h = nullptr;        // fp32 residual stream [rows][hidden]
  _Float16* pf_qkv = nullptr;   // fp16 [rows][(heads + 2 kv_heads) * head_dim]
  _Float16* pf_attn = nullptr;  // fp16 [rows][heads * head_dim]
  _Float16* pf_act = nullptr;   // fp16 [rows][inter]
  void* pf_ws = nullptr;        // GEMM pack workspace
  float* pf_last = nullptr;     // fp32 [max_batch][hidden]
  float* pf_logits = nullptr;   // fp32 [max_batch][vocab]
  // sampled token tail (woq_sample.hip): with `sampler_on` a chaining step picks its token with launch_sample_tail instead
  // of the argmax launches. The parameters live in `samp_cfg` (device), the repetition penalty's history in `samp_seen`
  bool sampler_on = false;
  woq_sampler_config* samp_cfg = nullptr;
  uint32_t* samp_seen = nullptr;  // [(vocab + 31) / 32]
  int seen_words() const { return (cfg.vocab + 31) / 32; }
  // sampler controls (logit bias, presence / frequency penalty, min_p): with `controls_on` the tail is the pre-pass +
  // the sampling launch over its scratch. Allocated by the first use, [vocab] each
  bool controls_on = false;
  woq_sampler_config samp_cfg_host = {};  // what samp_cfg holds (the controls' checks read do_sample)
  woq_sampler_controls samp_ctl_host = {};  // what samp_ctl holds (set_sampler re-checks min_p against do_sample)
  woq_sampler_controls* samp_ctl = nullptr;
  float* samp_bias = nullptr;      // dense, NaN = no entry
  uint32_t* samp_count = nullptr;  // times each id was generated in this request
  float* samp_adj = nullptr;       // the pre-pass's scores
  int32_t* samp_bias_ids = nullptr;  // [1024] + [1024] staging of the (id, value) pairs
  float* samp_bias_vals = nullptr;
  // token guide (woq_sample.hip): with `guide_on` the tail is the guided pre-pass + the sampling launch + the state's
  // advance. It runs over the controls' memory whether or not controls are installed (neutral values then). The table
  // is the engine's own copy, grown on demand and kept; `guide` (device) names it and holds the state
  bool guide_on = false;
  woq::GuideState* guide = nullptr;
  woq::GuideState guide_host = {};  // what `guide` holds, bar the state the steps move
  uint16_t* guide_table = nullptr;
  size_t guide_cap = 0;  // bytes
  // log-probability record (woq_logprob.hip): with `logprobs_on` every chaining step writes row pos - 1 of three logs,
  // [max_ctx + 1] rows each like tok_log, after its pick. Allocated by the first woq_engine_set_logprobs(e, 1)
  bool logprobs_on = false;
  float* lp_chosen = nullptr;   // [max_ctx + 1]
  int32_t* lp_top_id = nullptr; // [max_ctx + 1][20]
  float* lp_top_lp = nullptr;   // [max_ctx + 1][20]
  void* lp_ws = nullptr;        // the slices' partial results
  // scored prompt pass (woq_score.hip): hi + lo rows, the logits of one block of 256 rows and their partials;
  // allocated by the first woq_engine_prefill_scored and held, like pf_ws
  void* score_ws = nullptr;
  // unmerged LoRA adapters (woq_lora.hip; woq_engine_lora_reserve / woq_engine_set_lora). Per layer and projection kind
  // one device descriptor (parts, ranks, scalings: what the kernels read) with its host mirror; per (layer, target) an A
  // and a B table at rank lora_rmax, which installed values are copied into; one delta buffer per projection kind, which
  // the decode step's GEMV takes as its bias. A (layer, kind) is active while one of its parts has a rank above 0: only
  // then does a step hold its delta launch, so a change of that set drops captured graphs, other values do not
  int lora_rmax = 0;  // 0 = not reserved
  struct LoraTable { float* A; float* B; };
  std::vector<LoraTable> lora_tab;         // [layers][LORA_TARGETS]
  std::vector<woq::LoraDesc> lora_host;    // [layers][P_COUNT], what lora_desc holds
  woq::LoraDesc* lora_desc = nullptr;      // device, [layers][P_COUNT]
  float* lora_delta[P_COUNT] = {nullptr, nullptr, nullptr, nullptr};  // fp32 [qkv_n], [hidden], [2 * inter], [hidden]
  float* pf_t = nullptr;                   // prompt pass: fp32 [rows][LORA_MAX_PARTS * lora_rmax], the shrink's output
  _Float16* pf_gu = nullptr;               // fp16 [rows][2 * inter]: gate/up before SiLU * mul, when gate or up is targeted
  size_t pf_t_rows = 0, pf_gu_rows = 0;
  int lora_ldt() const { return woq::LORA_MAX_PARTS * lora_rmax; }
  int lora_rows(int l, int k) const {  // stacked rows of (layer, kind); 0 = no adapter there
    if (lora_rmax == 0) return 0;
    const woq::LoraDesc& d = lora_host[(size_t)l * P_COUNT + k];
    int r = 0;
    for (int p = 0; p < d.n_parts; ++p) r += d.part[p].r;
    return r;
  }
  const woq::LoraDesc* lora_dev(int l, int k) const { return lora_desc + (size_t)l * P_COUNT + k; }
  int lora_active_count() const {
    int n = 0;
    for (int l = 0; lora_rmax > 0 && l < cfg.layers; ++l)
      for (int k = 0; k < P_COUNT; ++k) n += lora_rows(l, k) > 0 ? 1 : 0;
    return n;
  }
  // the token tail, decided here alone: the pick after the lm_head of a step (after_prompt: of a prompt pass)
  Tail tail(bool greedy, bool fuse_next, bool after_prompt) const;
  woq::SampleTail sample_tail() const;  // the buffers of a sampled pick
  TailKey tail_key() const { return TailKey{sampler_on, controls_on, guide_on, logprobs_on}; }
  // the sampler, the guide, the record and a scored prompt read every logit: a tensor-parallel head is vocab-sharded
  bool whole_vocab() const { return cfg.tp_size <= 1 && comm == nullptr && allreduce == nullptr; }
};

using namespace woq;

AttnDecodePlan woq_engine::attn_plan(int l, const AttnOptions& o) const {
  const bool xq = use_xq();
  // the one device-derived number (asked once per shape, then remembered): only the grouped form's all-to-all merge reads it
  const int slots = xq && o.grouped && o.grouped_a2a ? attn_decode_mfma_slots(cfg.kv_dtype, cfg.heads / cfg.kv_heads) : 0;
  return plan_attn_decode(AttnShape{cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.kv_dtype, cfg.max_ctx, window}, o,
                          AttnFacts{xq, qkv_g != nullptr && attn_part_g != nullptr, cfg.layers, &layers[l].p[P_QKV].hdr, slots,
                                    layers[l].q_norm != nullptr});
}

AttnDecodeIO woq_engine::attn_io(int l, const XqPtrs& xo) const {
  return AttnDecodeIO{qkv, k_of(l), v_of(l), pos, cs, sn, attn, xo, attn_part, attn_cnt, attn_part_g, step_seq, l, fuse_status,
                      layers[l].q_norm, layers[l].k_norm, cfg.rms_eps};
}

const woq::CommDev* woq_engine::tp_push() const {
  return cfg.tp_size > 1 && comm != nullptr && tp_fused_push ? woq_comm_dev_ptr(comm) : nullptr;
}

static const XqPtrs kNoXq = {nullptr, nullptr, nullptr};

// Why the engine's layers cannot be launched over (null = they can): every entry point that launches a layer's kernels
// asks before its first launch. An unset layer holds null blobs; fp8 and integer layers take different kernels off one
// engine-wide switch (fp8_type), so a mix would hand one kind's blob to the other's kernel.
static const char* engine_layers_problem(const woq_engine* e) {
  for (const EngineLayer& w : e->layers) {
    if (w.kind == LAYER_UNSET) return "QBits: engine layer not set (woq_engine_set_layer comes first, for every layer)";
    // (woq_engine_set_layer never commits a mix: this line guards the kernels' precondition where they are launched)
    if (w.kind != e->layers[0].kind) return "QBits: fp8 and integer layers cannot be mixed in one engine";
  }
  return nullptr;
}
#define WOQ_CHECK_LAYERS(e)                                                \
  do {                                                                     \
    if (const char* why = engine_layers_problem(e)) return woq::fail(why); \
  } while (0)

// the static per-column bias of projection k (Qwen2's q | k | v biases), null = none
static const float* engine_static_bias(const woq_engine* e, int l, Proj k) {
  return k == P_QKV ? e->layers[l].qkv_bias : nullptr;
}

// projection k of layer l as one batch-1 GEMV over an XQ vector, adapter-less (what the timing hooks launch)
static int engine_gemv_xq_base(woq_engine* e, int l, Proj k, const XqPtrs& xin, float* out, const float* ssq_in,
                               const float* residual, const XqPtrs& xo, const float* next_norm_w, float* ssq_out,
                               hipStream_t st, const CommDev* tp = nullptr) {
  const EngineProj& p = e->layers[l].p[k];
  return launch_gemv_xq(xin, p.blob, p.hdr, engine_static_bias(e, l, k), out, ssq_in, e->cfg.rms_eps, residual,
                        kProjEpi[k], xo, next_norm_w, ssq_out, st, tp);
}

// The `bias` the decode GEMV of (l, k) takes. No adapter there: the static bias, and nothing is launched. With one: the
// delta launch over the projection's own input (woq_lora.hip) writes static bias + s * B . (inv * A . x) into the kind's
// buffer, which every GEMV form adds after the RMSNorm factor. Exactly one of xin.limbs / x32 is given.
static int engine_lora_bias(woq_engine* e, int l, Proj k, const XqPtrs& xin, const float* ssq_in, const float* x32,
                            const float* norm_w, hipStream_t st, const float** bias) {
  *bias = engine_static_bias(e, l, k);
  if (e->lora_rows(l, k) == 0) return 0;
  const woq_blob_header& h = e->layers[l].p[k].hdr;
  const int rc = x32 == nullptr ? launch_lora_delta_xq(e->lora_dev(l, k), xin, ssq_in, e->cfg.rms_eps, h.K, h.N, *bias,
                                                       e->lora_delta[k], st)
                                : launch_lora_delta_f32(e->lora_dev(l, k), x32, norm_w, e->cfg.rms_eps, h.K, h.N, *bias,
                                                        e->lora_delta[k], st);
  *bias = e->lora_delta[k];
  return rc;
}

// projection k of layer l as one batch-1 GEMV over an XQ vector (behind its adapter's delta launch, if it has one)
static int engine_gemv_xq(woq_engine* e, int l, Proj k, const XqPtrs& xin, float* out, const float* ssq_in,
                          const float* residual, const XqPtrs& xo, const float* next_norm_w, float* ssq_out,
                          hipStream_t st, const CommDev* tp = nullptr) {
  if (e->lora_rows(l, k) == 0)
    return engine_gemv_xq_base(e, l, k, xin, out, ssq_in, residual, xo, next_norm_w, ssq_out, st, tp);
  const float* bias = nullptr;
  if (const int rc = engine_lora_bias(e, l, k, xin, ssq_in, nullptr, nullptr, st, &bias)) return rc;
  const EngineProj& p = e->layers[l].p[k];
  return launch_gemv_xq(xin, p.blob, p.hdr, bias, out, ssq_in, e->cfg.rms_eps, residual, kProjEpi[k], xo, next_norm_w,
                        ssq_out, st, tp);
}

// The row-parallel projection that ends a sub-block (o_proj / down_proj), XQ path. One GPU: hidden += x . W, and the new
// hidden leaves as the next GEMV's XQ input. Tensor parallel: hidden = this rank's partial sum (tp_residual), pushed
// into the peers' inboxes from the epilogue; the all-reduce that follows emits the XQ vector.
static int engine_row_parallel_xq(woq_engine* e, int l, Proj k, const XqPtrs& xin, const XqPtrs& xo,
                                  const float* next_norm_w, float* ssq_out, hipStream_t st) {
  if (e->cfg.tp_size <= 1)
    return engine_gemv_xq(e, l, k, xin, e->hidden, nullptr, e->hidden, xo, next_norm_w, ssq_out, st);
  return engine_gemv_xq(e, l, k, xin, e->hidden, nullptr, e->tp_residual(e->hidden), kNoXq, nullptr, nullptr, st,
                        e->tp_push());
}

// XQ form of the two sub-blocks: the same five launches, activations handed over as limb blocks
static int engine_attn_block_xq(woq_engine* e, int l, hipStream_t st) {
  const woq_engine_config& c = e->cfg;
  const EngineLayer& w = e->layers[l];
  int rc = 0;
  const AttnDecodePlan plan = e->attn_plan(l, e->attn_opt);
  const AttnDecodeIO io = e->attn_io(l, e->xq_attn);
  if (plan.form == ATTN_FUSED) {
    const float* bias = nullptr;
    if ((rc = engine_lora_bias(e, l, P_QKV, e->xq_hidden, e->ssq_part, nullptr, nullptr, st, &bias)) != 0) return rc;
    rc = launch_gemv_xq_attn(plan, io, e->xq_hidden, w.p[P_QKV].blob, w.p[P_QKV].hdr, e->qkv_g, e->ssq_part, c.rms_eps, st,
                             bias);
    if (rc) return rc;
  } else {
    rc = engine_gemv_xq(e, l, P_QKV, e->xq_hidden, e->qkv, e->ssq_part, nullptr, kNoXq, nullptr, nullptr, st);
    if (rc) return rc;
    rc = launch_attn_decode(plan, io, st);
    if (rc) return rc;
  }
  // hidden += attn . W_o ; the new hidden leaves as the MLP's XQ input (times ln2) with its sums of squares
  return engine_row_parallel_xq(e, l, P_O, e->xq_attn, e->xq_hidden, w.ln2, e->ssq_part, st);
}

static int engine_mlp_block_xq(woq_engine* e, int l, hipStream_t st) {
  const int rc = engine_gemv_xq(e, l, P_GATE_UP, e->xq_hidden, nullptr, e->ssq_part, nullptr, e->xq_act, nullptr, nullptr,
                                st);
  if (rc) return rc;
  const bool last = l + 1 == e->cfg.layers;  // the last layer's output feeds the head, which reads fp32
  return engine_row_parallel_xq(e, l, P_DOWN, e->xq_act, last ? kNoXq : e->xq_hidden,
                                last ? nullptr : e->layers[l + 1].ln1, last ? nullptr : e->ssq_part, st);
}

// projection k of layer l in the fp32-activation step: integer / table blobs through the tile / generic GEMVs, fp8 layers
// through the fp8 matrix-core GEMV
static int engine_linear_f32(woq_engine* e, int l, Proj k, const float* act, int lda, float* out, int ldo,
                             const float* norm_w, const float* residual, hipStream_t st) {
  const woq_engine_config& c = e->cfg;
  const EngineProj& p = e->layers[l].p[k];
  if (e->fp8_type != 0)
    return launch_gemv_fp8_engine(act, lda, p.blob, p.hdr, p.fp8_lo, e->fp8_type, out, ldo, norm_w, c.rms_eps, residual,
                                  c.hidden, kProjEpi[k], e->gu_tmp, st);
  const float* bias = nullptr;
  if (const int rc = engine_lora_bias(e, l, k, kNoXq, nullptr, act, norm_w, st, &bias)) return rc;
  return launch_gemv_from_header(act, WOQ_F32, lda, p.blob, p.hdr, bias, out, WOQ_F32, ldo, 1, norm_w, c.rms_eps, residual,
                                 c.hidden, kProjEpi[k], st);
}

static int engine_attn_block(woq_engine* e, int l, hipStream_t st) {
  if (e->use_xq()) return engine_attn_block_xq(e, l, st);
  const woq_engine_config& c = e->cfg;
  const EngineLayer& w = e->layers[l];
  int rc = engine_linear_f32(e, l, P_QKV, e->hidden, c.hidden, e->qkv, w.p[P_QKV].hdr.N, w.ln1, nullptr, st);
  if (rc) return rc;
  rc = launch_attn_decode(e->attn_plan(l, e->attn_opt), e->attn_io(l, kNoXq), st);
  if (rc) return rc;
  return engine_linear_f32(e, l, P_O, e->attn, c.heads * c.head_dim, e->hidden, c.hidden, nullptr,
                           e->tp_residual(e->hidden), st);
}

static int engine_mlp_block(woq_engine* e, int l, hipStream_t st) {
  if (e->use_xq()) return engine_mlp_block_xq(e, l, st);
  const woq_engine_config& c = e->cfg;
  const int rc = engine_linear_f32(e, l, P_GATE_UP, e->hidden, c.hidden, e->act, c.inter, e->layers[l].ln2, nullptr, st);
  if (rc) return rc;
  return engine_linear_f32(e, l, P_DOWN, e->act, c.inter, e->hidden, c.hidden, nullptr, e->tp_residual(e->hidden), st);
}

// A sampler's penalty changes values after the lm_head, so its pairs are of no use; the prompt pass's lm_head emits none.
// fuse_next: this step's greedy argmax and the NEXT step's embedding kernel as one launch (steps chained inside one
// captured graph; one GPU) — woq_ops.hip argmax_embed_kernel. A vocab-sharded head: one (max, global index) pair per rank
Tail woq_engine::tail(bool greedy, bool fuse_next, bool after_prompt) const {
  if (!greedy) return {PICK_NONE, false};
  if (sampler_on) return {PICK_SAMPLED, false};
  if (after_prompt) return {PICK_ARGMAX_FULL, false};
  if (fuse_next && cfg.tp_size <= 1 && comm == nullptr) return {PICK_ARGMAX_EMBED, true};
  return {comm != nullptr && cfg.tp_size > 1 ? PICK_TP_GREEDY : PICK_ARGMAX_PAIRS, true};
}
static bool engine_can_fuse_next(const woq_engine* e, int greedy) {
  return e->tail(greedy != 0, true, false).pick == PICK_ARGMAX_EMBED;  // sampled chains: sample -> embed
}
// the controls' memory travels with controls or a guide (which reads neutral controls when none are installed)
SampleTail woq_engine::sample_tail() const {
  SampleTail t;
  t.logits = logits, t.vocab = cfg.vocab, t.seen = samp_seen, t.cfg = samp_cfg;
  if (controls_on || guide_on) t.counts = samp_count, t.bias = samp_bias, t.ctl = samp_ctl, t.adj = samp_adj;
  if (guide_on) t.guide = guide;
  t.token = token, t.pos_advance = pos, t.log = tok_log, t.status = fuse_status, t.discarded = discarded;
  return t;
}
// the record of the pick that was just launched: reads token[0], pos[0] - 1 and the logits, which the stream orders
// before the next lm_head (also behind a fused argmax + embed launch: that one writes the residual stream, not logits)
static int engine_logprobs(woq_engine* e, hipStream_t st) {
  if (!e->logprobs_on) return 0;
  return launch_logprobs(e->logits, e->cfg.vocab, e->token, e->pos, e->cfg.max_ctx + 1, e->lp_ws, e->lp_chosen,
                         e->lp_top_id, e->lp_top_lp, st);
}
// the pick, then its record (the tensor-parallel greedy pick has none: the record needs the whole vocabulary)
static int engine_tail(woq_engine* e, TailPick pick, hipStream_t st) {
  const woq_engine_config& c = e->cfg;
  const int n_pairs = (c.vocab + 15) / 16;  // of the lm_head's (max, index) pairs
  switch (pick) {
    case PICK_NONE: return 0;
    case PICK_TP_GREEDY:
      return woq_comm_launch_greedy(e->comm, e->am_val, e->am_idx, n_pairs, e->vocab_offset, e->token, e->pos, e->tok_log,
                                    e->fuse_status, st);
    case PICK_SAMPLED: {  // token <- sample(logits), tok_log[pos] = token, pos += 1; a guide's state follows the pick
      const SampleTail t = e->sample_tail();
      if (const int rc = launch_sample_tail(t, st)) return rc;
      if (t.guide != nullptr) launch_guide_advance(e->guide, t.vocab, t.token, t.status, st);
      break;
    }
    case PICK_ARGMAX_FULL: launch_argmax(e->logits, c.vocab, e->token, e->pos, st); break;  // token <- argmax, pos += 1
    case PICK_ARGMAX_PAIRS:
      launch_argmax_pairs(e->am_val, e->am_idx, n_pairs, e->token, e->pos, e->tok_log, e->fuse_status, st);
      break;
    case PICK_ARGMAX_EMBED: {
      const bool xq = e->use_xq();
      launch_argmax_embed(e->am_val, e->am_idx, n_pairs, e->token, e->pos, e->tok_log, e->embed, e->embed_dtype, c.hidden,
                          e->hidden, xq ? e->layers[0].ln1 : nullptr, xq ? e->xq_hidden : kNoXq,
                          xq ? e->ssq_part : nullptr, e->step_seq, c.max_ctx, e->fuse_status, st);
    }
  }
  return engine_logprobs(e, st);
}
static int engine_head(woq_engine* e, int greedy, hipStream_t st, bool fuse_next = false) {
  const woq_engine_config& c = e->cfg;
  const Tail t = e->tail(greedy != 0, fuse_next, false);
  launch_lm_head(e->hidden, e->final_norm, c.rms_eps, e->lm_head, e->lm_dtype, c.hidden, c.vocab, e->logits,
                 t.pairs ? e->am_val : nullptr, t.pairs ? e->am_idx : nullptr, st);
  return engine_tail(e, t.pick, st);
}

// sum of the row-parallel partials over the tensor-parallel ranks, in place on the residual stream, after sub-block
// `which` (0 attention, 1 MLP) of layer l. XQ path: the producing GEMV already pushed this rank's share (tp_push) and
// the summed vector leaves as the next GEMV's XQ input as well.
static int engine_allreduce_after(woq_engine* e, int l, int which, hipStream_t st) {
  const woq_engine_config& c = e->cfg;
  if (c.tp_size <= 1) return 0;
  if (e->comm && e->use_xq()) {
    const bool last = which == 1 && l + 1 == c.layers;
    const float* nw = which == 0 ? e->layers[l].ln2 : (last ? nullptr : e->layers[l + 1].ln1);
    return woq_comm_launch_allreduce_ex(e->comm, e->hidden, (size_t)c.hidden, e->tp_push() != nullptr ? 1 : 0, nw,
                                        last ? kNoXq : e->xq_hidden, last ? nullptr : e->ssq_part, st);
  }
  float* buf = e->hidden;
  const size_t count = (size_t)c.hidden;
  if (e->comm) return woq_comm_launch_allreduce(e->comm, buf, count, st);
  if (e->allreduce && e->allreduce(e->allreduce_user, buf, count, st) != 0)
    return woq::fail("QBits: tensor-parallel all-reduce callback failed");
  return 0;
}

// prompt pass: [rows, hidden] partials. Bandwidth-bound, so the bound callback (RCCL through torch.distributed) is the
// transport when there is one; without it the device exchange carries the rows in inbox-sized pieces.
static int engine_allreduce_rows(woq_engine* e, float* buf, size_t count, hipStream_t st) {
  if (e->cfg.tp_size <= 1) return 0;
  if (e->allreduce) {
    if (e->allreduce(e->allreduce_user, buf, count, st) != 0)
      return woq::fail("QBits: tensor-parallel all-reduce callback failed");
    return 0;
  }
  if (!e->comm) return woq::fail("QBits: tensor-parallel engine without a communicator");
  const size_t piece = woq_comm_max_elems(e->comm);
  for (size_t o = 0; o < count; o += piece) {
    const int rc = woq_comm_launch_allreduce(e->comm, buf + o, std::min(piece, count - o), st);
    if (rc) return rc;
  }
  return 0;
}

static void engine_embed(woq_engine* e, hipStream_t st) {
  const bool xq = e->use_xq();
  launch_embed(e->embed, e->embed_dtype, e->token, e->cfg.hidden, e->hidden, xq ? e->layers[0].ln1 : nullptr,
               xq ? e->xq_hidden : kNoXq, xq ? e->ssq_part : nullptr, e->step_seq, e->pos, e->cfg.max_ctx, e->fuse_status,
               st);
}

// chain bit 0: the previous step of the same captured graph already ran this step's embedding (its fused tail);
// bit 1: this step's tail is fused with the next step's embedding
static int engine_step_impl(woq_engine* e, int greedy, hipStream_t st, int chain = 0) {
  const woq_engine_config& c = e->cfg;
  const bool fuse_next = (chain & 2) != 0;
  if (!(chain & 1)) engine_embed(e, st);
  for (int l = 0; l < c.layers; ++l) {
    int rc = engine_attn_block(e, l, st);
    if (rc) return rc;
    if ((rc = engine_allreduce_after(e, l, 0, st)) != 0) return rc;
    rc = engine_mlp_block(e, l, st);
    if (rc) return rc;
    if ((rc = engine_allreduce_after(e, l, 1, st)) != 0) return rc;
  }
  return engine_head(e, greedy, st, fuse_next);
}

// ---- prompt pass -------------------------------------------------------------------------------------------------
// HF runs the prompt as ONE forward over [batch, T] (generation's first step); the reference's qbits linears then see
// M = batch * T rows (nn/modules.py:140-169). Same here: every linear is one MFMA GEMM over all rows
// (woq_gemm_f16.hip: RMSNorm fused into the activation pack pass, residual add / SiLU*mul fused into the epilogue),
// attention is one launch per layer over the KV cache (woq_prefill.hip). 6 launches + 4 pack passes per layer.

// the adapters' share of the prompt pass's buffers: the shrink's output for `rows` rows and, while gate or up is
// targeted somewhere, the un-activated gate/up rows
static int engine_prefill_reserve_lora(woq_engine* e, size_t rows) {
  const woq_engine_config& c = e->cfg;
  bool any = false, gu = false;
  for (int l = 0; l < c.layers; ++l)
    for (int k = 0; k < P_COUNT; ++k)
      if (e->lora_rows(l, k) > 0) any = true, gu = gu || k == P_GATE_UP;
  if (any && rows > e->pf_t_rows) {
    WOQ_HIP(hipDeviceSynchronize());
    if (e->pf_t) WOQ_HIP(hipFree(e->pf_t));
    e->pf_t = nullptr, e->pf_t_rows = 0;
    WOQ_HIP(hipMalloc((void**)&e->pf_t, rows * (size_t)e->lora_ldt() * 4));
    e->pf_t_rows = rows;
  }
  if (gu && rows > e->pf_gu_rows) {
    WOQ_HIP(hipDeviceSynchronize());
    if (e->pf_gu) WOQ_HIP(hipFree(e->pf_gu));
    e->pf_gu = nullptr, e->pf_gu_rows = 0;
    WOQ_HIP(hipMalloc((void**)&e->pf_gu, rows * (size_t)c.inter * 2 * 2));
    e->pf_gu_rows = rows;
  }
  return 0;
}

static int engine_prefill_reserve(woq_engine* e, size_t rows) {
  const woq_engine_config& c = e->cfg;
  if (e->lora_rmax > 0)
    if (const int rc = engine_prefill_reserve_lora(e, rows)) return rc;
  // the largest call's workspace over EVERY layer's blobs: packed activation tiles + scales (+ the fragment image of a
  // table-type blob, so that such prompt passes allocate nothing per call either)
  size_t ws = 0;
  for (const EngineLayer& w : e->layers)
    for (const EngineProj& p : w.p)
      ws = std::max(ws, gemm_f16_workspace_bytes_blob((int)rows, p.hdr, 1, e->fp8_type != 0));
  if (rows <= e->pf_rows && ws <= e->pf_ws_bytes) return 0;
  WOQ_HIP(hipDeviceSynchronize());
  for (void* p : {(void*)e->pf_h, (void*)e->pf_qkv, (void*)e->pf_attn, (void*)e->pf_act, e->pf_ws})
    if (p) WOQ_HIP(hipFree(p));
  e->pf_h = nullptr, e->pf_qkv = nullptr, e->pf_attn = nullptr, e->pf_act = nullptr, e->pf_ws = nullptr;
  e->pf_rows = 0;
  const size_t qkv_n = (size_t)(c.heads + 2 * c.kv_heads) * c.head_dim;
  WOQ_HIP(hipMalloc((void**)&e->pf_h, rows * c.hidden * 4));
  WOQ_HIP(hipMalloc((void**)&e->pf_qkv, rows * qkv_n * 2));
  WOQ_HIP(hipMalloc((void**)&e->pf_attn, rows * (size_t)c.heads * c.head_dim * 2));
  WOQ_HIP(hipMalloc((void**)&e->pf_act, rows * (size_t)c.inter * 2));
  WOQ_HIP(hipMalloc((void**)&e->pf_ws, ws));
  e->pf_rows = rows;
  e->pf_ws_bytes = ws;
  return 0;
}

// The prompt pass's GEMM call: projection k of layer l over M rows. The column-parallel ones (qkv, gate/up) read the
// residual stream through RMSNorm `norm_w`, the row-parallel ones (o, down) add onto it.
static int engine_prefill_gemm(woq_engine* e, int l, Proj k, int M, const void* act, int act_dtype, int lda, void* out,
                               int out_dtype, int ldo, const float* norm_w, hipStream_t st, int epi = -1) {
  const woq_engine_config& c = e->cfg;
  const EngineProj& p = e->layers[l].p[k];
  const bool rowp = k == P_O || k == P_DOWN;
  return launch_gemm_f16(act, act_dtype, lda, p.blob, p.hdr, k == P_QKV ? e->layers[l].qkv_bias : nullptr, out, out_dtype,
                         ldo, M, norm_w,
                         rowp ? 0.f : c.rms_eps, rowp ? e->tp_residual(e->pf_h) : nullptr, rowp ? c.hidden : 0,
                         epi < 0 ? kProjEpi[k] : epi, e->pf_ws, 0, st, p.fp8_lo, e->fp8_type, e->pf_ws_bytes);
}

// The adapter of (l, k) over the prompt pass's M rows (woq_lora.hip): T = inv * A . (X * norm_w), then the expand in the
// kind's store mode. qkv: onto the fp16 q | k | v rows after the base GEMM (one more fp16 rounding of q, k, v than the
// adapter-less pass has); o_proj / down_proj: onto the fp32 residual stream BEFORE the base GEMM, which adds onto it through
// its residual slot; gate/up: the base GEMM left plain gate / up rows in pf_gu, the expand adds, applies SiLU * mul and
// writes pf_act. Only called for a (layer, kind) with an adapter.
static int engine_prefill_lora(woq_engine* e, int l, Proj k, int M, hipStream_t st) {
  const woq_engine_config& c = e->cfg;
  const woq_blob_header& h = e->layers[l].p[k].hdr;
  const LoraDesc* d = e->lora_dev(l, k);
  const EngineLayer& w = e->layers[l];
  const void* x = k == P_O ? (const void*)e->pf_attn : k == P_DOWN ? (const void*)e->pf_act : (const void*)e->pf_h;
  const bool f32 = k == P_QKV || k == P_GATE_UP;
  const float* norm_w = k == P_QKV ? w.ln1 : k == P_GATE_UP ? w.ln2 : nullptr;
  int rc = launch_lora_shrink(d, e->lora_rows(l, k), x, f32 ? WOQ_F32 : WOQ_F16, h.K, M, h.K, norm_w, c.rms_eps, e->pf_t,
                              e->lora_ldt(), st);
  if (rc) return rc;
  switch (k) {
    case P_QKV: return launch_lora_expand(d, e->pf_t, e->lora_ldt(), M, h.N, LORA_EXPAND_ADD_F16, e->pf_qkv, h.N, nullptr, 0, st);
    case P_GATE_UP:
      return launch_lora_expand(d, e->pf_t, e->lora_ldt(), M, h.N, LORA_EXPAND_SILU, e->pf_act, c.inter, e->pf_gu, h.N, st);
    default: return launch_lora_expand(d, e->pf_t, e->lora_ldt(), M, h.N, LORA_EXPAND_ADD_F32, e->pf_h, c.hidden, nullptr, 0, st);
  }
}

static int engine_prefill_impl(woq_engine* e, const int32_t* tokens, int n_seq, int T, int start, int greedy,
                               hipStream_t st) {
  const woq_engine_config& c = e->cfg;
  const int M = n_seq * T;
  const int qkv_n = (c.heads + 2 * c.kv_heads) * c.head_dim;
  const size_t seq_stride = e->kv_layer_bytes / woq_dtype_size((uint32_t)c.kv_dtype) * c.layers;  // elements between sequences
  int rc = engine_prefill_reserve(e, (size_t)M);
  if (rc) return rc;
  launch_embed_rows(e->embed, e->embed_dtype, tokens, M, c.hidden, e->pf_h, st);
  for (int l = 0; l < c.layers; ++l) {
    const EngineLayer& w = e->layers[l];
    uint8_t *kc = e->k_of(l), *vc = e->v_of(l);
    rc = engine_prefill_gemm(e, l, P_QKV, M, e->pf_h, WOQ_F32, c.hidden, e->pf_qkv, WOQ_F16, qkv_n, w.ln1, st);
    if (rc) return rc;
    if (e->lora_rows(l, P_QKV) > 0 && (rc = engine_prefill_lora(e, l, P_QKV, M, st)) != 0) return rc;
    if ((rc = launch_rope_append(e->pf_qkv, n_seq, T, start, c.heads, c.kv_heads, c.head_dim, e->cs, e->sn, kc, vc,
                                 c.kv_dtype, seq_stride, st, w.q_norm, w.k_norm, c.rms_eps)) != 0)
      return rc;
    if ((rc = launch_attn_prefill(e->pf_qkv, n_seq, T, start, c.heads, c.kv_heads, c.head_dim, kc, vc, c.kv_dtype,
                                  seq_stride, e->pf_attn, e->window, st)) != 0)
      return rc;
    if (e->lora_rows(l, P_O) > 0 && (rc = engine_prefill_lora(e, l, P_O, M, st)) != 0) return rc;
    rc = engine_prefill_gemm(e, l, P_O, M, e->pf_attn, WOQ_F16, c.heads * c.head_dim, e->pf_h, WOQ_F32, c.hidden, nullptr, st);
    if (rc) return rc;
    if ((rc = engine_allreduce_rows(e, e->pf_h, (size_t)M * c.hidden, st)) != 0) return rc;
    if (e->lora_rows(l, P_GATE_UP) > 0) {  // plain gate / up rows, then the adapter's expand applies SiLU * mul
      rc = engine_prefill_gemm(e, l, P_GATE_UP, M, e->pf_h, WOQ_F32, c.hidden, e->pf_gu, WOQ_F16, 2 * c.inter, w.ln2, st, 0);
      if (rc == 0) rc = engine_prefill_lora(e, l, P_GATE_UP, M, st);
    } else {
      rc = engine_prefill_gemm(e, l, P_GATE_UP, M, e->pf_h, WOQ_F32, c.hidden, e->pf_act, WOQ_F16, c.inter, w.ln2, st);
    }
    if (rc) return rc;
    if (e->lora_rows(l, P_DOWN) > 0 && (rc = engine_prefill_lora(e, l, P_DOWN, M, st)) != 0) return rc;
    rc = engine_prefill_gemm(e, l, P_DOWN, M, e->pf_act, WOQ_F16, c.inter, e->pf_h, WOQ_F32, c.hidden, nullptr, st);
    if (rc) return rc;
    if ((rc = engine_allreduce_rows(e, e->pf_h, (size_t)M * c.hidden, st)) != 0) return rc;
  }
  // logits of every sequence's last position; sequence 0 also lands in the decode step's buffers
  launch_gather_last(e->pf_h, n_seq, T, c.hidden, e->pf_last, st);
  for (int s = 0; s < n_seq; ++s)
    launch_lm_head(e->pf_last + (size_t)s * c.hidden, e->final_norm, c.rms_eps, e->lm_head, e->lm_dtype, c.hidden,
                   c.vocab, e->pf_logits + (size_t)s * c.vocab, nullptr, nullptr, st);
  WOQ_HIP(hipMemcpyAsync(e->hidden, e->pf_last, (size_t)c.hidden * 4, hipMemcpyDeviceToDevice, st));
  WOQ_HIP(hipMemcpyAsync(e->logits, e->pf_logits, (size_t)c.vocab * 4, hipMemcpyDeviceToDevice, st));
  WOQ_HIP(hipMemsetD32Async((hipDeviceptr_t)e->pos, start + T - 1, 1, st));
  // greedy: token <- sample at counter start + T - 1 or argmax, pos <- start + T, and the first generated token's
  // record, row start + T - 1
  return engine_tail(e, e->tail(greedy != 0, false, true).pick, st);
}

// `reps` passes of `body(stream)` between two events on `st` (after one untimed pass): what the launches cost inside the
// engine's own regime. eager: the passes issued back to back on `st` — how decode bursts run with WOQ_ENGINE_LAUNCH=eager;
// otherwise ONE pass captured on a private stream and its graph launched on `st` itself, the way the decode step's graph
// is replayed since round 4 (a graph launched on a stream that sits behind a cross-stream event wait pays ~1 us per
// kernel boundary, profiles/r04ab_stream_mode_probe.txt — so the capture stream is never the launch stream here).
template <typename F>
static int time_captured(hipStream_t st, int reps, F body, float* total_ms, bool eager = false) {
  int rc = body(st);  // eager once: lazy kernel attributes outside of capture
  if (rc) return rc;
  WOQ_HIP(hipStreamSynchronize(st));
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  hipStream_t cs = nullptr;
  auto cleanup = [&]() {
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
    if (ge) hipGraphExecDestroy(ge);
    if (g) hipGraphDestroy(g);
    if (cs) hipStreamDestroy(cs);
  };
#define WOQ_TC(expr)                                                                               \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      cleanup();                                                                                   \
      return woq::fail(std::string("QBits: HIP error '") + hipGetErrorString(_e) + "' at " #expr); \
    }                                                                                              \
  } while (0)
  WOQ_TC(hipEventCreate(&ev0));
  WOQ_TC(hipEventCreate(&ev1));
  if (eager) {
    if ((rc = body(st)) != 0) {
      cleanup();
      return rc;
    }
    WOQ_TC(hipEventRecord(ev0, st));
    for (int r = 0; r < reps; ++r)
      if ((rc = body(st)) != 0) {
        cleanup();
        return rc;
      }
  } else {
    WOQ_TC(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    WOQ_TC(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    rc = body(cs);
    hipError_t ce = hipStreamEndCapture(cs, &g);
    if (rc) {
      cleanup();
      return rc;
    }
    WOQ_TC(ce);
    WOQ_TC(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    WOQ_TC(hipGraphLaunch(ge, st));
    WOQ_TC(hipEventRecord(ev0, st));
    for (int r = 0; r < reps; ++r) WOQ_TC(hipGraphLaunch(ge, st));
  }
  WOQ_TC(hipEventRecord(ev1, st));
  WOQ_TC(hipStreamSynchronize(st));
  WOQ_TC(hipEventElapsedTime(total_ms, ev0, ev1));
#undef WOQ_TC
  cleanup();
  return 0;
}

extern "C" {

int woq_engine_prefill(woq_engine* e, const int32_t* tokens_dev, int n_seq, int T, int start_pos, int greedy,
                       void* stream) {
  WOQ_TRY
  WOQ_CHECK(e && e->embed && e->lm_head, "QBits: engine head not set");
  WOQ_CHECK(tokens_dev && n_seq >= 1 && T >= 1 && start_pos >= 0, "QBits: bad prefill arguments");
  WOQ_CHECK(n_seq <= e->max_batch, "QBits: prefill batch exceeds the engine's max_batch");
  WOQ_CHECK(start_pos + T <= e->cfg.max_ctx, "QBits: prefill runs past max_ctx");
  WOQ_CHECK_LAYERS(e);
  WOQ_CHECK((long long)n_seq * T < (1ll << 31), "QBits: prefill row count overflows");
  int rc = engine_prefill_impl(e, tokens_dev, n_seq, T, start_pos, greedy, (hipStream_t)stream);
  if (rc) return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

int woq_engine_prefill_scored(woq_engine* e, const int32_t* tokens_dev, int T, int start_pos,
                              const int32_t* targets_dev, int greedy, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e && e->embed && e->lm_head, "QBits: engine head not set");
  WOQ_CHECK(tokens_dev && targets_dev && T >= 1 && start_pos >= 0, "QBits: bad prefill arguments");
  WOQ_CHECK(start_pos + T <= e->cfg.max_ctx, "QBits: prefill runs past max_ctx");
  WOQ_CHECK(e->whole_vocab(), "QBits: a tensor-parallel engine cannot score a prompt (its lm_head is vocab-sharded)");
  WOQ_CHECK(e->lp_chosen != nullptr, "QBits: no log-probability log before the first woq_engine_set_logprobs(e, 1)");
  const woq_engine_config& c = e->cfg;
  if (const char* why = score_shape_problem(e->lm_head, e->lm_dtype, c.hidden, c.vocab)) return woq::fail(why);
  WOQ_CHECK_LAYERS(e);  // (after the argument checks, before the first allocation and launch)
  const hipStream_t st = (hipStream_t)stream;
  if (e->score_ws == nullptr) WOQ_HIP(hipMalloc(&e->score_ws, score_workspace_bytes(c.hidden, c.vocab)));
  int rc = engine_prefill_impl(e, tokens_dev, 1, T, start_pos, greedy, st);
  if (rc) return rc;
  const int rows = greedy ? T - 1 : T;  // greedy: row start_pos + T - 1 is the chaining tail's
  if (rows > 0) {
    rc = launch_score_rows(e->pf_h, e->final_norm, c.rms_eps, e->lm_head, e->lm_dtype, c.hidden, c.vocab, targets_dev,
                           rows, start_pos, c.max_ctx + 1, e->score_ws, e->lp_chosen, e->lp_top_id, e->lp_top_lp, st);
    if (rc) return rc;
  }
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

void* woq_engine_prefill_logits_ptr(woq_engine* e) { return e ? e->pf_logits : nullptr; }
void* woq_engine_prefill_rows_ptr(woq_engine* e) { return e ? e->pf_h : nullptr; }
int woq_engine_set_attn_splits(woq_engine* e, int splits) {
  WOQ_TRY
  WOQ_CHECK(e && splits >= 1 && splits <= 64, "QBits: attn_splits must be in [1, 64]");
  e->attn_opt.splits = splits;  // takes effect at the next step / capture (a captured graph keeps its own)
  WOQ_END
}
int woq_engine_attn_splits(woq_engine* e) { return e ? e->attn_opt.splits : 0; }
int woq_engine_set_attn_grouped(woq_engine* e, int on) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr, "QBits: null engine");
  e->attn_opt.grouped = on != 0;
  WOQ_END
}
int woq_engine_attn_grouped(woq_engine* e) { return e ? (int)e->attn_opt.grouped : 0; }
int woq_engine_set_attn_chunk(woq_engine* e, int chunk) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr && chunk >= 0 && chunk % 32 == 0, "QBits: attn_chunk must be a non-negative multiple of 32");
  e->attn_opt.chunk_fixed = chunk;  // takes effect at the next step / capture
  WOQ_END
}
int woq_engine_attn_chunk(woq_engine* e) { return e ? e->attn_opt.chunk_fixed : 0; }
int woq_engine_set_time_eager(woq_engine* e, int on) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr, "QBits: null engine");
  e->time_eager = on != 0;
  WOQ_END
}
int woq_engine_set_tp_options(woq_engine* e, int xq, int fused_push) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr, "QBits: null engine");
  e->tp_xq = xq != 0;
  e->tp_fused_push = fused_push != 0;
  WOQ_END
}
int woq_engine_set_fuse_attn(woq_engine* e, int on) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr, "QBits: null engine");
  e->attn_opt.fuse_attn = on != 0;
  WOQ_END
}
int woq_engine_status(woq_engine* e, void* stream) {  // bit 0 hand-off give-up, bit 1 position clamp
  if (!e || !e->fuse_status) return 0;
  int v = 0;
  if (hipMemcpyAsync(&v, e->fuse_status, 4, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return -1;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  return v;
}
int woq_engine_clear_status(woq_engine* e, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e, "QBits: null engine");
  if (e->fuse_status) WOQ_HIP(hipMemsetAsync(e->fuse_status, 0, 4, (hipStream_t)stream));
  // the slices' arrival counters return to zero by themselves when a merge completes; an aborted launch would leave
  // them mid-count and no later merge would ever fire (WOQ_ATTN_FOLD=1 only)
  if (e->attn_cnt) WOQ_HIP(hipMemsetAsync(e->attn_cnt, 0, (size_t)e->cfg.heads * 4, (hipStream_t)stream));
  WOQ_END
}
int woq_engine_fuse_attn(woq_engine* e) {
  if (!e || !e->use_xq() || e->layers.empty()) return 0;
  return e->attn_plan(0, e->attn_opt).form == ATTN_FUSED ? 1 : 0;
}
int woq_engine_attn_plan(woq_engine* e, int splits, int grouped, long long* out11) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr && out11 != nullptr && !e->layers.empty() && splits <= 64, "QBits: bad argument");
  AttnOptions o = e->attn_opt;  // a copy: the engine keeps its own
  if (splits > 0) o.splits = splits;
  if (grouped >= 0) o.grouped = grouped != 0;
  attn_plan_report(e->attn_plan(0, o), out11);  // a refused plan is an answer too: its form, and refused = 1
  WOQ_END
}
void* woq_engine_kv_cache_ptr(woq_engine* e, int which) { return e ? (which ? e->vcache : e->kcache) : nullptr; }

// rolling KV cache: every argument is checked before the first launch, so a refused call leaves the cache as it was
int woq_engine_kv_shift(woq_engine* e, int seq, int n_keep, int n_discard, int n_cached, int move_pos, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr, "QBits: null engine");
  const woq_engine_config& c = e->cfg;
  WOQ_CHECK(c.tp_size <= 1 && e->comm == nullptr && e->allreduce == nullptr,
            "QBits: the rolling KV cache runs on one GPU (no tensor-parallel shift)");
  WOQ_CHECK(e->window == 0, "QBits: the rolling KV cache does not combine with a sliding window");
  WOQ_CHECK(seq >= 0 && seq < e->max_batch, "QBits: KV shift: sequence outside [0, max_batch)");
  WOQ_CHECK(n_keep >= 0 && n_discard >= 1, "QBits: KV shift needs n_keep >= 0 and n_discard >= 1");
  WOQ_CHECK((long long)n_keep + n_discard <= n_cached, "QBits: KV shift: n_keep + n_discard exceeds the cached positions");
  WOQ_CHECK(n_cached <= c.max_ctx, "QBits: KV shift: n_cached exceeds the engine's max_ctx");
  WOQ_CHECK(move_pos == 0 || seq == 0, "QBits: KV shift: only sequence 0 has a position to move");
  WOQ_CHECK(e->cs != nullptr && e->sn != nullptr, "QBits: KV shift before woq_engine_set_head (no rotation tables)");
  const hipStream_t st = (hipStream_t)stream;
  const size_t seq_bytes = e->kv_layer_bytes * c.layers;
  if (const int rc = launch_kv_shift(e->kcache + seq_bytes * seq, e->vcache + seq_bytes * seq, c.kv_dtype, c.layers,
                                     c.kv_heads, c.head_dim, c.max_ctx, e->cs, e->sn, n_keep, n_discard, n_cached, st))
    return rc;
  if (move_pos != 0) launch_kv_shift_words(e->pos, e->discarded, n_discard, st);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}
void* woq_engine_discarded_ptr(woq_engine* e) { return e ? e->discarded : nullptr; }
int woq_engine_discarded_set(woq_engine* e, int value, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr, "QBits: null engine");
  launch_i32_store(e->discarded, value, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

int woq_engine_create(const woq_engine_config* cfg, woq_engine** out) {
  WOQ_TRY
  WOQ_CHECK(cfg && out, "QBits: null engine config");
  WOQ_CHECK(cfg->heads % cfg->kv_heads == 0, "QBits: heads must be a multiple of kv_heads");
  WOQ_CHECK(cfg->kv_dtype == WOQ_F16 || cfg->kv_dtype == WOQ_BF16 || cfg->kv_dtype == WOQ_FP8_E4M3,
            "QBits: kv_dtype must be fp16, bf16 or fp8_e4m3");
  woq_engine* e = new woq_engine();
  e->cfg = *cfg;
  e->layers.resize(cfg->layers);
  const int qkv_n = (cfg->heads + 2 * cfg->kv_heads) * cfg->head_dim;
  WOQ_HIP(hipMalloc((void**)&e->hidden, (size_t)cfg->hidden * 4));
  WOQ_HIP(hipMalloc((void**)&e->qkv, (size_t)qkv_n * 4));
  WOQ_HIP(hipMalloc((void**)&e->attn, (size_t)cfg->heads * cfg->head_dim * 4));
  WOQ_HIP(hipMalloc((void**)&e->act, (size_t)cfg->inter * 4));
  WOQ_HIP(hipMalloc((void**)&e->logits, (size_t)cfg->vocab * 4));
  WOQ_HIP(hipMalloc((void**)&e->token, 4));
  WOQ_HIP(hipMalloc((void**)&e->pos, 4));
  WOQ_HIP(hipMemset(e->token, 0, 4));
  WOQ_HIP(hipMemset(e->pos, 0, 4));
  WOQ_HIP(hipMalloc((void**)&e->discarded, 4));
  WOQ_HIP(hipMemset(e->discarded, 0, 4));
  e->kv_layer_bytes = (size_t)cfg->max_ctx * cfg->kv_heads * cfg->head_dim * woq_dtype_size((uint32_t)cfg->kv_dtype);
  // KV cache [sequence][layer][position][kv head][d]; sequence 0 is the one the decode step continues
  e->max_batch = cfg->reserved[0] > 1 ? cfg->reserved[0] : 1;
  const size_t kv_total = e->kv_layer_bytes * cfg->layers * e->max_batch;
  WOQ_HIP(hipMalloc((void**)&e->kcache, kv_total));
  WOQ_HIP(hipMalloc((void**)&e->vcache, kv_total));
  WOQ_HIP(hipMemset(e->kcache, 0, kv_total));
  WOQ_HIP(hipMemset(e->vcache, 0, kv_total));
  // decode attention slices: reserved[1] if given, else enough to fill the chip once the context is long
  e->attn_opt.splits = cfg->reserved[1] > 0 ? cfg->reserved[1]
                       : (cfg->max_ctx > 4096 ? std::max(2, std::min(32, 1024 / std::max(1, (int)cfg->heads))) : 1);
  WOQ_CHECK(e->attn_opt.splits <= 64, "QBits: attn_splits must be <= 64");
  e->window = cfg->reserved[2] > 0 ? cfg->reserved[2] : 0;
  WOQ_HIP(hipMalloc((void**)&e->attn_part, (size_t)cfg->heads * 64 * (cfg->head_dim + 2) * 4));  // room for 64 slices
  WOQ_HIP(hipMalloc((void**)&e->attn_cnt, (size_t)cfg->heads * 4));
  WOQ_HIP(hipMemset(e->attn_cnt, 0, (size_t)cfg->heads * 4));
  {
    const char* af = getenv("WOQ_ATTN_FOLD");
    e->attn_opt.fold = af ? af[0] != '0' : false;
    const char* ga = getenv("WOQ_GROUPED_A2A");
    e->attn_opt.grouped_a2a = ga ? ga[0] != '0' : true;
    const char* fs = getenv("WOQ_FUSE_SLICED");
    e->attn_opt.fuse_sliced = fs ? fs[0] != '0' : true;
  }
  WOQ_HIP(hipMalloc((void**)&e->tok_log, (size_t)(cfg->max_ctx + 1) * 4));
  WOQ_HIP(hipMemset(e->tok_log, 0, (size_t)(cfg->max_ctx + 1) * 4));
  WOQ_HIP(hipMalloc((void**)&e->am_val, (size_t)((cfg->vocab + 15) / 16) * 4));
  WOQ_HIP(hipMalloc((void**)&e->am_idx, (size_t)((cfg->vocab + 15) / 16) * 4));
  WOQ_HIP(hipMalloc((void**)&e->pf_last, (size_t)e->max_batch * cfg->hidden * 4));
  WOQ_HIP(hipMalloc((void**)&e->pf_logits, (size_t)e->max_batch * cfg->vocab * 4));
  WOQ_HIP(hipMalloc((void**)&e->step_seq, 8));  // step counter (hand-off tags) + sticky status word
  WOQ_HIP(hipMemset(e->step_seq, 0, 8));
  e->fuse_status = (int*)(e->step_seq + 1);
  WOQ_HIP(hipMalloc((void**)&e->samp_cfg, sizeof(woq_sampler_config)));
  WOQ_HIP(hipMemset(e->samp_cfg, 0, sizeof(woq_sampler_config)));
  WOQ_HIP(hipMalloc((void**)&e->samp_seen, (size_t)e->seen_words() * 4));
  WOQ_HIP(hipMemset(e->samp_seen, 0, (size_t)e->seen_words() * 4));
  e->owned = {e->hidden, e->qkv, e->attn, e->act, e->logits, e->token, e->pos, e->kcache, e->vcache, e->pf_last,
              e->pf_logits, e->attn_part, e->attn_cnt, e->am_val, e->am_idx, e->tok_log, e->step_seq, e->samp_cfg, e->samp_seen,
              e->discarded};
  {  // XQ vectors (woq_xq.h) for the three GEMV inputs of a layer
    // WOQ_ENGINE_XQ=0 turns the XQ hand-off off (the fp32-activation kernels). Round 2 picked by shape — at hidden 8192
    // the second recombination per tile cost more than the staging it removed (Llama-2-70B 119-120 vs 125-127 tokens/s);
    // with round 3's balanced digits and lean kernel the XQ path wins there too (129.1 vs 127.7 tokens/s, kernel 0.646
    // vs 0.624 of 8 TB/s, profiles/r03z_70b_xq.txt), and on the tensor-parallel rank shapes (2.32 vs 2.52 ms per token)
    const char* sw = getenv("WOQ_ENGINE_XQ");
    e->xq_enabled = sw ? sw[0] != '0' : true;
    const char* fa = getenv("WOQ_ENGINE_FUSE_ATTN");
    e->attn_opt.fuse_attn = fa ? fa[0] != '0' : true;
    const char* tx = getenv("WOQ_TP_XQ");
    e->tp_xq = tx ? tx[0] != '0' : true;
    const char* tf = getenv("WOQ_TP_FUSED_PUSH");
    e->tp_fused_push = tf ? tf[0] != '0' : true;
    const int attn_k = cfg->heads * cfg->head_dim;
    if ((cfg->hidden % 16) == 0 && (attn_k % 16) == 0 && (cfg->inter % 16) == 0) {
      void *bh = nullptr, *ba = nullptr, *bc = nullptr;
      WOQ_HIP(hipMalloc(&bh, xq_bytes(cfg->hidden)));
      WOQ_HIP(hipMalloc(&ba, xq_bytes(attn_k)));
      WOQ_HIP(hipMalloc(&bc, xq_bytes(cfg->inter)));
      WOQ_HIP(hipMalloc((void**)&e->ssq_part, (size_t)(cfg->hidden / 16) * 4));
      WOQ_HIP(hipMalloc((void**)&e->qkv_g, (size_t)qkv_n * 8));
      WOQ_HIP(hipMemset(e->qkv_g, 0, (size_t)qkv_n * 8));  // tag 0 is never a live tag
      const size_t pg_bytes = (size_t)cfg->heads * 64 * (cfg->head_dim + 2) * 8;
      WOQ_HIP(hipMalloc((void**)&e->attn_part_g, pg_bytes));
      WOQ_HIP(hipMemset(e->attn_part_g, 0, pg_bytes));
      WOQ_HIP(hipMemset(bh, 0, xq_bytes(cfg->hidden)));
      WOQ_HIP(hipMemset(ba, 0, xq_bytes(attn_k)));
      WOQ_HIP(hipMemset(bc, 0, xq_bytes(cfg->inter)));
      WOQ_HIP(hipMemset(e->ssq_part, 0, (size_t)(cfg->hidden / 16) * 4));
      e->xq_hidden = xq_carve(bh, cfg->hidden);
      e->xq_attn = xq_carve(ba, attn_k);
      e->xq_act = xq_carve(bc, cfg->inter);
      for (void* p : {bh, ba, bc, (void*)e->ssq_part, (void*)e->qkv_g, (void*)e->attn_part_g}) e->owned.push_back(p);
    }
  }
  *out = e;
  WOQ_END
}

static void engine_drop_graphs(woq_engine* e) {
  if (e->exec) hipGraphExecDestroy(e->exec);
  if (e->graph) hipGraphDestroy(e->graph);
  if (e->exec_k) hipGraphExecDestroy(e->exec_k);
  if (e->graph_k) hipGraphDestroy(e->graph_k);
  e->exec = e->exec_k = nullptr;
  e->graph = e->graph_k = nullptr;
}
static void engine_tail_changed(woq_engine* e, const TailKey& before) {
  if (!(e->tail_key() == before)) engine_drop_graphs(e);
}

void woq_engine_destroy(woq_engine* e) {
  if (!e) return;
  engine_drop_graphs(e);
  for (void* p : e->owned) hipFree(p);
  for (void* p : {(void*)e->pf_h, (void*)e->pf_qkv, (void*)e->pf_attn, (void*)e->pf_act, e->pf_ws})
    if (p) hipFree(p);
  if (e->score_ws) hipFree(e->score_ws);
  if (e->pf_t) hipFree(e->pf_t);
  if (e->pf_gu) hipFree(e->pf_gu);
  if (e->guide_table) hipFree(e->guide_table);
  delete e;
}

int woq_engine_set_layer(woq_engine* e, int layer, const woq_layer_weights* w) {
  WOQ_TRY
  WOQ_CHECK(e && w && layer >= 0 && layer < e->cfg.layers, "QBits: bad layer index");
  const woq_engine_config& c = e->cfg;
  // built and checked as a local: a refused call leaves the engine as it was (a layer set again starts without extras:
  // woq_engine_set_layer_extras comes after)
  EngineLayer in = {{{w->qkv_blob, w->qkv_hdr, nullptr},
                     {w->o_blob, w->o_hdr, nullptr},
                     {w->gate_up_blob, w->gate_up_hdr, nullptr},
                     {w->down_blob, w->down_hdr, nullptr}},
                    w->ln1,
                    w->ln2};
  auto all = [&](auto pred) { return std::all_of(std::begin(in.p), std::end(in.p), pred); };
  const woq_blob_header qkv = in.p[P_QKV].hdr, o = in.p[P_O].hdr, gu = in.p[P_GATE_UP].hdr, down = in.p[P_DOWN].hdr;
  // round 6: fp8_e4m3 / fp8_e5m2 layers (all four projections of every layer the same type; one GPU)
  const bool fp8 = woq_weight_is_fp8(qkv.weight_type);
  if (fp8) {
    WOQ_CHECK(all([&](const EngineProj& p) { return p.hdr.weight_type == qkv.weight_type; }),
              "QBits: an fp8 layer needs all four projections in the same fp8 type");
    WOQ_CHECK(c.tp_size <= 1, "QBits: fp8-weight layers run on one GPU (no tensor-parallel decode path)");
    WOQ_CHECK(e->lora_rmax == 0, "QBits: fp8-weight layers do not take LoRA adapters (woq_engine_lora_reserve has run)");
  } else {
    // int4, or (round 4) a 4-bit table type: the same kernels with a digit-plane unpack (woq_gemv_common.h LutArgs); the
    // fused qkv + attention launch stays int4-only (its support check says no)
    WOQ_CHECK(all([](const EngineProj& p) {
                return p.hdr.weight_type == WOQ_W_INT4_CLIP || (is_table_type(p.hdr.weight_type) && p.hdr.off_zp == 0);
              }),
              "QBits: the fused engine takes int4_clip / nf4 / fp4 / fp8 layers");
  }

  WOQ_CHECK(all([](const EngineProj& p) { return p.hdr.magic == WOQ_BLOB_MAGIC; }),
            "QBits: layer weights must be WQH1 blobs");
  WOQ_CHECK(qkv.K == c.hidden && qkv.N == (c.heads + 2 * c.kv_heads) * c.head_dim, "QBits: qkv blob shape mismatch");
  WOQ_CHECK(o.K == c.heads * c.head_dim && o.N == c.hidden, "QBits: o_proj blob shape mismatch");
  WOQ_CHECK(gu.K == c.hidden && gu.N == 2 * c.inter && (c.inter % 16) == 0,
            "QBits: gate_up blob shape mismatch (inter must be a multiple of 16)");
  WOQ_CHECK(down.K == c.inter && down.N == c.hidden, "QBits: down_proj blob shape mismatch");
  // one kind per engine, whichever order the layers arrive in (the layer being replaced does not count)
  in.kind = fp8 ? LAYER_FP8 : LAYER_INT;
  for (int l = 0; l < c.layers; ++l) {
    const EngineLayer& other = e->layers[l];
    if (l == layer || other.kind == LAYER_UNSET) continue;
    WOQ_CHECK(other.kind == in.kind, "QBits: fp8 and integer layers cannot be mixed in one engine");
    WOQ_CHECK(!fp8 || e->fp8_type == qkv.weight_type, "QBits: one fp8 type per engine");
  }
  if (fp8) {
    // the composite container [outer header][HI blob][LO blob] (include/woq_blob.h): the engine keeps the HI plane as the
    // projection's blob / header and the LO plane's tile data beside it; its headers follow from the outer one's parameters
    for (EngineProj& p : in.p) {
      const woq_blob_header outer = p.hdr;
      woq_blob_header o2, hi, lo;
      WOQ_CHECK(outer.off_shuffle == 0, "QBits: fp8 layers with g_idx stay on the module path");
      WOQ_CHECK(woq_fp8_headers(&o2, &hi, &lo, outer.K, outer.N, outer.group, outer.weight_type, outer.scale_type,
                                outer.compute_type, 0) == 0, "QBits: corrupt fp8 header");
      const uint8_t* base = (const uint8_t*)p.blob;
      p = {base + outer.off_q, hi, base + outer.off_scale + lo.off_q};  // the HI plane's blob, the LO plane's tile data
    }
    // (the one effect ahead of the commit: engine-owned scratch that nothing reads unless an fp8 layer is committed)
    if (e->gu_tmp == nullptr) {
      WOQ_HIP(hipMalloc((void**)&e->gu_tmp, (size_t)2 * c.inter * 4));
      e->owned.push_back(e->gu_tmp);
    }
  }
  // every check has passed: commit
  e->layers[layer] = in;
  e->fp8_type = fp8 ? qkv.weight_type : 0;  // (all set layers are of this kind)
  // xq_shapes_ok only ever goes from true to false: an engine whose fp8 (or XQ-refused) layer is later replaced by one
  // the XQ GEMV covers stays on the fp32-activation step — correct, only slower
  if (fp8)
    e->xq_shapes_ok = false;  // fp8 layers run the fp32-activation step
  else
    for (int k = 0; k < P_COUNT; ++k) e->xq_shapes_ok = e->xq_shapes_ok && gemv_xq_supported(in.p[k].hdr, kProjEpi[k]);
  WOQ_END
}

int woq_engine_set_layer_extras(woq_engine* e, int layer, const float* qkv_bias_dev, const float* q_norm_dev,
                                const float* k_norm_dev) {
  WOQ_TRY
  WOQ_CHECK(e && layer >= 0 && layer < e->cfg.layers, "QBits: bad layer index");
  EngineLayer& w = e->layers[layer];
  const bool any = qkv_bias_dev != nullptr || q_norm_dev != nullptr || k_norm_dev != nullptr;
  WOQ_CHECK(!any || (e->cfg.tp_size <= 1 && e->comm == nullptr && e->allreduce == nullptr),
            "QBits: layer extras (qkv bias, q/k norm) run on one GPU (no tensor-parallel path)");
  WOQ_CHECK(w.p[P_QKV].blob != nullptr, "QBits: woq_engine_set_layer_extras comes after woq_engine_set_layer");
  WOQ_CHECK((q_norm_dev != nullptr) == (k_norm_dev != nullptr), "QBits: q_norm and k_norm come together (both or neither)");
  WOQ_CHECK(qkv_bias_dev == nullptr || e->fp8_type == 0, "QBits: fp8-weight layers do not take a qkv bias");
  WOQ_CHECK(q_norm_dev == nullptr || (e->cfg.head_dim % 16) == 0, "QBits: a q/k norm needs head_dim to be a multiple of 16");
  // which extras are present decides which kernels a captured step holds (and their pointers are baked into it)
  if (w.qkv_bias != qkv_bias_dev || w.q_norm != q_norm_dev || w.k_norm != k_norm_dev) engine_drop_graphs(e);
  w.qkv_bias = qkv_bias_dev, w.q_norm = q_norm_dev, w.k_norm = k_norm_dev;
  WOQ_END
}

// ---- unmerged LoRA adapters ------------------------------------------------------------------------------------------
// target -> (projection kind, part of it, K, columns): q | k | v, o, gate / up, down
enum { LORA_TARGETS = 7 };
struct LoraTargetShape { Proj kind; int part, K, n; };
static LoraTargetShape lora_target_shape(const woq_engine_config& c, int target) {
  const int attn_k = c.heads * c.head_dim, kv_n = c.kv_heads * c.head_dim;
  switch (target) {
    case 0: return {P_QKV, 0, c.hidden, attn_k};
    case 1: return {P_QKV, 1, c.hidden, kv_n};
    case 2: return {P_QKV, 2, c.hidden, kv_n};
    case 3: return {P_O, 0, attn_k, c.hidden};
    case 4: return {P_GATE_UP, 0, c.hidden, c.inter};
    case 5: return {P_GATE_UP, 1, c.hidden, c.inter};
    default: return {P_DOWN, 0, c.inter, c.hidden};
  }
}
// why this engine cannot carry adapters (null = it can)
static const char* engine_lora_problem(const woq_engine* e) {
  if (e->cfg.tp_size > 1 || e->comm != nullptr || e->allreduce != nullptr)
    return "QBits: LoRA adapters run on one GPU (no tensor-parallel path)";
  if (e->fp8_type != 0) return "QBits: fp8-weight layers do not take LoRA adapters (their engine GEMV takes no bias)";
  return nullptr;
}
// the host mirror -> the device descriptors, between steps (steps in flight on any stream still read them)
static int engine_lora_upload(woq_engine* e) {
  WOQ_HIP(hipMemcpy(e->lora_desc, e->lora_host.data(), e->lora_host.size() * sizeof(LoraDesc), hipMemcpyHostToDevice));
  WOQ_HIP(hipDeviceSynchronize());
  return 0;
}

int woq_engine_lora_reserve(woq_engine* e, int r_max) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr, "QBits: null engine");
  WOQ_CHECK(r_max >= 1 && r_max <= LORA_MAX_RANK, "QBits: LoRA ranks run from 1 to 64");
  WOQ_CHECK(e->lora_rmax == 0, "QBits: woq_engine_lora_reserve runs once per engine");
  if (const char* why = engine_lora_problem(e)) return woq::fail(why);
  const woq_engine_config& c = e->cfg;
  size_t a_floats = 0, b_floats = 0;  // of one layer, at rank 1
  for (int t = 0; t < LORA_TARGETS; ++t) {
    const LoraTargetShape s = lora_target_shape(c, t);
    WOQ_CHECK(s.K >= 16 && (s.K & 15) == 0 && s.n >= 16 && (s.n & 15) == 0,
              "QBits: LoRA adapters need every projection's rows and columns to be multiples of 16");
    WOQ_CHECK(((size_t)s.K + LORA_MAX_ROWS + 4) * 4 <= (size_t)LORA_DELTA_MAX_LDS,
              "QBits: the LoRA delta launch holds K up to 40000 input values");
    a_floats += (size_t)s.K, b_floats += (size_t)s.n;
  }
  const size_t per_layer = (a_floats + b_floats) * r_max;  // every table's size is a multiple of 16 floats
  const int qkv_n = (c.heads + 2 * c.kv_heads) * c.head_dim;
  const size_t delta_floats = (size_t)qkv_n + c.hidden + 2 * (size_t)c.inter + c.hidden;
  float* tab = nullptr;
  LoraDesc* desc = nullptr;
  WOQ_HIP(hipMalloc((void**)&tab, (per_layer * c.layers + delta_floats) * 4));
  if (hipMalloc((void**)&desc, (size_t)c.layers * P_COUNT * sizeof(LoraDesc)) != hipSuccess) {
    hipFree(tab);
    return woq::fail("QBits: out of device memory for the LoRA descriptors");
  }
  WOQ_HIP(hipMemset(tab, 0, (per_layer * c.layers + delta_floats) * 4));
  e->owned.push_back(tab);
  e->owned.push_back(desc);
  e->lora_tab.assign((size_t)c.layers * LORA_TARGETS, woq_engine::LoraTable{nullptr, nullptr});
  e->lora_host.assign((size_t)c.layers * P_COUNT, LoraDesc{});
  float* cur = tab;
  for (int l = 0; l < c.layers; ++l) {
    for (int k = 0; k < P_COUNT; ++k) {
      LoraDesc& d = e->lora_host[(size_t)l * P_COUNT + k];
      d.n_parts = k == P_QKV ? 3 : k == P_GATE_UP ? 2 : 1;
      d.interleave = k == P_GATE_UP ? 1 : 0;
    }
    for (int t = 0; t < LORA_TARGETS; ++t) {
      const LoraTargetShape s = lora_target_shape(c, t);
      woq_engine::LoraTable& tb = e->lora_tab[(size_t)l * LORA_TARGETS + t];
      tb.A = cur, cur += (size_t)s.K * r_max;
      tb.B = cur, cur += (size_t)s.n * r_max;
      e->lora_host[(size_t)l * P_COUNT + s.kind].part[s.part] = LoraPart{tb.A, tb.B, 0, s.n, 0.f, 0};
    }
  }
  e->lora_delta[P_QKV] = cur, cur += qkv_n;
  e->lora_delta[P_O] = cur, cur += c.hidden;
  e->lora_delta[P_GATE_UP] = cur, cur += 2 * (size_t)c.inter;
  e->lora_delta[P_DOWN] = cur;
  e->lora_desc = desc;
  e->lora_rmax = r_max;  // (no part has a rank yet: no step changes, the captured graphs stay)
  return engine_lora_upload(e);
  WOQ_END
}

int woq_engine_set_lora(woq_engine* e, int layer, int target, const float* a_dev, const float* b_dev, int r,
                        float scaling) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr, "QBits: null engine");
  WOQ_CHECK(e->lora_rmax > 0, "QBits: woq_engine_set_lora comes after woq_engine_lora_reserve");
  if (const char* why = engine_lora_problem(e)) return woq::fail(why);
  WOQ_CHECK(layer >= 0 && layer < e->cfg.layers, "QBits: bad layer index");
  WOQ_CHECK(target >= 0 && target < LORA_TARGETS, "QBits: LoRA targets run from 0 (q_proj) to 6 (down_proj)");
  WOQ_CHECK(e->layers[layer].kind != LAYER_UNSET, "QBits: woq_engine_set_lora comes after woq_engine_set_layer");
  WOQ_CHECK(r >= 0 && r <= e->lora_rmax, "QBits: the adapter's rank exceeds the r_max of woq_engine_lora_reserve");
  WOQ_CHECK(r == 0 || (a_dev != nullptr && b_dev != nullptr), "QBits: a LoRA target needs its A and B tables");
  const LoraTargetShape s = lora_target_shape(e->cfg, target);
  const size_t di = (size_t)layer * P_COUNT + s.kind;
  const woq_engine::LoraTable& tb = e->lora_tab[(size_t)layer * LORA_TARGETS + target];
  const bool was = e->lora_rows(layer, s.kind) > 0;
  WOQ_HIP(hipDeviceSynchronize());  // steps in flight on any stream still read the tables
  if (r > 0) {
    WOQ_HIP(hipMemcpy(tb.A, a_dev, (size_t)r * s.K * 4, hipMemcpyDeviceToDevice));
    WOQ_HIP(hipMemcpy(tb.B, b_dev, (size_t)s.n * r * 4, hipMemcpyDeviceToDevice));
  }
  LoraPart& P = e->lora_host[di].part[s.part];
  P.r = r, P.s = r > 0 ? scaling : 0.f;
  if (const int rc = engine_lora_upload(e)) return rc;
  // which projections have an adapter decides which launches a captured step holds; ranks and values are device data
  if ((e->lora_rows(layer, s.kind) > 0) != was) engine_drop_graphs(e);
  WOQ_END
}

int woq_engine_clear_lora(woq_engine* e) {
  WOQ_TRY
  WOQ_CHECK(e != nullptr, "QBits: null engine");
  if (e->lora_rmax == 0 || e->lora_active_count() == 0) return 0;
  WOQ_HIP(hipDeviceSynchronize());
  for (LoraDesc& d : e->lora_host)
    for (LoraPart& P : d.part) P.r = 0, P.s = 0.f;
  if (const int rc = engine_lora_upload(e)) return rc;
  engine_drop_graphs(e);
  WOQ_END
}

int woq_engine_lora_on(woq_engine* e) { return e ? e->lora_active_count() : 0; }

int woq_engine_set_head(woq_engine* e, const void* embed_dev, int embed_dtype, const float* final_norm_dev,
                        const void* lm_head_dev, int lm_head_dtype, const float* cos_dev, const float* sin_dev) {
  WOQ_TRY
  WOQ_CHECK(e, "QBits: null engine");
  WOQ_CHECK(lm_head_dtype == WOQ_F16 || lm_head_dtype == WOQ_BF16, "QBits: lm_head must be fp16 or bf16");
  WOQ_CHECK((e->cfg.hidden % 8) == 0, "QBits: hidden must be a multiple of 8");
  e->embed = embed_dev;
  e->embed_dtype = embed_dtype;
  e->final_norm = final_norm_dev;
  e->lm_head = lm_head_dev;
  e->lm_dtype = lm_head_dtype;
  e->cs = cos_dev;
  e->sn = sin_dev;
  WOQ_END
}

int woq_engine_bind_io(woq_engine* e, void* token_dev, void* pos_dev, void* logits_dev, void* hidden_dev) {
  WOQ_TRY
  WOQ_CHECK(e, "QBits: null engine");
  // internal buffers stay allocated (freed in destroy via the *_own pointers)
  if (token_dev) e->token = (int32_t*)token_dev;
  if (pos_dev) e->pos = (int32_t*)pos_dev;
  if (logits_dev) e->logits = (float*)logits_dev;
  if (hidden_dev) e->hidden = (float*)hidden_dev;
  WOQ_END
}

void* woq_engine_token_log_ptr(woq_engine* e) { return e ? e->tok_log : nullptr; }
void* woq_engine_token_ptr(woq_engine* e) { return e->token; }
void* woq_engine_pos_ptr(woq_engine* e) { return e->pos; }
void* woq_engine_logits_ptr(woq_engine* e) { return e->logits; }
void* woq_engine_hidden_ptr(woq_engine* e) { return e->hidden; }

int woq_engine_set_allreduce(woq_engine* e, woq_allreduce_fn fn, void* user) {
  WOQ_TRY
  WOQ_CHECK(e, "QBits: null engine");
  WOQ_CHECK(fn == nullptr || e->lora_active_count() == 0, "QBits: LoRA adapters run on one GPU (no tensor-parallel path)");
  e->allreduce = fn;
  e->allreduce_user = user;
  WOQ_END
}

int woq_engine_set_comm(woq_engine* e, woq_comm* comm, int vocab_offset) {
  WOQ_TRY
  WOQ_CHECK(e, "QBits: null engine");
  WOQ_CHECK(vocab_offset >= 0, "QBits: bad vocabulary offset");
  WOQ_CHECK(comm == nullptr || e->lora_active_count() == 0, "QBits: LoRA adapters run on one GPU (no tensor-parallel path)");
  e->comm = comm;
  e->vocab_offset = vocab_offset;
  WOQ_END
}

int woq_engine_uses_xq(woq_engine* e) { return e && e->use_xq() ? 1 : 0; }

int woq_engine_set_sampler(woq_engine* e, const woq_sampler_config* cfg) {
  WOQ_TRY
  WOQ_CHECK(e, "QBits: null engine");
  const TailKey before = e->tail_key();
  if (cfg != nullptr) {
    WOQ_CHECK(e->whole_vocab(),
              "QBits: the native sampler needs the whole vocabulary on one GPU (a tensor-parallel head is vocab-sharded)");
    const char* why = sampler_config_problem(*cfg);
    if (why) return woq::fail(why);
    // the controls' own rule, whichever of the two entry points comes second
    WOQ_CHECK(!(e->controls_on && e->samp_ctl_host.min_p > 0.f && cfg->do_sample == 0),
              "QBits: min_p needs do_sample (greedy decoding keeps one token anyway)");
    // steps in flight on any stream still read the struct
    WOQ_HIP(hipDeviceSynchronize());
    WOQ_HIP(hipMemcpy(e->samp_cfg, cfg, sizeof(woq_sampler_config), hipMemcpyHostToDevice));
    e->samp_cfg_host = *cfg;
  }
  e->sampler_on = cfg != nullptr;
  if (!e->sampler_on) e->controls_on = e->guide_on = false;  // the controls and the guide live beside a sampler
  engine_tail_changed(e, before);
  WOQ_END
}

// the controls' device memory, on first use (never inside a capture: both callers are host-synchronous set-up calls)
static int engine_controls_alloc(woq_engine* e) {
  WOQ_TRY
  if (e->samp_count != nullptr) return 0;
  const size_t v = (size_t)e->cfg.vocab;
  char* buf = nullptr;  // [counts v][bias v][adj v][ids 1024][vals 1024][controls]
  WOQ_HIP(hipMalloc((void**)&buf, (3 * v + 2048) * 4 + sizeof(woq_sampler_controls)));
  WOQ_HIP(hipMemset(buf, 0, (3 * v + 2048) * 4 + sizeof(woq_sampler_controls)));
  WOQ_HIP(hipMemset(buf + v * 4, 0xFF, v * 4));  // no bias entries
  e->owned.push_back(buf);
  e->samp_count = (uint32_t*)buf;
  e->samp_bias = (float*)(buf + v * 4);
  e->samp_adj = (float*)(buf + 2 * v * 4);
  e->samp_bias_ids = (int32_t*)(buf + 3 * v * 4);
  e->samp_bias_vals = (float*)(buf + (3 * v + 1024) * 4);
  e->samp_ctl = (woq_sampler_controls*)(buf + (3 * v + 2048) * 4);
  WOQ_END
}

// neutral controls into the (allocated) controls' memory: what the guided tail reads when only a guide is installed
static int engine_controls_neutral(woq_engine* e) {
  WOQ_TRY
  WOQ_HIP(hipDeviceSynchronize());
  WOQ_HIP(hipMemset(e->samp_bias, 0xFF, (size_t)e->cfg.vocab * 4));  // no bias entries
  WOQ_HIP(hipMemset(e->samp_ctl, 0, sizeof(woq_sampler_controls)));
  e->samp_ctl_host = woq_sampler_controls{};
  WOQ_HIP(hipDeviceSynchronize());
  WOQ_END
}

int woq_engine_set_sampler_controls(woq_engine* e, const woq_sampler_controls* ctl, const int32_t* bias_ids_host,
                                    const float* bias_vals_host) {
  WOQ_TRY
  WOQ_CHECK(e, "QBits: null engine");
  const TailKey before = e->tail_key();
  if (ctl != nullptr) {
    WOQ_CHECK(e->whole_vocab(),
              "QBits: the native sampler needs the whole vocabulary on one GPU (a tensor-parallel head is vocab-sharded)");
    WOQ_CHECK(e->sampler_on, "QBits: sampler controls need a sampler installed (woq_engine_set_sampler first)");
    const char* why = sampler_controls_problem(*ctl, e->samp_cfg_host, e->cfg.vocab, bias_ids_host, bias_vals_host);
    if (why) return woq::fail(why);
    if (engine_controls_alloc(e) != 0) return 1;
    WOQ_HIP(hipDeviceSynchronize());  // steps in flight on any stream still read the struct and the table
    if (ctl->n_bias > 0) {
      WOQ_HIP(hipMemcpy(e->samp_bias_ids, bias_ids_host, (size_t)ctl->n_bias * 4, hipMemcpyHostToDevice));
      WOQ_HIP(hipMemcpy(e->samp_bias_vals, bias_vals_host, (size_t)ctl->n_bias * 4, hipMemcpyHostToDevice));
    }
    if (launch_sampler_bias_store(e->samp_bias, e->cfg.vocab, e->samp_bias_ids, e->samp_bias_vals, ctl->n_bias, nullptr) != 0)
      return 1;
    WOQ_HIP(hipMemcpy(e->samp_ctl, ctl, sizeof(woq_sampler_controls), hipMemcpyHostToDevice));
    e->samp_ctl_host = *ctl;
    WOQ_HIP(hipDeviceSynchronize());
  } else if (e->guide_on && e->controls_on) {
    if (engine_controls_neutral(e) != 0) return 1;  // the guided tail goes on reading them
  }
  e->controls_on = ctl != nullptr;
  engine_tail_changed(e, before);
  WOQ_END
}

int woq_engine_set_guide(woq_engine* e, const void* table_dev, int n_states, int start_state) {
  WOQ_TRY
  WOQ_CHECK(e, "QBits: null engine");
  const TailKey before = e->tail_key();
  if (table_dev == nullptr) {  // the table stays allocated for the next guide
    e->guide_on = false;
    engine_tail_changed(e, before);
    return 0;
  }
  WOQ_CHECK(e->whole_vocab(),
            "QBits: a token guide needs the whole vocabulary on one GPU (a tensor-parallel head is vocab-sharded)");
  WOQ_CHECK(e->sampler_on, "QBits: a token guide needs a sampler installed (woq_engine_set_sampler first)");
  const char* why = guide_problem(n_states, start_state);
  if (why) return woq::fail(why);
  if (engine_controls_alloc(e) != 0) return 1;
  WOQ_HIP(hipDeviceSynchronize());  // steps in flight on any stream still read the struct and the table
  if (!e->controls_on && engine_controls_neutral(e) != 0) return 1;
  if (e->guide == nullptr) {
    WOQ_HIP(hipMalloc((void**)&e->guide, sizeof(GuideState)));
    e->owned.push_back(e->guide);
  }
  const size_t bytes = (size_t)n_states * (size_t)e->cfg.vocab * sizeof(uint16_t);
  uint16_t* retired = nullptr;
  if (bytes > e->guide_cap) {  // a failed allocation leaves the installed guide as it is
    uint16_t* grown = nullptr;
    WOQ_HIP(hipMalloc((void**)&grown, bytes));
    retired = e->guide_table;
    e->guide_table = grown, e->guide_cap = bytes;
  }
  WOQ_HIP(hipMemcpy(e->guide_table, table_dev, bytes, hipMemcpyDeviceToDevice));
  e->guide_host = GuideState{e->guide_table, n_states, start_state};
  WOQ_HIP(hipMemcpy(e->guide, &e->guide_host, sizeof(GuideState), hipMemcpyHostToDevice));
  WOQ_HIP(hipDeviceSynchronize());
  if (retired) hipFree(retired);  // the device struct names the new table by now
  e->guide_on = true;
  engine_tail_changed(e, before);
  WOQ_END
}

int woq_engine_guide_reset(woq_engine* e, int state, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e && e->guide_on, "QBits: no token guide installed");
  WOQ_CHECK(state >= 0 && state < e->guide_host.n_states, "QBits: the token guide's state is outside its table");
  launch_guide_state_store(e->guide, state, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

void* woq_engine_guide_state_ptr(woq_engine* e) { return e && e->guide ? &e->guide->state : nullptr; }

int woq_engine_sampler_counts(woq_engine* e, const int32_t* tokens_dev, int n, int clear, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e && n >= 0 && (tokens_dev != nullptr || n == 0), "QBits: bad sampler count arguments");
  if (engine_controls_alloc(e) != 0) return 1;
  if (clear) WOQ_HIP(hipMemsetAsync(e->samp_count, 0, (size_t)e->cfg.vocab * 4, (hipStream_t)stream));
  launch_sampler_counts(e->samp_count, e->cfg.vocab, tokens_dev, n, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

void* woq_engine_sampler_count_ptr(woq_engine* e) {
  return e && engine_controls_alloc(e) == 0 ? e->samp_count : nullptr;
}

int woq_engine_sampler_seen(woq_engine* e, const int32_t* tokens_dev, int n, int clear, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e && n >= 0 && (tokens_dev != nullptr || n == 0), "QBits: bad sampler history arguments");
  if (clear) WOQ_HIP(hipMemsetAsync(e->samp_seen, 0, (size_t)e->seen_words() * 4, (hipStream_t)stream));
  launch_sampler_seen(e->samp_seen, e->cfg.vocab, tokens_dev, n, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

void* woq_engine_sampler_seen_ptr(woq_engine* e) { return e ? e->samp_seen : nullptr; }

int woq_engine_set_logprobs(woq_engine* e, int on) {
  WOQ_TRY
  WOQ_CHECK(e, "QBits: null engine");
  const TailKey before = e->tail_key();
  if (on != 0) {
    WOQ_CHECK(e->whole_vocab(),
              "QBits: log-probabilities need the whole vocabulary on one GPU (a tensor-parallel head is vocab-sharded)");
    WOQ_CHECK(logprob_vocab_ok(e->cfg.vocab), "QBits: the log-probability record covers vocabularies of up to 418816 ids");
    if (e->lp_chosen == nullptr) {
      const size_t rows = (size_t)e->cfg.max_ctx + 1;
      void *a = nullptr, *b = nullptr, *c = nullptr, *w = nullptr;
      WOQ_HIP(hipMalloc(&a, rows * 4));
      e->owned.push_back(a);
      WOQ_HIP(hipMalloc(&b, rows * 20 * 4));
      e->owned.push_back(b);
      WOQ_HIP(hipMalloc(&c, rows * 20 * 4));
      e->owned.push_back(c);
      WOQ_HIP(hipMalloc(&w, logprob_workspace_bytes(e->cfg.vocab)));
      e->owned.push_back(w);
      WOQ_HIP(hipMemset(a, 0, rows * 4));
      WOQ_HIP(hipMemset(b, 0, rows * 20 * 4));
      WOQ_HIP(hipMemset(c, 0, rows * 20 * 4));
      e->lp_top_id = (int32_t*)b, e->lp_top_lp = (float*)c, e->lp_ws = w;
      e->lp_chosen = (float*)a;  // last: what woq_engine_logprob_ptr and the steps test
    }
  }
  e->logprobs_on = on != 0;
  engine_tail_changed(e, before);
  WOQ_END
}

int woq_engine_logprobs(woq_engine* e) { return e && e->logprobs_on ? 1 : 0; }

void* woq_engine_logprob_ptr(woq_engine* e, int which) {
  if (!e || e->lp_chosen == nullptr) return nullptr;
  return which == 0 ? (void*)e->lp_chosen : which == 1 ? (void*)e->lp_top_id : which == 2 ? (void*)e->lp_top_lp : nullptr;
}

int woq_engine_step(woq_engine* e, int greedy, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e && e->embed && e->lm_head, "QBits: engine head not set");
  WOQ_CHECK_LAYERS(e);
  int rc = engine_step_impl(e, greedy, (hipStream_t)stream);
  if (rc) return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

int woq_engine_phase(woq_engine* e, int layer, int phase, int greedy, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e && e->embed && e->lm_head, "QBits: engine head not set");
  WOQ_CHECK_LAYERS(e);
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  if (phase == 0) {
    WOQ_CHECK(layer >= 0 && layer < e->cfg.layers, "QBits: bad layer index");
    if (layer == 0) engine_embed(e, st);
    rc = engine_attn_block(e, layer, st);
  } else if (phase == 1) {
    WOQ_CHECK(layer >= 0 && layer < e->cfg.layers, "QBits: bad layer index");
    rc = engine_mlp_block(e, layer, st);
  } else {
    rc = engine_head(e, greedy, st);
  }
  if (rc) return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

int woq_engine_capture(woq_engine* e, int greedy, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e && e->embed && e->lm_head, "QBits: engine head not set");
  WOQ_CHECK_LAYERS(e);
  WOQ_CHECK(!e->allreduce || (e->comm && e->cfg.tp_size > 1),
            "QBits: graph capture with a host all-reduce callback is not supported (bind a device communicator)");
  hipStream_t st = (hipStream_t)stream;
  if (e->attn_cnt) WOQ_HIP(hipMemsetAsync(e->attn_cnt, 0, (size_t)e->cfg.heads * 4, st));
  // one eager, non-advancing step first: sets the lazy kernel attributes outside of capture.
  // (re-writing the KV slot at the current position is idempotent)
  int rc = engine_step_impl(e, 0, st);
  if (rc) return rc;
  WOQ_HIP(hipStreamSynchronize(st));
  engine_drop_graphs(e);
  WOQ_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  rc = engine_step_impl(e, greedy, st);
  hipError_t ce = hipStreamEndCapture(st, &e->graph);
  if (rc) return rc;
  WOQ_HIP(ce);
  WOQ_HIP(hipGraphInstantiate(&e->exec, e->graph, nullptr, nullptr, 0));
  // k chained steps as one graph — greedy chains only (a non-greedy step leaves the next token to the host) and never
  // with a host-side all-reduce callback in the step
  if (greedy) {
    WOQ_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    // interior token boundaries of the chain: argmax + next embedding in one launch
    const bool fuse = engine_can_fuse_next(e, greedy);
    for (int i = 0; i < e->graph_unroll && rc == 0; ++i)
      rc = engine_step_impl(e, greedy, st, fuse ? ((i > 0 ? 1 : 0) | (i + 1 < e->graph_unroll ? 2 : 0)) : 0);
    ce = hipStreamEndCapture(st, &e->graph_k);
    if (rc) return rc;
    WOQ_HIP(ce);
    WOQ_HIP(hipGraphInstantiate(&e->exec_k, e->graph_k, nullptr, nullptr, 0));
  }
  WOQ_END
}

// n decode steps issued eagerly, back to back, no graph: the greedy token / position chain on the device exactly as in
// a replayed graph, and the host stays ahead of the GPU (~131 launches of ~2.6 us host time against ~1 ms of device
// time per 7B token). Same device time as hipGraphLaunch of the captured step on the same stream (1.04 ms per
// Llama-2-7B token either way, profiles/r04ab_stream_mode_probe.txt); what made graph replays 12 % slower through
// round 3 was the stream they were launched on (behind cross-stream event waits), not the graph.
int woq_engine_steps(woq_engine* e, int n, int greedy, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e && e->embed && e->lm_head, "QBits: engine head not set");
  WOQ_CHECK_LAYERS(e);
  for (int i = 0; i < n; ++i) {
    const int rc = engine_step_impl(e, greedy, (hipStream_t)stream);
    if (rc) return rc;
  }
  WOQ_END
}

int woq_engine_replay(woq_engine* e, int n, void* stream) {
  WOQ_TRY
  WOQ_CHECK(e && e->exec, "QBits: engine graph not captured");
  int left = n;
  if (e->exec_k)
    for (; left >= e->graph_unroll; left -= e->graph_unroll) WOQ_HIP(hipGraphLaunch(e->exec_k, (hipStream_t)stream));
  for (; left > 0; --left) WOQ_HIP(hipGraphLaunch(e->exec, (hipStream_t)stream));
  WOQ_END
}

// mask: which of the layer's projections a pass launches (bit 0 qkv, 1 o, 2 gate/up, 3 down); bytes and launch count
// are those of the selected ones
int woq_engine_time_gemv_mask(woq_engine* e, int mask, int reps, void* stream, float* total_ms, double* bytes_per_pass,
                              int* launches_per_pass) {
  WOQ_TRY
  WOQ_CHECK(e && total_ms && bytes_per_pass && launches_per_pass && (mask & 15) != 0, "QBits: bad argument");
  WOQ_CHECK_LAYERS(e);
  hipStream_t st = (hipStream_t)stream;
  const woq_engine_config& c = e->cfg;
  double bytes = 0;
  for (const EngineLayer& w : e->layers) {
    for (int k = 0; k < P_COUNT; ++k) {
      if (!((mask >> k) & 1)) continue;
      const woq_blob_header& h = w.p[k].hdr;
      // algorithmic bytes: int4 payload + scales (+ zero points), unpadded
      bytes += (double)h.K * h.N * 0.5 + (double)h.n_groups * h.N * (h.scale_type == WOQ_F32 ? 4 : 2) +
               (h.off_zp ? (double)h.n_groups * h.N * 0.5 : 0.0);
    }
  }
  auto pass = [&](hipStream_t st) -> int {
    for (int l = 0; l < c.layers; ++l) {
      const EngineLayer& w = e->layers[l];
      const EngineProj &qkv = w.p[P_QKV], &o = w.p[P_O], &gu = w.p[P_GATE_UP], &down = w.p[P_DOWN];
      int rc;
      if (e->use_xq()) {  // the step's own four GEMV launches: same kernels, epilogues, XQ outputs, residual chaining
        const bool last = l + 1 == c.layers;
        if ((mask & 1) && (rc = engine_gemv_xq_base(e, l, P_QKV, e->xq_hidden, e->qkv, e->ssq_part, nullptr, kNoXq, nullptr,
                                               nullptr, st)) != 0)
          return rc;
        if ((mask & 2) && (rc = engine_gemv_xq_base(e, l, P_O, e->xq_attn, e->hidden, nullptr, e->hidden, e->xq_hidden, w.ln2,
                                               e->ssq_part, st)) != 0)
          return rc;
        if ((mask & 4) && (rc = engine_gemv_xq_base(e, l, P_GATE_UP, e->xq_hidden, nullptr, e->ssq_part, nullptr, e->xq_act,
                                               nullptr, nullptr, st)) != 0)
          return rc;
        if ((mask & 8) && (rc = engine_gemv_xq_base(e, l, P_DOWN, e->xq_act, e->hidden, nullptr, e->hidden,
                                               last ? kNoXq : e->xq_hidden, last ? nullptr : e->layers[l + 1].ln1,
                                               last ? nullptr : e->ssq_part, st)) != 0)
          return rc;
        continue;
      }
      rc = (mask & 1) ? launch_gemv_from_header(e->hidden, WOQ_F32, c.hidden, qkv.blob, qkv.hdr, nullptr, e->qkv,
                                                WOQ_F32, qkv.hdr.N, 1, w.ln1, c.rms_eps, nullptr, 0, 0, st)
                      : 0;
      if (rc) return rc;
      rc = (mask & 2) ? launch_gemv_from_header(e->attn, WOQ_F32, c.heads * c.head_dim, o.blob, o.hdr, nullptr,
                                                e->qkv, WOQ_F32, c.hidden, 1, nullptr, 0.f, nullptr, 0, 0, st)
                      : 0;
      if (rc) return rc;
      rc = (mask & 4) ? launch_gemv_from_header(e->hidden, WOQ_F32, c.hidden, gu.blob, gu.hdr, nullptr,
                                                e->act, WOQ_F32, c.inter, 1, w.ln2, c.rms_eps, nullptr, 0, 1, st)
                      : 0;
      if (rc) return rc;
      rc = (mask & 8) ? launch_gemv_from_header(e->act, WOQ_F32, c.inter, down.blob, down.hdr, nullptr, e->qkv,
                                                WOQ_F32, c.hidden, 1, nullptr, 0.f, nullptr, 0, 0, st)
                      : 0;
      if (rc) return rc;
    }
    return 0;
  };
  const int rc = time_captured(st, reps, pass, total_ms, e->time_eager);
  if (rc) return rc;
  *bytes_per_pass = bytes;
  *launches_per_pass = c.layers * __builtin_popcount(mask & 15);
  WOQ_END
}
int woq_engine_time_gemv(woq_engine* e, int reps, void* stream, float* total_ms, double* bytes_per_pass,
                         int* launches_per_pass) {
  return woq_engine_time_gemv_mask(e, 15, reps, stream, total_ms, bytes_per_pass, launches_per_pass);
}

// roofline.ceiling of bench.py: the decode step's four GEMV launches per layer with the arithmetic taken out — mode 0:
// load-only twins (same grids, waves, K slices, non-temporal requests over the engine's own blobs), mode 1: empty
// kernels on the same grids — timed like woq_engine_time_gemv (one event pair around each pass, back to back).
int woq_engine_time_twin(woq_engine* e, int mode, int reps, void* stream, float* total_ms) {
  WOQ_TRY
  WOQ_CHECK(e && total_ms && (mode == 0 || mode == 1), "QBits: bad argument");
  WOQ_CHECK_LAYERS(e);
  hipStream_t st = (hipStream_t)stream;
  unsigned int* sink = (unsigned int*)e->am_idx;  // any device word; never written (the twins' store is unreachable)
  auto pass = [&](hipStream_t st) -> int {
    for (const EngineLayer& w : e->layers)
      for (int k = 0; k < P_COUNT; ++k) {
        const int rc = launch_gemv_twin(w.p[k].blob, w.p[k].hdr, kProjEpi[k], mode, sink, st);
        if (rc) return rc;
      }
    return 0;
  };
  // empty kernels are shorter than the host's launch call (~2.6 us): issued eagerly the pass would be host-bound and
  // read the host's rate, not the device's — always a replayed graph for mode 1
  const int rc = time_captured(st, reps, pass, total_ms, mode == 1 ? false : e->time_eager);
  if (rc) return rc;
  WOQ_END
}

// The prompt pass's dominant GEMM in place: the engine's own gate/up call of `layer` over n_seq * T rows (RMSNorm pack
// pass + MFMA GEMM with the SiLU * mul epilogue into the fp16 activation buffer), `reps` times; gemm_ms = the GEMM
// kernel alone (events right around its launch), call_ms = pack pass + GEMM. The residual stream must hold a prompt
// pass's rows (call woq_engine_prefill with the same n_seq * T first).
int woq_engine_time_prefill_gemm(woq_engine* e, int layer, int n_rows, int reps, void* stream, float* gemm_ms,
                                 float* call_ms) {
  WOQ_TRY
  WOQ_CHECK(e && gemm_ms && call_ms && layer >= 0 && layer < e->cfg.layers && reps >= 1, "QBits: bad argument");
  WOQ_CHECK((size_t)n_rows <= e->pf_rows && n_rows > 8, "QBits: run a prompt pass of at least n_rows rows first");
  WOQ_CHECK_LAYERS(e);
  hipStream_t st = (hipStream_t)stream;
  const woq_engine_config& c = e->cfg;
  hipEvent_t k0, k1, c0, c1;
  WOQ_HIP(hipEventCreate(&k0));
  WOQ_HIP(hipEventCreate(&k1));
  WOQ_HIP(hipEventCreate(&c0));
  WOQ_HIP(hipEventCreate(&c1));
  std::vector<std::pair<float, float>> samples;  // (kernel, call) per timed pass
  for (int r = 0; r <= reps; ++r) {  // pass 0 warms up
    WOQ_HIP(hipEventRecord(c0, st));
    set_gemm_time_events(k0, k1);
    const int rc = engine_prefill_gemm(e, layer, P_GATE_UP, n_rows, e->pf_h, WOQ_F32, c.hidden, e->pf_act, WOQ_F16,
                                       c.inter, e->layers[layer].ln2, st);
    set_gemm_time_events(nullptr, nullptr);
    if (rc) return rc;
    WOQ_HIP(hipEventRecord(c1, st));
    WOQ_HIP(hipStreamSynchronize(st));
    float tk = 0.f, tc = 0.f;
    WOQ_HIP(hipEventElapsedTime(&tk, k0, k1));
    WOQ_HIP(hipEventElapsedTime(&tc, c0, c1));
    if (r > 0) samples.emplace_back(tk, tc);
  }
  for (hipEvent_t ev : {k0, k1, c0, c1}) hipEventDestroy(ev);
  // the MEDIAN pass: one visit of the round caught a single 6 ms pass among ~1.1 ms ones (a box hiccup; the rerun was
  // clean) and the mean of three reported 0.10 of peak for a 0.54 kernel
  std::sort(samples.begin(), samples.end());
  *gemm_ms = samples[samples.size() / 2].first;
  *call_ms = samples[samples.size() / 2].second;
  WOQ_END
}

}  // extern "C"
