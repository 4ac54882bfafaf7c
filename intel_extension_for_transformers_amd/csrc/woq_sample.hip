// woq_sample.hip — the next-token choice of a decode step with a sampler installed: Hugging Face's repetition penalty,
// temperature, top-k, top-p and the draw, in HF's order (runtime/engine.py DeviceSampler.processed is the torch
// restatement), as ONE launch after the lm_head in place of the greedy argmax. One workgroup of 1024 threads; the launch
// shape does not depend on data and every parameter is read from a device struct, so the step stays capturable and a
// change of temperature / k / p / penalty / seed needs no new capture.
//
// Numerics. score = logit, for ids in the history bit set `s < 0 ? s * pen : s / pen`, then `/ T` when sampling: IEEE
// fp32 operations (no fast-math), the same two torch applies — the kept set is pure comparisons of these values.
//  - no sampling: argmax of the scores, lowest id on ties;
//  - 1 <= top_k <= 1024: radix select (4 x 8 bits over an order-preserving uint32 key) of the k-th largest score, every
//    score >= it is a candidate (ties at the k-th value survive, as in HF's `scores < kth` mask), candidates sorted by
//    (score descending, id ascending), w_i = expf(s_i - s_0), inclusive sums c_i, nucleus cut on the tail mass
//    Z - c_(i-1) <= (1 - top_p) * Z (never the first), draw = first kept i with c_i > u * Z';
//  - top_k = 0 (top_p = 1): softmax over the whole vocabulary, the same inverse-CDF rule over ids in ascending order.
// u = (x0 >> 8) * 2^-24, x0 = word 0 of Philox4x32-10 with counter (position + discarded, 0, 0, 0) and key (seed_lo,
// seed_hi); `discarded` = the positions a rolling KV cache has dropped (woq_engine_kv_shift; 0 otherwise), so the counter
// is the token's absolute index in the stream and a draw depends on (seed, absolute position, logits) only: eager steps
// and graphs of any burst size give the same tokens, and no u comes round again after a shift.
//
// Sampler controls (woq_sampler_controls: logit bias, presence / frequency penalty, min_p). With them installed a pre-pass
// over the whole chip (score_adjust_kernel<false>, one id per thread) writes, for every id, the fp32 score
//   s = l; s = s + b[i] (ids with a bias entry); repetition penalty as above; for ids generated c[i] > 0 times
//   s = s - (freq * (float)c[i]); s = s - pres
// — every operation rounded on its own (compiled with fp contraction off: no fma) — into an engine-owned
// scratch, and the sampling workgroup runs over that scratch with its own penalty step off (sample_kernel<true>): its six
// walks over the vocabulary stay one load per visit. A dense bias table holds NaN where an id has no entry (a bias is
// never NaN), so `-0.0` stays `-0.0` there. min_p (HF MinPLogitsWarper after top-k / top-p): a candidate stays iff
// w_i = expf(s_i - s_0) >= min_p; in the whole-vocabulary walk a weight below min_p counts as 0. The finishing thread
// also counts its pick in c. The logits themselves are never modified (the log-probability record reads them).
//
// Token guide (woq_host.h GuideState: a dense uint16 table next[n_states][vocab] and a state, both on the device). With
// one installed the pre-pass is score_adjust_kernel<true>: the four steps above, then step 5, `s = -inf` where the
// state's row holds 0xFFFF. After the sampling launch a one-thread launch (guide_advance_kernel) moves the state to
// row[token]. Pointer and state are read from the struct: another guide, or a reset, needs no new capture.
// One launcher, launch_sample_tail, issues all three forms: the buffers set in its SampleTail (woq_host.h) decide.
#include <algorithm>
#include <vector>

#include "woq_device.h"
#include "woq_host.h"
#include "woq_score_key.h"
#include "../../include/woq_hip_experimental.h"

namespace woq {
namespace {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int SAMPLE_MAX_CAND = 1024;
constexpr int SAMPLER_MAX_BIAS = 1024;

struct ScoreArgs {
  const float* logits;
  const uint32_t* seen;
  float pen, temp;
  bool use_pen, scale;
};
__device__ __forceinline__ float score_at(const ScoreArgs& a, int i) {
  float s = a.logits[i];
  if (a.use_pen && ((a.seen[i >> 5] >> (i & 31)) & 1u)) s = s < 0.f ? s * a.pen : s / a.pen;
  if (a.scale) s = s / a.temp;
  return s;
}

// Philox4x32-10 (Salmon et al., Random123): word 0..3 of counter (c0, 0, 0, 0) under key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1, uint32_t out[4]) {
  uint32_t c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__device__ __forceinline__ float wave_scan_f32(float v, int lane) {  // inclusive, lane order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ unsigned int wave_scan_u32(unsigned int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// hist[bin] += 1 for every active lane, one LDS atomic per distinct bin of the wave: the top byte of a logit's key
// takes a handful of values, and 64 lanes on one LDS address would serialise. Called by whole waves.
__device__ __forceinline__ void wave_hist_add(unsigned int* hist, bool active, uint32_t bin, int lane) {
  unsigned long long todo = __ballot(active);
  while (todo != 0ull) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t b = __shfl(bin, leader, 64);
    const unsigned long long same = __ballot(active && bin == b);
    if (lane == leader) atomicAdd(&hist[b], (unsigned int)__popcll(same));
    todo &= ~same;
  }
}

// max over the workgroup of (key << 32 | ~id): the largest score, lowest id on ties. Every thread gets the result.
__device__ __forceinline__ unsigned long long block_best(const ScoreArgs& a, int vocab, unsigned long long* red, int tid) {
  unsigned long long best = 0ull;
  for (int i = tid; i < vocab; i += SAMPLE_THREADS) {
    const unsigned long long v = ((unsigned long long)score_key(score_at(a, i)) << 32) | (uint32_t)(~i);
    best = v > best ? v : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(best, o, 64);
    best = t > best ? t : best;
  }
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  best = red[0];
#pragma unroll
  for (int w = 1; w < SAMPLE_WAVES; ++w) best = red[w] > best ? red[w] : best;
  __syncthreads();
  return best;
}

// `advance` != 0: the engine's chain — log[pos] = token, pos += 1 (the next step's embedding kernel guards max_ctx)
// CTL (sampler controls): `logits` is the pre-pass's adjusted-score scratch (no penalty step here), min_p comes from
// `ctlp`, the pick is counted in `counts` and kept_out (nullable; the probe's) receives how many ids a sampled draw
// was over; without CTL all three are unused and the kernel is the one it always was
template <bool CTL>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(
    const float* __restrict__ logits, int vocab, uint32_t* __restrict__ seen, const woq_sampler_config* __restrict__ cfgp,
    const float* __restrict__ u_in, int32_t* __restrict__ token, int32_t* __restrict__ pos_io,
    const int32_t* __restrict__ pos_ro, int32_t* __restrict__ log, uint32_t* __restrict__ philox_out,
    int* __restrict__ status, const woq_sampler_controls* __restrict__ ctlp, uint32_t* __restrict__ counts,
    uint32_t* __restrict__ kept_out, const int32_t* __restrict__ discarded) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned long long cand[SAMPLE_MAX_CAND];
  __shared__ float cdf[SAMPLE_MAX_CAND];
  __shared__ unsigned long long red[SAMPLE_WAVES];
  __shared__ float wsum[SAMPLE_WAVES];
  __shared__ unsigned int wcnt[SAMPLE_WAVES];
  __shared__ unsigned int sel[4];   // radix select: prefix, rank wanted inside it, keys above it, keys equal (last pass)
  __shared__ unsigned int slot[4];  // compaction counters (front, ties), first dropped index, picked index

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const woq_sampler_config cfg = *cfgp;
  const bool do_sample = cfg.do_sample != 0;
  ScoreArgs sa;
  sa.logits = logits, sa.seen = seen, sa.pen = cfg.repetition_penalty, sa.temp = cfg.temperature;
  sa.use_pen = !CTL && cfg.repetition_penalty != 1.0f, sa.scale = do_sample;
  float min_p = 0.f;
  if constexpr (CTL) min_p = ctlp->min_p;

  // what the finishing thread does with its pick (exactly one thread calls it; every read of `seen` lies before a
  // barrier that this thread has passed)
  auto finish = [&](int tok, int flags) {
    const int p = pos_io != nullptr ? pos_io[0] : (pos_ro != nullptr ? pos_ro[0] : 0);
    token[0] = tok;
    atomicOr(&seen[tok >> 5], 1u << (tok & 31));
    if constexpr (CTL) counts[tok] += 1u;
    if (log != nullptr) log[p] = tok;
    if (pos_io != nullptr) pos_io[0] = p + 1;
    if (flags != 0 && status != nullptr) atomicOr(status, flags);
  };

  float u = 0.f;
  if (do_sample) {  // every thread computes the same uniform (uniform control flow, scalar-friendly)
    const int p = pos_io != nullptr ? pos_io[0] : (pos_ro != nullptr ? pos_ro[0] : 0);
    uint32_t x[4];
    // the counter is the token's absolute index in the stream: the position fed plus what a rolling cache has dropped
    const uint32_t c0 = (uint32_t)p + (discarded != nullptr ? (uint32_t)discarded[0] : 0u);
    philox4x32_10(c0, cfg.seed_lo, cfg.seed_hi, x);
    if (tid == 0 && philox_out != nullptr) philox_out[0] = x[0], philox_out[1] = x[1], philox_out[2] = x[2], philox_out[3] = x[3];
    u = u_in != nullptr ? u_in[0] : (float)(x[0] >> 8) * 5.9604644775390625e-08f;
  }
  __syncthreads();  // the position was read by everyone before anyone advances it

  const unsigned long long best = block_best(sa, vocab, red, tid);
  const uint32_t best_key = (uint32_t)(best >> 32);
  if (best_key == 0u) {  // every score NaN: token 0 and a status bit, as the argmax kernels do
    if (tid == 0) finish(0, 4);
    return;
  }
  if (!do_sample) {
    if (tid == 0) finish((int)~(uint32_t)best, 0);
    return;
  }
  const float s_max = key_score(best_key);

  if (cfg.top_k <= 0) {
    // ---- whole vocabulary: wave w owns the ids [w * seg, (w + 1) * seg), walked 64 at a time in ascending order; the
    // running sum of a wave is built from the same scans in both passes, so the second pass ends on the first one's total
    const int seg = (((vocab + SAMPLE_WAVES - 1) / SAMPLE_WAVES) + 63) & ~63;
    const int w_lo = wid * seg < vocab ? wid * seg : vocab, w_hi = w_lo + seg < vocab ? w_lo + seg : vocab;
    auto weight = [&](int i) -> float {
      if (i >= w_hi) return 0.f;
      const float s = score_at(sa, i);
      const float wv = s != s ? 0.f : (s == s_max ? 1.f : expf(s - s_max));
      if constexpr (CTL) return wv >= min_p ? wv : 0.f;
      return wv;
    };
    float running = 0.f;
    unsigned int n_mass = 0u;
    for (int b = w_lo; b < w_hi; b += 64) {
      const float wv = weight(b + lane);
      if constexpr (CTL) n_mass += (unsigned int)__popcll(__ballot(wv > 0.f));
      running += __shfl(wave_scan_f32(wv, lane), 63, 64);
    }
    if (lane == 0) wsum[wid] = running;
    if constexpr (CTL)
      if (lane == 0) wcnt[wid] = n_mass;
    __syncthreads();
    if constexpr (CTL)
      if (tid == 0 && kept_out != nullptr) {
        unsigned int total = 0u;
        for (int w = 0; w < SAMPLE_WAVES; ++w) total += wcnt[w];
        kept_out[0] = total;
      }
    float z = 0.f;
    for (int w = 0; w < SAMPLE_WAVES; ++w) z += wsum[w];
    const float target = u * z;
    float base = 0.f, cum = 0.f;
    int wsel = -1, wlast = 0;
    for (int w = 0; w < SAMPLE_WAVES; ++w) {
      const float nxt = cum + wsum[w];
      if (wsum[w] > 0.f) wlast = w;
      if (wsel < 0 && nxt > target) wsel = w, base = cum;
      cum = nxt;
    }
    // rounding left no wave above the target: the last id with any mass (no lane of wave `wlast` then hits in the walk
    // below, because base + its sum <= target, and the walk ends on its last lane with mass)
    if (wsel < 0) {
      wsel = wlast, base = 0.f;
      for (int w = 0; w < wlast; ++w) base += wsum[w];
    }
    if (wid != wsel) return;
    int found = -1, last_mass = w_lo;
    running = 0.f;
    for (int b = w_lo; b < w_hi && found < 0; b += 64) {
      const float wv = weight(b + lane);
      const float sc = wave_scan_f32(wv, lane);
      const unsigned long long hit = __ballot(wv > 0.f && base + (running + sc) > target);
      const unsigned long long mass = __ballot(wv > 0.f);
      if (hit != 0ull) found = b + __ffsll((long long)hit) - 1;
      if (mass != 0ull) last_mass = b + 63 - __clzll((long long)mass);
      running += __shfl(sc, 63, 64);
    }
    if (lane == 0) finish(found >= 0 ? found : last_mass, 0);
    return;
  }

  // ---- top-k: radix select of the k-th largest key, most significant byte first -----------------------------------
  uint32_t prefix = 0u;
  unsigned int want = (unsigned int)(cfg.top_k < vocab ? cfg.top_k : vocab);
  want = want < (unsigned int)SAMPLE_MAX_CAND ? want : (unsigned int)SAMPLE_MAX_CAND;
  unsigned int n_greater = 0u, n_equal = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int base = 0; base < vocab; base += SAMPLE_THREADS) {  // whole waves, whatever the tail
      const int i = base + tid;
      bool act = false;
      uint32_t bin = 0u;
      if (i < vocab) {
        const uint32_t key = score_key(score_at(sa, i));
        act = pass == 0 ? true : ((key >> (shift + 8)) == prefix);
        bin = (key >> shift) & 255u;
      }
      wave_hist_add(hist, act, bin, lane);
    }
    __syncthreads();
    if (wid == 0) {  // lane L looks at bins 255 - 4L .. 252 - 4L: counts from the top down
      const unsigned int c0 = hist[255 - 4 * lane], c1 = hist[254 - 4 * lane], c2 = hist[253 - 4 * lane],
                         c3 = hist[252 - 4 * lane];
      const unsigned int mine = c0 + c1 + c2 + c3;
      const unsigned int incl = wave_scan_u32(mine, lane), excl = incl - mine;
      if (excl < want && want <= incl) {  // exactly one lane
        unsigned int above = excl, b = 255u - 4u * lane, c = c0;
        if (above + c < want) above += c, b -= 1u, c = c1;
        if (above + c < want) above += c, b -= 1u, c = c2;
        if (above + c < want) above += c, b -= 1u, c = c3;
        sel[0] = (prefix << 8) | b, sel[1] = want - above, sel[2] = n_greater + above, sel[3] = c;
      }
    }
    __syncthreads();
    prefix = sel[0], want = sel[1], n_greater = sel[2], n_equal = sel[3];
  }
  const uint32_t kth = prefix;
  if (kth == 0u) n_equal = 0u;  // fewer than k scores that are not NaN: those are the candidates, NaN never is
  const unsigned int room = (unsigned int)SAMPLE_MAX_CAND - n_greater;  // n_greater < k <= 1024
  const bool overflow = n_equal > room;  // more than 1024 survive the tie rule: the lowest ids among the tied, bit 8
  // ... unless the tie is at -inf under a finite best score (fewer than k finite scores): those weigh exactly 0
  const bool flag_overflow = overflow && !(kth == score_key(-INFINITY) && best_key != kth);
  const unsigned int n = n_greater + (overflow ? room : n_equal);

  // ---- candidates into LDS as (key << 32 | ~id), then a bitonic sort: score descending, id ascending ------------------
  cand[tid] = 0ull;
  if (tid < 4) slot[tid] = tid == 2 ? n : 0u;
  __syncthreads();
  for (int i = tid; i < vocab; i += SAMPLE_THREADS) {
    const uint32_t key = score_key(score_at(sa, i));
    const unsigned long long v = ((unsigned long long)key << 32) | (uint32_t)(~i);
    if (key > kth)
      cand[atomicAdd(&slot[0], 1u)] = v;
    else if (key == kth && kth != 0u && !overflow)
      cand[n_greater + atomicAdd(&slot[1], 1u)] = v;
  }
  if (overflow) {  // ties in id order, 1024 ids at a time, until the room is used up
    unsigned int placed = 0u;
    for (int base = 0; base < vocab && placed < room; base += SAMPLE_THREADS) {
      const int i = base + tid;
      const bool tie = i < vocab && score_key(score_at(sa, i)) == kth;
      const unsigned long long m = __ballot(tie);
      if (lane == 0) wcnt[wid] = (unsigned int)__popcll(m);
      __syncthreads();
      unsigned int before = 0u, total = 0u;
      for (int w = 0; w < SAMPLE_WAVES; ++w) before += w < wid ? wcnt[w] : 0u, total += wcnt[w];
      const unsigned int r = placed + before + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
      if (tie && r < room) cand[n_greater + r] = ((unsigned long long)kth << 32) | (uint32_t)(~i);
      placed += total;
      __syncthreads();
    }
  }
  __syncthreads();
  int P = 64;
  while (P < (int)n) P <<= 1;
  for (int k2 = 2; k2 <= P; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      if (tid < (P >> 1)) {
        const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), l = i | j;
        const unsigned long long a = cand[i], b = cand[l];
        if (((i & k2) == 0) ? (a < b) : (a > b)) cand[i] = b, cand[l] = a;
      }
      __syncthreads();
    }

  // ---- weights, inclusive sums, nucleus, draw ---------------------------------------------------------------------
  const float s0 = key_score((uint32_t)(cand[0] >> 32));
  float w = 0.f;
  if (tid < (int)n) {
    const float s = key_score((uint32_t)(cand[tid] >> 32));
    w = s == s0 ? 1.f : expf(s - s0);
  }
  float c = wave_scan_f32(w, lane);
  if (lane == 63) wsum[wid] = c;
  __syncthreads();
  float z = 0.f, off = 0.f;
  for (int ww = 0; ww < SAMPLE_WAVES; ++ww) {
    if (ww == wid) off = z;
    z += wsum[ww];
  }
  c += off;
  cdf[tid] = c;
  __syncthreads();
  if (cfg.top_p < 1.0f && tid >= 1 && tid < (int)n && z - cdf[tid - 1] <= (1.0f - cfg.top_p) * z) atomicMin(&slot[2], (unsigned int)tid);
  if constexpr (CTL)  // min_p: sorted candidates, so the kept ones are a prefix too (the first weighs exactly 1)
    if (tid >= 1 && tid < (int)n && !(w >= min_p)) atomicMin(&slot[2], (unsigned int)tid);
  __syncthreads();
  const unsigned int m = slot[2];  // kept: the first m candidates (m >= 1)
  if (tid == 0) slot[3] = m - 1u;
  if constexpr (CTL)
    if (tid == 0 && kept_out != nullptr) kept_out[0] = m;
  __syncthreads();
  const float target = u * cdf[m - 1u];
  if (tid < (int)m && w > 0.f && c > target) atomicMin(&slot[3], (unsigned int)tid);
  __syncthreads();
  if (tid == 0) finish((int)~(uint32_t)cand[slot[3]], flag_overflow ? 8 : 0);
}

__global__ void sampler_seen_kernel(uint32_t* __restrict__ seen, int vocab, const int32_t* __restrict__ tokens, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = tokens[i];
  if (t >= 0 && t < vocab) atomicOr(&seen[t >> 5], 1u << (t & 31));
}

// a host struct into device memory as a kernel argument: stream-ordered and capturable, whatever the host memory is
__global__ void sampler_config_store_kernel(woq_sampler_config v, woq_sampler_config* __restrict__ dst) { *dst = v; }
__global__ void sampler_controls_store_kernel(woq_sampler_controls v, woq_sampler_controls* __restrict__ dst) { *dst = v; }

constexpr int ADJUST_THREADS = 256;  // one id per thread: 125 .. 501 workgroups for 32000 .. 128256 ids, four loads each

// steps 1-4 of the controls' contract for every id (the header comment); `adj` is what sample_kernel<true> reads.
// GUIDED: then step 5, the ban of the guide's current row (`guide` is not read otherwise). The table pointer and the
// state come from the device struct, never from the launch: another guide or a reset keeps a captured graph valid.
template <bool GUIDED>
__global__ __launch_bounds__(ADJUST_THREADS) void score_adjust_kernel(
    const float* __restrict__ logits, int vocab, const uint32_t* __restrict__ seen, const uint32_t* __restrict__ counts,
    const float* __restrict__ bias, const woq_sampler_config* __restrict__ cfgp,
    const woq_sampler_controls* __restrict__ ctlp, const GuideState* __restrict__ guide, float* __restrict__ adj) {
// No contraction: `s - freq * c` must round twice. Plain operators under this pragma — HIP's __fmul_rn / __fsub_rn are
// inline functions over plain operators that carry their header's contract flag, and fuse into one fma once inlined.
#pragma clang fp contract(off)
  const int i = blockIdx.x * ADJUST_THREADS + threadIdx.x;
  if (i >= vocab) return;
  const float pen = cfgp->repetition_penalty, pres = ctlp->presence_penalty, freq = ctlp->frequency_penalty;
  const uint16_t* row = nullptr;
  if constexpr (GUIDED) row = guide->table + (size_t)guide->state * (size_t)vocab;  // 64-bit: 65535 states x 128256 ids
  float s = logits[i];
  const float b = bias[i];
  if (b == b) s = s + b;  // NaN = no entry
  if (pen != 1.0f && ((seen[i >> 5] >> (i & 31)) & 1u)) s = s < 0.f ? s * pen : s / pen;
  const uint32_t c = counts[i];
  if (c > 0u) {
    const float step = freq * (float)c;
    s = s - step;
    s = s - pres;
  }
  if constexpr (GUIDED)  // last: a positive penalty cannot lift -inf, so the order does not matter
    if (row[i] == GUIDE_BANNED) s = -INFINITY;
  adj[i] = s;
}

// after the pick: the guide's state follows the picked id. One thread; the sampler's token is always inside [0, vocab).
// A banned pick (only a state with every id banned, or a table that names a state it does not have, gets here) leaves
// the state where it is and raises status bit 4.
__global__ void guide_advance_kernel(GuideState* __restrict__ guide, int vocab, const int32_t* __restrict__ token,
                                     int* __restrict__ status) {
  const int32_t st = guide->state;
  const uint16_t nxt = guide->table[(size_t)st * (size_t)vocab + (size_t)token[0]];
  if (nxt != GUIDE_BANNED && (int32_t)nxt < guide->n_states)
    guide->state = (int32_t)nxt;
  else if (status != nullptr)
    atomicOr(status, 16);
}

__global__ void guide_state_store_kernel(GuideState* __restrict__ guide, int32_t state) { guide->state = state; }

__global__ void sampler_counts_kernel(uint32_t* __restrict__ counts, int vocab, const int32_t* __restrict__ tokens, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = tokens[i];
  if (t >= 0 && t < vocab) atomicAdd(&counts[t], 1u);
}

// bias[ids[j]] = vals[j] over a table that launch_sampler_bias_store has just filled with NaN (ids checked by the host)
__global__ void sampler_bias_scatter_kernel(float* __restrict__ bias, int vocab, const int32_t* __restrict__ ids,
                                            const float* __restrict__ vals, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int t = ids[j];
  if (t >= 0 && t < vocab) bias[t] = vals[j];
}

}  // namespace

int launch_sample_tail(const SampleTail& t, hipStream_t st) {
  const bool ctl = t.adj != nullptr;
  // a missing or misplaced slot fails here, not on the device (without `adj` the kernel then gets nulls for the rest)
  if ((t.counts != nullptr) != ctl || (t.bias != nullptr) != ctl || (t.ctl != nullptr) != ctl || (t.guide != nullptr && !ctl))
    return fail("QBits: a sampled pick takes the controls' four buffers or none of them, and a guide only with them");
  if (ctl)  // the pre-pass: logits -> adj
    hipLaunchKernelGGL(t.guide != nullptr ? score_adjust_kernel<true> : score_adjust_kernel<false>,
                       dim3((t.vocab + ADJUST_THREADS - 1) / ADJUST_THREADS), dim3(ADJUST_THREADS), 0, st, t.logits, t.vocab,
                       (const uint32_t*)t.seen, (const uint32_t*)t.counts, t.bias, t.cfg, t.ctl, t.guide, t.adj);
  hipLaunchKernelGGL(ctl ? sample_kernel<true> : sample_kernel<false>, dim3(1), dim3(SAMPLE_THREADS), 0, st,
                     ctl ? (const float*)t.adj : t.logits, t.vocab, t.seen, t.cfg, t.u, t.token, t.pos_advance, t.pos_fixed,
                     t.log, t.philox_out, t.status, t.ctl, t.counts, ctl ? t.kept_out : nullptr, t.discarded);
  return 0;
}

void launch_guide_advance(GuideState* guide_dev, int vocab, const int32_t* token, int* status, hipStream_t st) {
  hipLaunchKernelGGL(guide_advance_kernel, dim3(1), dim3(1), 0, st, guide_dev, vocab, token, status);
}

void launch_guide_state_store(GuideState* guide_dev, int32_t state, hipStream_t st) {
  hipLaunchKernelGGL(guide_state_store_kernel, dim3(1), dim3(1), 0, st, guide_dev, state);
}

const char* guide_problem(int n_states, int start_state) {
  if (n_states < 1 || n_states > 65535) return "QBits: a token guide has 1 to 65535 states";
  if (start_state < 0 || start_state >= n_states) return "QBits: the token guide's start state is outside its table";
  return nullptr;
}

void launch_sampler_counts(uint32_t* counts, int vocab, const int32_t* tokens, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(sampler_counts_kernel, dim3((n + 255) / 256), dim3(256), 0, st, counts, vocab, tokens, n);
}

int launch_sampler_bias_store(float* bias, int vocab, const int32_t* ids_dev, const float* vals_dev, int n, hipStream_t st) {
  WOQ_TRY
  WOQ_HIP(hipMemsetAsync(bias, 0xFF, (size_t)vocab * 4, st));  // 0xFFFFFFFF: a NaN, "no entry"
  if (n > 0)
    hipLaunchKernelGGL(sampler_bias_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, st, bias, vocab, ids_dev, vals_dev, n);
  WOQ_END
}

void launch_sampler_controls_store(const woq_sampler_controls& ctl, woq_sampler_controls* dst, hipStream_t st) {
  hipLaunchKernelGGL(sampler_controls_store_kernel, dim3(1), dim3(1), 0, st, ctl, dst);
}

void launch_sampler_seen(uint32_t* seen, int vocab, const int32_t* tokens, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(sampler_seen_kernel, dim3((n + 255) / 256), dim3(256), 0, st, seen, vocab, tokens, n);
}

void launch_sampler_config_store(const woq_sampler_config& cfg, woq_sampler_config* dst, hipStream_t st) {
  hipLaunchKernelGGL(sampler_config_store_kernel, dim3(1), dim3(1), 0, st, cfg, dst);
}

const char* sampler_config_problem(const woq_sampler_config& c) {
  if (!(c.repetition_penalty > 0.f)) return "QBits: repetition_penalty must be a positive float";
  if (c.do_sample == 0) return nullptr;
  if (!(c.temperature > 0.f) || c.temperature * 0.f != 0.f) return "QBits: temperature must be a positive finite float when sampling";
  if (!(c.top_p >= 0.f && c.top_p <= 1.f)) return "QBits: top_p must be in [0, 1]";
  if (c.top_k < 0 || c.top_k > SAMPLE_MAX_CAND)
    return "QBits: the native sampler takes top_k in [0, 1024] (larger values stay on the torch sampler)";
  if (c.top_k == 0 && c.top_p < 1.f)
    return "QBits: the native sampler takes top_k = 0 only with top_p = 1 (a nucleus over the whole vocabulary stays on "
           "the torch sampler)";
  return nullptr;
}

const char* sampler_controls_problem(const woq_sampler_controls& c, const woq_sampler_config& cfg, int vocab,
                                     const int32_t* ids, const float* vals) {
  if (c.presence_penalty * 0.f != 0.f || c.frequency_penalty * 0.f != 0.f)
    return "QBits: presence_penalty and frequency_penalty must be finite floats";
  if (!(c.min_p >= 0.f && c.min_p <= 1.f)) return "QBits: min_p must be in [0, 1]";
  if (c.min_p > 0.f && cfg.do_sample == 0) return "QBits: min_p needs do_sample (greedy decoding keeps one token anyway)";
  if (c.n_bias < 0 || c.n_bias > SAMPLER_MAX_BIAS) return "QBits: the native sampler takes at most 1024 logit_bias entries";
  if (c.n_bias > 0 && (ids == nullptr || vals == nullptr)) return "QBits: logit_bias entries without their arrays";
  std::vector<int32_t> sorted(ids, ids + c.n_bias);
  std::sort(sorted.begin(), sorted.end());
  for (int j = 0; j < c.n_bias; ++j) {
    if (sorted[j] < 0 || sorted[j] >= vocab) return "QBits: logit_bias token id outside the vocabulary";
    if (j > 0 && sorted[j] == sorted[j - 1]) return "QBits: duplicate logit_bias token id";
    if (vals[j] != vals[j] || vals[j] == INFINITY) return "QBits: a logit_bias value must be finite or -inf (a ban)";
  }
  return nullptr;
}

// What a probe's pick `t` needs on the device, one allocation on `st` (the caller frees `*out` on `st`): [config 32] and,
// with controls (`ctl` not null), [controls 32][guide state 32, not written here][bias table vocab * 4][ids n * 4]
// [values n * 4]. `t` (its vocab is read) leaves with the config and, with controls, their struct and table.
constexpr size_t PROBE_GUIDE_AT = 64;
static int probe_tail_setup(const woq_sampler_config& cfg, const woq_sampler_controls* ctl, const int32_t* bias_ids_host,
                            const float* bias_vals_host, hipStream_t st, SampleTail* t, char** out) {
  WOQ_TRY
  const int n = ctl != nullptr ? ctl->n_bias : 0;
  char* buf = nullptr;
  const size_t table = 96, ids_at = table + (size_t)t->vocab * 4, vals_at = ids_at + (size_t)n * 4;
  WOQ_HIP(hipMallocAsync((void**)&buf, ctl != nullptr ? vals_at + (size_t)n * 4 + 4 : sizeof(woq_sampler_config), st));
  if (n > 0) {  // the host arrays may go away when the probe returns: copies that have completed by then
    hipError_t err = hipMemcpyAsync(buf + ids_at, bias_ids_host, (size_t)n * 4, hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipMemcpyAsync(buf + vals_at, bias_vals_host, (size_t)n * 4, hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) {
      hipFreeAsync(buf, st);
      return fail(std::string("QBits: HIP error '") + hipGetErrorString(err) + "' copying the logit_bias entries");
    }
  }
  *out = buf;
  launch_sampler_config_store(cfg, (woq_sampler_config*)buf, st);
  t->cfg = (const woq_sampler_config*)buf;
  if (ctl == nullptr) return 0;
  launch_sampler_controls_store(*ctl, (woq_sampler_controls*)(buf + 32), st);
  t->ctl = (const woq_sampler_controls*)(buf + 32), t->bias = (const float*)(buf + table);
  if (launch_sampler_bias_store((float*)(buf + table), t->vocab, (const int32_t*)(buf + ids_at),
                                (const float*)(buf + vals_at), n, st) != 0) {
    hipFreeAsync(buf, st);
    return 1;
  }
  WOQ_END
}

}  // namespace woq

extern "C" {

static int probe_sample_impl(const float* logits, int vocab, uint32_t* seen, const woq_sampler_config* cfg,
                             const float* u_or_null, const int32_t* pos_dev, const int32_t* discarded_dev,
                             int32_t* token_out, uint32_t* philox_out4, int* status, void* stream) {
  WOQ_TRY
  WOQ_CHECK(logits && seen && cfg && pos_dev && token_out && vocab >= 1, "QBits: bad sampler probe arguments");
  const char* why = woq::sampler_config_problem(*cfg);
  if (why) return woq::fail(why);
  const hipStream_t st = (hipStream_t)stream;
  woq::SampleTail t;
  t.logits = logits, t.vocab = vocab, t.seen = seen, t.token = token_out, t.pos_fixed = pos_dev, t.status = status;
  t.u = u_or_null, t.philox_out = philox_out4, t.discarded = discarded_dev;
  char* buf = nullptr;
  int rc = woq::probe_tail_setup(*cfg, nullptr, nullptr, nullptr, st, &t, &buf);
  if (rc) return rc;
  rc = woq::launch_sample_tail(t, st);
  WOQ_HIP(hipFreeAsync(buf, st));
  if (rc) return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

WOQ_API int woq_probe_sample(const float* logits, int vocab, uint32_t* seen, const woq_sampler_config* cfg,
                             const float* u_or_null, const int32_t* pos_dev, int32_t* token_out, uint32_t* philox_out4,
                             int* status, void* stream) {
  return probe_sample_impl(logits, vocab, seen, cfg, u_or_null, pos_dev, nullptr, token_out, philox_out4, status, stream);
}

WOQ_API int woq_probe_sample_stream(const float* logits, int vocab, uint32_t* seen, const woq_sampler_config* cfg,
                                    const float* u_or_null, const int32_t* pos_dev, const int32_t* discarded_dev,
                                    int32_t* token_out, uint32_t* philox_out4, int* status, void* stream) {
  return probe_sample_impl(logits, vocab, seen, cfg, u_or_null, pos_dev, discarded_dev, token_out, philox_out4, status,
                           stream);
}

WOQ_API int woq_probe_sample_controls(const float* logits, int vocab, uint32_t* seen, uint32_t* counts,
                                      const woq_sampler_config* cfg, const woq_sampler_controls* ctl,
                                      const int32_t* bias_ids_host, const float* bias_vals_host, const float* u_or_null,
                                      const int32_t* pos_dev, int32_t* token_out, float* adjusted_out,
                                      uint32_t* kept_out, int* status, void* stream) {
  WOQ_TRY
  WOQ_CHECK(logits && seen && counts && cfg && ctl && pos_dev && token_out && adjusted_out && vocab >= 1,
            "QBits: bad sampler probe arguments");
  const char* why = woq::sampler_config_problem(*cfg);
  if (why == nullptr) why = woq::sampler_controls_problem(*ctl, *cfg, vocab, bias_ids_host, bias_vals_host);
  if (why) return woq::fail(why);
  const hipStream_t st = (hipStream_t)stream;
  woq::SampleTail t;
  t.logits = logits, t.vocab = vocab, t.seen = seen, t.token = token_out, t.pos_fixed = pos_dev, t.status = status;
  t.u = u_or_null, t.counts = counts, t.adj = adjusted_out, t.kept_out = kept_out;
  char* buf = nullptr;
  int rc = woq::probe_tail_setup(*cfg, ctl, bias_ids_host, bias_vals_host, st, &t, &buf);
  if (rc) return rc;
  rc = woq::launch_sample_tail(t, st);
  WOQ_HIP(hipFreeAsync(buf, st));
  if (rc) return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

WOQ_API int woq_probe_guide(const float* logits, int vocab, uint32_t* seen, uint32_t* counts,
                            const woq_sampler_config* cfg, const woq_sampler_controls* ctl,
                            const int32_t* bias_ids_host, const float* bias_vals_host, const uint16_t* table_dev,
                            int n_states, int state, int advance_state, const float* u_or_null, const int32_t* pos_dev,
                            int32_t* token_out, float* adjusted_out, int32_t* state_out, int* status, void* stream) {
  WOQ_TRY
  WOQ_CHECK(logits && seen && counts && cfg && ctl && table_dev && pos_dev && token_out && adjusted_out && state_out &&
                vocab >= 1,
            "QBits: bad guide probe arguments");
  const char* why = woq::sampler_config_problem(*cfg);
  if (why == nullptr) why = woq::sampler_controls_problem(*ctl, *cfg, vocab, bias_ids_host, bias_vals_host);
  if (why == nullptr) why = woq::guide_problem(n_states, state);
  if (why == nullptr && advance_state >= 0) why = woq::guide_problem(n_states, advance_state);
  if (why) return woq::fail(why);
  const hipStream_t st = (hipStream_t)stream;
  woq::SampleTail t;
  t.logits = logits, t.vocab = vocab, t.seen = seen, t.token = token_out, t.pos_fixed = pos_dev, t.status = status;
  t.u = u_or_null, t.counts = counts, t.adj = adjusted_out;
  char* buf = nullptr;
  int rc = woq::probe_tail_setup(*cfg, ctl, bias_ids_host, bias_vals_host, st, &t, &buf);
  if (rc) return rc;
  woq::GuideState* guide = (woq::GuideState*)(buf + woq::PROBE_GUIDE_AT);
  t.guide = guide;
  const woq::GuideState g = {table_dev, n_states, state};
  hipError_t err = hipMemcpyAsync(guide, &g, sizeof(g), hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);  // `g` goes away when this returns
  if (err == hipSuccess && (rc = woq::launch_sample_tail(t, st)) == 0) {
    if (advance_state >= 0) woq::launch_guide_state_store(guide, advance_state, st);
    woq::launch_guide_advance(guide, vocab, token_out, status, st);
    err = hipMemcpyAsync(state_out, &guide->state, 4, hipMemcpyDeviceToDevice, st);
  }
  hipFreeAsync(buf, st);
  if (rc) return rc;
  WOQ_HIP(err);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

}  // extern "C"
