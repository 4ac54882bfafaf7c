// woq_logprob.hip — the log-probability record of a chaining decode step (woq_engine_set_logprobs): what the raw model
// distribution, log_softmax over the fp32 lm_head logits before any penalty / temperature / top-k / top-p, says about
// the token the step picked and about its 20 best ids. Two launches after the pick (argmax pairs, argmax + embed, or the
// sampler), both of a shape fixed by `vocab` alone, so the step stays capturable:
//   1. logprob_partial_kernel, one workgroup of 256 threads per slice of 1024 ids: the slice's best key, its
//      sum of expf(s - slice max) and its 20 best (score_key << 32 | ~id) pairs;
//   2. logprob_merge_kernel, one workgroup of 1024 threads: the 20 best of the slices' candidates, M = the row maximum,
//      Z = sum over slices of sum_i * expf(max_i - M), logZ = M + logf(Z), then the record of row p = pos[0] - 1:
//      chosen[p] = logits[token[0]] - logZ, top_id[p][r], top_lp[p][r] = score_r - logZ.
// The kernel boundary is the hand-off between the two: no flags, counters or fences, nothing to reset between launches.
// Both kernels carry a row dimension (launch_logprob_rows: the scored prompt pass, woq_score.hip, records one row per
// prompt position from a [rows][vocab] logits scratch); the decode step's form is the same code with one row.
//
// Order. Pairs compare as (score descending, id ascending) under one unsigned 64-bit maximum; they are distinct, so
// round r of a selection is the largest pair below round r - 1's winner and nothing is ever removed. 0 stands for "no
// pair": NaN scores (key 0) and ids past the vocabulary. A list that runs out pads with id -1 / -inf.
// Numerics. Plain IEEE fp32, expf / logf. Every sum has one fixed shape, independent of which workgroup finishes first
// (tests/logprob_reference.py restates it): a thread adds its 4 ids in ascending order, a wave adds its lanes as an xor
// butterfly (32, 16, .. 1), the waves are added in ascending order; the merge does the same over slice index. A score
// equal to the maximum weighs exactly 1 (also when both are -inf or +inf), NaN weighs 0.
#include "woq_device.h"
#include "woq_host.h"
#include "woq_score_key.h"
#include "../../include/woq_hip_experimental.h"

namespace woq {
namespace {

constexpr int LP_TOP = 20;            // ids recorded per position (the OpenAI maximum)
constexpr int LP_SLICE = 1024;        // ids per workgroup of the first launch
constexpr int LP_THREADS = 256;
constexpr int LP_PER = LP_SLICE / LP_THREADS;
constexpr int LP_MERGE_THREADS = 1024;
constexpr int LP_MERGE_PER = 8;       // candidates a merge thread holds: n_slices * 20 <= 8 * 1024
constexpr int LP_MAX_SLICES = LP_MERGE_THREADS * LP_MERGE_PER / LP_TOP;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ float wave_sum_butterfly(float v) {  // every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the workgroup's largest `local`, in every thread. `red` holds two rows of WAVES words: round r uses row r & 1, so one
// barrier per round suffices (a wave can write row r & 1 again only after everyone has passed round r + 1's barrier)
template <int WAVES>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long local, unsigned long long* red, int round,
                                                            int tid) {
  unsigned long long* row = red + (round & 1) * WAVES;
  const unsigned long long v = wave_max_u64(local);
  if ((tid & 63) == 0) row[tid >> 6] = v;
  __syncthreads();
  unsigned long long best = row[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) best = row[w] > best ? row[w] : best;
  return best;
}

// the workgroup's sum of `v` in the fixed shape: butterfly inside a wave, waves in ascending order. Valid in thread 0.
template <int WAVES>
__device__ __forceinline__ float block_sum_ordered(float v, float* wsum, int tid) {
  v = wave_sum_butterfly(v);
  if ((tid & 63) == 0) wsum[tid >> 6] = v;
  __syncthreads();
  float z = wsum[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) z += wsum[w];
  return z;
}

// blockIdx.y = row: logits row `row` starts at logits + row * row_stride, its partials at index row * gridDim.x + slice
__global__ __launch_bounds__(LP_THREADS) void logprob_partial_kernel(const float* __restrict__ logits, size_t row_stride,
                                                                     int vocab, uint32_t* __restrict__ part_key,
                                                                     float* __restrict__ part_sum,
                                                                     unsigned long long* __restrict__ part_top) {
  constexpr int WAVES = LP_THREADS / 64;
  __shared__ unsigned long long red[2 * WAVES];
  __shared__ unsigned long long tops[LP_TOP];
  __shared__ float wsum[WAVES];
  const int tid = threadIdx.x, slice = blockIdx.x;
  const int base = slice * LP_SLICE;
  const size_t prow = (size_t)blockIdx.y * gridDim.x;
  logits += (size_t)blockIdx.y * row_stride;
  part_key += prow, part_sum += prow, part_top += prow * LP_TOP;
  float s[LP_PER];
  unsigned long long c[LP_PER];
#pragma unroll
  for (int j = 0; j < LP_PER; ++j) {
    const int i = base + j * LP_THREADS + tid;
    s[j] = 0.f, c[j] = 0ull;
    if (i < vocab) {
      s[j] = logits[i];
      const uint32_t key = score_key(s[j]);
      if (key != 0u) c[j] = ((unsigned long long)key << 32) | (uint32_t)(~i);
    }
  }
  if (tid < LP_TOP) tops[tid] = 0ull;
  unsigned long long prev = ~0ull;  // above every pair (the largest key, +inf's, is 0xFF800000)
  uint32_t m_key = 0u;
  for (int r = 0; r < LP_TOP; ++r) {
    unsigned long long local = 0ull;
#pragma unroll
    for (int j = 0; j < LP_PER; ++j) local = (c[j] < prev && c[j] > local) ? c[j] : local;
    const unsigned long long best = block_max_u64<WAVES>(local, red, r, tid);
    if (r == 0) {  // the slice maximum is known: the slice's sum, before the list goes on
      m_key = (uint32_t)(best >> 32);
      const float m = key_score(m_key);
      float w = 0.f;
#pragma unroll
      for (int j = 0; j < LP_PER; ++j)
        if (c[j] != 0ull) w += (uint32_t)(c[j] >> 32) == m_key ? 1.f : expf(s[j] - m);
      const float z = block_sum_ordered<WAVES>(w, wsum, tid);
      if (tid == 0) part_key[slice] = m_key, part_sum[slice] = z;
    }
    if (best == 0ull) break;  // the slice ran out (every thread sees the same `best`)
    if (tid == 0) tops[r] = best;
    prev = best;
  }
  __syncthreads();
  if (tid < LP_TOP) part_top[(size_t)slice * LP_TOP + tid] = tops[tid];
}

// max_rows: rows of the three logs. blockIdx.x = row: its logits, partials and token[row]. pos != nullptr (the decode
// step, one row): log row pos[0] - 1; pos == nullptr: log row row0 + row (the probe, the scored prompt pass)
__global__ __launch_bounds__(LP_MERGE_THREADS) void logprob_merge_kernel(
    const float* __restrict__ logits, size_t row_stride, int vocab, int n_slices, const uint32_t* __restrict__ part_key,
    const float* __restrict__ part_sum, const unsigned long long* __restrict__ part_top,
    const int32_t* __restrict__ token, const int32_t* __restrict__ pos, int row0, int max_rows,
    float* __restrict__ chosen, int32_t* __restrict__ top_id, float* __restrict__ top_lp) {
  constexpr int WAVES = LP_MERGE_THREADS / 64;
  __shared__ unsigned long long red[2 * WAVES];
  __shared__ unsigned long long tops[LP_TOP];
  __shared__ float wsum[WAVES];
  const int tid = threadIdx.x, row = blockIdx.x;
  logits += (size_t)row * row_stride;
  part_key += (size_t)row * n_slices, part_sum += (size_t)row * n_slices, part_top += (size_t)row * n_slices * LP_TOP;
  const int n_cand = n_slices * LP_TOP;
  unsigned long long c[LP_MERGE_PER];
#pragma unroll
  for (int j = 0; j < LP_MERGE_PER; ++j) {
    const int i = j * LP_MERGE_THREADS + tid;
    c[j] = i < n_cand ? part_top[i] : 0ull;
  }
  if (tid < LP_TOP) tops[tid] = 0ull;
  unsigned long long prev = ~0ull;
  uint32_t m_key = 0u;
  for (int r = 0; r < LP_TOP; ++r) {
    unsigned long long local = 0ull;
#pragma unroll
    for (int j = 0; j < LP_MERGE_PER; ++j) local = (c[j] < prev && c[j] > local) ? c[j] : local;
    const unsigned long long best = block_max_u64<WAVES>(local, red, r, tid);
    if (r == 0) m_key = (uint32_t)(best >> 32);
    if (best == 0ull) break;
    if (tid == 0) tops[r] = best;
    prev = best;
  }
  // Z over the slices, by slice index: thread t owns slices t, t + 1024, ...
  const float M = key_score(m_key);
  float acc = 0.f;
  for (int sl = tid; sl < n_slices; sl += LP_MERGE_THREADS) {
    const uint32_t k = part_key[sl];
    if (k != 0u) acc += part_sum[sl] * (k == m_key ? 1.f : expf(key_score(k) - M));
  }
  const float Z = block_sum_ordered<WAVES>(acc, wsum, tid);  // (its barrier also publishes `tops`)
  if (tid >= LP_TOP) return;
  const int p = pos != nullptr ? pos[0] - 1 : row0 + row;
  if (p < 0 || p >= max_rows) return;  // a position the logs have no row for: nothing is written
  const float logZ = M + logf(Z);
  const bool none = m_key == 0u;  // every logit NaN
  const unsigned long long t = tops[tid];
  top_id[(size_t)p * LP_TOP + tid] = t != 0ull ? (int32_t)(~(uint32_t)t) : -1;
  top_lp[(size_t)p * LP_TOP + tid] = t != 0ull ? key_score((uint32_t)(t >> 32)) - logZ : -INFINITY;
  if (tid == 0) {
    const int tok = token[row];
    chosen[p] = (none || tok < 0 || tok >= vocab) ? __uint_as_float(0x7FC00000u) : logits[tok] - logZ;
  }
}

}  // namespace

bool logprob_vocab_ok(int vocab) { return vocab >= 1 && (vocab + LP_SLICE - 1) / LP_SLICE <= LP_MAX_SLICES; }

size_t logprob_workspace_bytes(int vocab) {
  const size_t n = (size_t)((vocab + LP_SLICE - 1) / LP_SLICE);
  return n * (LP_TOP * 8 + 4 + 4);
}

// the two launches over `rows` logits rows; ws = rows * logprob_workspace_bytes(vocab)
static int launch_logprobs_impl(const float* logits, size_t row_stride, int vocab, int rows, const int32_t* token,
                                const int32_t* pos, int row0, int max_rows, void* ws, float* chosen, int32_t* top_id,
                                float* top_lp, hipStream_t st) {
  const int n_slices = (vocab + LP_SLICE - 1) / LP_SLICE;
  if (!logprob_vocab_ok(vocab)) return woq::fail("QBits: the log-probability record covers vocabularies of up to 418816 ids");
  const size_t n = (size_t)rows * n_slices;
  unsigned long long* part_top = (unsigned long long*)ws;  // [rows][n_slices][20], then the slice sums, then their max keys
  float* part_sum = (float*)(part_top + n * LP_TOP);
  uint32_t* part_key = (uint32_t*)(part_sum + n);
  hipLaunchKernelGGL(logprob_partial_kernel, dim3(n_slices, rows), dim3(LP_THREADS), 0, st, logits, row_stride, vocab,
                     part_key, part_sum, part_top);
  hipLaunchKernelGGL(logprob_merge_kernel, dim3(rows), dim3(LP_MERGE_THREADS), 0, st, logits, row_stride, vocab, n_slices,
                     part_key, part_sum, part_top, token, pos, row0, max_rows, chosen, top_id, top_lp);
  return 0;
}

int launch_logprobs(const float* logits, int vocab, const int32_t* token, const int32_t* pos, int max_rows, void* ws,
                    float* chosen, int32_t* top_id, float* top_lp, hipStream_t st) {
  return launch_logprobs_impl(logits, 0, vocab, 1, token, pos, 0, max_rows, ws, chosen, top_id, top_lp, st);
}

int launch_logprob_rows(const float* logits, size_t row_stride, int vocab, int rows, const int32_t* targets, int row0,
                        int max_rows, void* ws, float* chosen, int32_t* top_id, float* top_lp, hipStream_t st) {
  if (rows < 1 || rows > 65535) return woq::fail("QBits: the row form of the log-probability record takes 1..65535 rows");
  return launch_logprobs_impl(logits, row_stride, vocab, rows, targets, nullptr, row0, max_rows, ws, chosen, top_id, top_lp,
                              st);
}

}  // namespace woq

extern "C" {

WOQ_API int woq_probe_logprobs(const float* logits, int vocab, const int32_t* token_dev, float* chosen_out,
                               int32_t* top_id_out20, float* top_lp_out20, void* stream) {
  WOQ_TRY
  WOQ_CHECK(logits && token_dev && chosen_out && top_id_out20 && top_lp_out20 && vocab >= 1,
            "QBits: bad logprob probe arguments");
  const hipStream_t st = (hipStream_t)stream;
  void* ws = nullptr;
  WOQ_HIP(hipMallocAsync(&ws, woq::logprob_workspace_bytes(vocab), st));
  const int rc = woq::launch_logprobs(logits, vocab, token_dev, nullptr, 1, ws, chosen_out, top_id_out20, top_lp_out20,
                                      st);
  WOQ_HIP(hipFreeAsync(ws, st));
  if (rc) return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

}  // extern "C"
