// woq_h2o.hip — H2O heavy-hitter KV eviction (reference transformers/kv_cache_compression/prune/h2o.py, docs/h2o.md):
// the cache keeps the rows attention has looked at most, plus a recent window. Four pieces of device work:
//
//   score (decode)   score[kvh][p] += sum over the group's query heads g of softmax_p(q_g . K[p] / sqrt(D)), p = 0 .. pos,
//                    one launch per layer after that layer's K row was appended (h2o_score_decode_kernel)
//   score (prompt)   the column sums of a prompt chunk's causal attention, two launches (h2o_prompt_lse_kernel,
//                    h2o_prompt_colsum_kernel)
//   select           per (layer, kv head): the n_discard lowest scores among rows [n_keep, n_cached - recent), ties to the
//                    lower row, as a destination row (or -1) per source row (h2o_select_kernel)
//   compact          the gather: V and score rows copied, K rows rotated back by their own distance (h2o_compact_kernel)
//
// The score is the reference's hh_score (attention summed over the query axis, carried across steps), summed over a GQA
// group. q is the q attention uses (qkv bias, per-head q-norm, RoPE at the query's cache position); K is the cache row.
//
// Matrix-core shape, all three score kernels: S^T = K Q^T per 16 cache rows on v_mfma_f32_16x16x32_f16, A = the K rows
// (lane i16 = row, quarter kq: d = 32 c + 8 kq + e in step c), B = query rows in the same d order — the G heads of a kv
// group (decode; rows G .. 15 are zero) or 16 prompt rows of one head. The result leaves column i16 (head / query) in
// lane i16 with cache rows 4 kq + j. fp32 accumulation; the decode q enters as fp16 hi + lo (two products, like the
// grouped decode attention), the prompt q is the fp16 row the prompt attention itself reads. bf16 cache rows enter as
// fp16 (kv_load8), as in the attention kernels.
//
// No floating-point atomics anywhere: every sum has one order, so the same inputs give the same bytes.
//  * decode: a workgroup owns a slice of H2O_SLICE rows of one kv head, writes its logits and its per-head (max, sum)
//    to scratch and counts itself in (an integer counter); the LAST workgroup to arrive combines the slices' (max, sum)
//    in slice order and adds the G probabilities of every row in head order. Nobody waits for anybody.
//  * prompt: launch 1 writes log-sum-exp per (head, query). Launch 2 gives a wave 16 cache rows of one kv head, whose K
//    fragments stay in registers; it walks the query tiles in ascending order and the group's heads in ascending order,
//    rebuilds P = exp(S - lse), sums each tile's columns with a fixed butterfly and adds them up in that order.
//  * compact: see below (h2o_compact_kernel).
#include <algorithm>

#include "woq_attn_decode.h"
#include "woq_device.h"
#include "woq_host.h"
#include "woq_kv_codec.h"

namespace woq {
namespace {

constexpr int H2O_SLICE = 256;  // cache rows per workgroup of the decode score: 4 waves x 4 tiles of 16
constexpr int H2O_GMAX = 16;    // query heads per kv head: the columns of one MFMA tile

__host__ __device__ inline int h2o_slices(int max_ctx) { return (max_ctx + H2O_SLICE - 1) / H2O_SLICE; }
// scratch of the decode score: [kv_heads] arrival counters (zero between launches) | [kv_heads][slices][2][16] the
// slices' per-head (max, sum) | [kv_heads][16][max_ctx] logits
__host__ __device__ inline size_t h2o_cnt_bytes(int kv_heads) { return ((size_t)kv_heads * 4 + 255) & ~(size_t)255; }
__host__ __device__ inline size_t h2o_part_floats(int kv_heads, int max_ctx) {
  return (size_t)kv_heads * h2o_slices(max_ctx) * 2 * H2O_GMAX;
}

__device__ __forceinline__ float ld_agent_f32(const float* p) {
  return __uint_as_float(__hip_atomic_load((const unsigned int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// 16 rows of K (A operand) against the B fragments: the tile's S^T, unscaled
template <int KVD, int DC>
__device__ __forceinline__ void h2o_load_k(const void* kc, size_t elem, int kq, h8 (&kf)[DC]) {
#pragma unroll
  for (int c = 0; c < DC; ++c) kf[c] = kv_load8<KVD>(kc, elem + 32 * c + 8 * kq);
}

struct H2oDecodeArgs {
  const float* qkv;      // fp32 [(heads + 2 kv_heads) * D], un-rotated, bias included
  const void* kcache;    // this layer's K cache [max_ctx][kv_heads][D]; row *pos is the one just appended
  const int32_t* pos;
  const float *cs, *sn;  // fp32 [max_ctx][D / 2]
  const float* q_norm;   // fp32 [D] or null
  float eps;
  float* score;          // this layer's [kv_heads][max_ctx]
  unsigned int* count;
  float *part, *logit;
  int heads, kv_heads, max_ctx;
};

template <int KVD, int HD>
__global__ __launch_bounds__(256) void h2o_score_decode_kernel(const H2oDecodeArgs g) {
  constexpr int DC = HD / 32, half = HD / 2;
  __shared__ __attribute__((aligned(16))) float qs[H2O_GMAX * HD];
  __shared__ float red[4][H2O_GMAX];
  __shared__ float fin[2][H2O_GMAX];
  __shared__ int is_last;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;
  const int kh = blockIdx.x, sp = blockIdx.y, ns = (int)gridDim.y;
  const int G = g.heads / g.kv_heads;
  const int apos = g.pos[0];
  if (apos < 0 || apos >= g.max_ctx) return;  // (the step's first kernel clamps the position and raises the status)
  const int n = apos + 1;                      // rows 0 .. pos
  const int t_lo = sp * H2O_SLICE;
  if (t_lo >= n) return;
  const int n_act = (n + H2O_SLICE - 1) / H2O_SLICE;  // workgroups of this kv head that got this far

  // K rows of this wave's four tiles: they depend on the position alone, so they are requested first
  const size_t cache_row = (size_t)g.kv_heads * HD;
  h8 kf[4][DC];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int t0 = t_lo + wid * 64 + a * 16;
    if (t0 < n) h2o_load_k<KVD, DC>(g.kcache, (size_t)min(t0 + i16, apos) * cache_row + (size_t)kh * HD, kq, kf[a]);
  }
  // the group's query heads, one wave per head: q-norm and rotation as the per-head decode attention does them
  // (woq_attn_decode.h), unscaled — 1 / sqrt(D) multiplies the logits in fp32
  for (int gq = wid; gq < G; gq += 4) {
    const size_t oq = (size_t)(kh * G + gq) * HD + lane;
    float qa = 0.f, qb = 0.f, rc = 0.f, rs = 0.f;
    if (lane < half) {
      qa = g.qkv[oq], qb = g.qkv[oq + half];
      rc = g.cs[(size_t)apos * half + lane], rs = g.sn[(size_t)apos * half + lane];
    }
    if (g.q_norm != nullptr) {  // (wave-uniform; lanes that hold no q add 0)
      const float r = attn_qk_rnorm<HD>(qa, qb, g.eps);
      if (lane < half) qa = qa * (r * g.q_norm[lane]), qb = qb * (r * g.q_norm[lane + half]);
    }
    if (lane < half) {
      qs[gq * HD + lane] = fmaf(qa, rc, -(qb * rs));
      qs[gq * HD + lane + half] = fmaf(qb, rc, qa * rs);
    }
  }
  __syncthreads();
  h8 qh[DC], ql[DC];
#pragma unroll
  for (int c = 0; c < DC; ++c) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = i16 < G ? qs[i16 * HD + 32 * c + 8 * kq + e] : 0.f;
      const _Float16 hi = (_Float16)v;
      qh[c][e] = hi;
      ql[c][e] = (_Float16)(v - (float)hi);
    }
  }
  const float scale = 1.0f / sqrtf((float)HD);
  float* lg = g.logit + ((size_t)kh * H2O_GMAX + i16) * g.max_ctx;
  float s[4][4];
  float mx = -INFINITY;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int t0 = t_lo + wid * 64 + a * 16;
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
    if (t0 < n) {
#pragma unroll
      for (int c = 0; c < DC; ++c) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[a][c], ql[c], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[a][c], qh[c], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = t0 + kq * 4 + j;
      s[a][j] = p < n ? acc[j] * scale : -INFINITY;
      if (p < n && i16 < G) lg[p] = s[a][j];
      mx = fmaxf(mx, s[a][j]);
    }
  }
  // the slice's per-head max, then its sum of exponentials: across the quarters, then across the waves in wave order
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  if (kq == 0) red[wid][i16] = mx;
  __syncthreads();
  const float m = fmaxf(fmaxf(red[0][i16], red[1][i16]), fmaxf(red[2][i16], red[3][i16]));  // finite: row t_lo is live
  float l = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) l += s[a][j] == -INFINITY ? 0.f : expf(s[a][j] - m);
  l = reduce_kq(l);
  __syncthreads();
  if (kq == 0) red[wid][i16] = l;
  __syncthreads();
  float* part = g.part + ((size_t)kh * ns + sp) * 2 * H2O_GMAX;
  if (tid < H2O_GMAX) {
    part[tid] = m;
    part[H2O_GMAX + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  }
  // count in; the last workgroup of this kv head to arrive finishes for all of them
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    const unsigned int prev = atomicAdd(g.count + kh, 1u);
    is_last = prev == (unsigned int)(n_act - 1) ? 1 : 0;
    if (is_last) g.count[kh] = 0u;  // zero again for the next launch
  }
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  if (tid < H2O_GMAX) {
    const float* pk = g.part + (size_t)kh * ns * 2 * H2O_GMAX;
    float M = -INFINITY, L = 0.f;
    for (int i = 0; i < n_act; ++i) M = fmaxf(M, ld_agent_f32(pk + (size_t)i * 2 * H2O_GMAX + tid));
    for (int i = 0; i < n_act; ++i)
      L += ld_agent_f32(pk + (size_t)i * 2 * H2O_GMAX + H2O_GMAX + tid) *
           expf(ld_agent_f32(pk + (size_t)i * 2 * H2O_GMAX + tid) - M);
    fin[0][tid] = M, fin[1][tid] = L;
  }
  __syncthreads();
  const float* lk = g.logit + (size_t)kh * H2O_GMAX * g.max_ctx;
  float* sc = g.score + (size_t)kh * g.max_ctx;
  for (int p = tid; p < n; p += 256) {
    float add = 0.f;
    for (int gq = 0; gq < G; ++gq) add += expf(ld_agent_f32(lk + (size_t)gq * g.max_ctx + p) - fin[0][gq]) / fin[1][gq];
    sc[p] += add;
  }
}

// ---- prompt score ---------------------------------------------------------------------------------------------------
struct H2oPromptArgs {
  const _Float16* qkv;  // fp16 [T][(heads + 2 kv_heads) * D], q rotated in place by the append launch
  const void* kcache;   // this layer's K cache, rows 0 .. start + T - 1 written
  float* lse;           // [heads][T]
  float* score;         // this layer's [kv_heads][max_ctx]
  int T, start, heads, kv_heads, max_ctx;
};

// 16 query rows of head h from row q0 on, as B fragments (rows past T - 1 repeat it and are masked by the caller)
template <int HD>
__device__ __forceinline__ void h2o_load_q(const H2oPromptArgs& g, int h, int q0, int i16, int kq, h8 (&qf)[HD / 32]) {
  const size_t ld = (size_t)(g.heads + 2 * g.kv_heads) * HD;
  const _Float16* q = g.qkv + (size_t)min(q0 + i16, g.T - 1) * ld + (size_t)h * HD + 8 * kq;
#pragma unroll
  for (int c = 0; c < HD / 32; ++c) qf[c] = *(const h8*)(q + 32 * c);
}

// launch 1: lse[h][q] = log sum_p exp(q . K[p] / sqrt(D)) over p <= start + q. A wave = 16 queries of one head; every lane
// keeps a running (max, sum) over the rows 4 kq + j it sees, the four quarters meet at the end.
template <int KVD, int HD>
__global__ __launch_bounds__(256) void h2o_prompt_lse_kernel(const H2oPromptArgs g) {
  constexpr int DC = HD / 32;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, i16 = lane & 15, kq = lane >> 4;
  const int h = blockIdx.y, kh = h / (g.heads / g.kv_heads);
  const int q0 = (blockIdx.x * 4 + wid) * 16;
  if (q0 >= g.T) return;
  h8 qf[DC];
  h2o_load_q<HD>(g, h, q0, i16, kq, qf);
  const int last = g.start + min(q0 + 15, g.T - 1);  // the highest row any of the wave's queries sees
  const int mine = g.start + q0 + i16;               // the highest row this lane's query sees
  const size_t cache_row = (size_t)g.kv_heads * HD;
  const float scale = 1.0f / sqrtf((float)HD);
  float m_run = -INFINITY, l_run = 0.f;
  h8 kf[DC], kn[DC];
  h2o_load_k<KVD, DC>(g.kcache, (size_t)min(i16, last) * cache_row + (size_t)kh * HD, kq, kf);
  for (int t0 = 0; t0 <= last; t0 += 16) {
    if (t0 + 16 <= last)  // the next tile's rows are in flight while this one is scored
      h2o_load_k<KVD, DC>(g.kcache, (size_t)min(t0 + 16 + i16, last) * cache_row + (size_t)kh * HD, kq, kn);
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DC; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[c], qf[c], acc, 0, 0, 0);
    float s[4], tm = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = t0 + kq * 4 + j <= mine ? acc[j] * scale : -INFINITY;
      tm = fmaxf(tm, s[j]);
    }
    if (tm > -INFINITY) {
      const float m_new = fmaxf(m_run, tm);
      float ps = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) ps += s[j] == -INFINITY ? 0.f : expf(s[j] - m_new);
      l_run = (m_run == -INFINITY ? 0.f : l_run * expf(m_run - m_new)) + ps;
      m_run = m_new;
    }
#pragma unroll
    for (int c = 0; c < DC; ++c) kf[c] = kn[c];
  }
  float m_all = fmaxf(m_run, __shfl_xor(m_run, 16, 64));
  m_all = fmaxf(m_all, __shfl_xor(m_all, 32, 64));  // finite: every query sees row 0
  const float l_all = reduce_kq(m_run == -INFINITY ? 0.f : l_run * expf(m_run - m_all));
  if (kq == 0 && q0 + i16 < g.T) g.lse[(size_t)h * g.T + q0 + i16] = m_all + logf(l_all);
}

// launch 2: score[kvh][p] += sum over the group's heads and the chunk's queries of exp(S - lse). A wave = 16 cache rows
// of one kv head, K fragments in registers for the whole walk.
template <int KVD, int HD>
__global__ __launch_bounds__(256) void h2o_prompt_colsum_kernel(const H2oPromptArgs g) {
  constexpr int DC = HD / 32;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, i16 = lane & 15, kq = lane >> 4;
  const int kh = blockIdx.y, G = g.heads / g.kv_heads;
  const int nk = g.start + g.T;
  const int k0 = (blockIdx.x * 4 + wid) * 16;
  if (k0 >= nk) return;
  h8 kf[DC];
  h2o_load_k<KVD, DC>(g.kcache, ((size_t)min(k0 + i16, nk - 1) * g.kv_heads + kh) * HD, kq, kf);
  const float scale = 1.0f / sqrtf((float)HD);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int n_qt = (g.T + 15) / 16;
  for (int qt = max(0, k0 - g.start) / 16; qt < n_qt; ++qt) {  // earlier tiles hold no query that sees row k0
    const int q = qt * 16 + i16;
    for (int gq = 0; gq < G; ++gq) {
      const int h = kh * G + gq;
      h8 qf[DC];
      h2o_load_q<HD>(g, h, qt * 16, i16, kq, qf);
      const float lse = g.lse[(size_t)h * g.T + min(q, g.T - 1)];
      float4_t st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < DC; ++c) st = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[c], qf[c], st, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = k0 + kq * 4 + j;
        float pr = q < g.T && p <= g.start + q ? expf(st[j] * scale - lse) : 0.f;  // unseen rows: exactly nothing
        pr += __shfl_xor(pr, 1, 64);  // the tile's column sum over its 16 queries, a fixed butterfly
        pr += __shfl_xor(pr, 2, 64);
        pr += __shfl_xor(pr, 4, 64);
        pr += __shfl_xor(pr, 8, 64);
        acc[j] += pr;
      }
    }
  }
  if (i16 == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = k0 + kq * 4 + j;
      if (p < nk) g.score[(size_t)kh * g.max_ctx + p] += acc[j];
    }
  }
}

// ---- select -------------------------------------------------------------------------------------------------------------
// One workgroup per (layer, kv head). Scores are >= 0, so their bit patterns order as unsigned integers: a radix select,
// 8 bits a pass over a 256-bin LDS histogram (integer atomics: any order gives the same counts), finds the n_discard-th
// smallest key T of rows [lo, hi) and how many rows equal to T still go (`need`; the lower rows first). Then one pass in
// row order, 256 rows at a time: a row goes when its key is below T, or equals T with fewer than `need` equal rows below
// it (ballot prefix counts); the kept rows' running count is their destination.
__global__ __launch_bounds__(256) void h2o_select_kernel(const float* __restrict__ score, int32_t* __restrict__ dst,
                                                         int max_ctx, int lo, int hi, int n_discard, int n_cached) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned int pick[2];
  __shared__ int wsum[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const unsigned int* key = (const unsigned int*)(score + (size_t)blockIdx.x * max_ctx);
  int32_t* out = dst + (size_t)blockIdx.x * max_ctx;
  unsigned int prefix = 0u, mask = 0u, need = (unsigned int)n_discard;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    __syncthreads();
    for (int p = lo + tid; p < hi; p += 256) {
      const unsigned int k = key[p];
      if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned int run = 0u, b = 0u;
      for (; b < 255u; ++b) {
        if (run + hist[b] >= need) break;
        run += hist[b];
      }
      pick[0] = b, pick[1] = need - run;
    }
    __syncthreads();
    prefix |= pick[0] << shift, mask |= 255u << shift, need = pick[1];
    __syncthreads();
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  int eq_seen = 0, kept_seen = 0;
  for (int base = 0; base < n_cached; base += 256) {
    const int p = base + tid;
    const bool in = p < n_cached, range = in && p >= lo && p < hi;
    const unsigned int k = range ? key[p] : 0u;
    const bool eq = range && k == prefix;
    const unsigned long long be = __ballot(eq);
    if (lane == 0) wsum[0][wid] = __popcll(be);
    __syncthreads();
    int eq_before = eq_seen + __popcll(be & below);
    for (int w = 0; w < wid; ++w) eq_before += wsum[0][w];
    const bool evict = range && (k < prefix || (eq && eq_before < (int)need));
    const bool keep = in && !evict;
    const unsigned long long bk = __ballot(keep);
    if (lane == 0) wsum[1][wid] = __popcll(bk);
    __syncthreads();
    int kept_before = kept_seen + __popcll(bk & below);
    for (int w = 0; w < wid; ++w) kept_before += wsum[1][w];
    if (in) out[p] = keep ? kept_before : -1;
    eq_seen += wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
    kept_seen += wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
    __syncthreads();
  }
}

// ---- compact ------------------------------------------------------------------------------------------------------------
// The shift kernel's ordering argument (woq_kv_shift.hip) with a destination per row. A thread owns COLUMNS of one
// (layer, kv head) — for K one 8-element chunk and its partner D / 2 further, for V one 16-byte chunk of the head, for
// the score the head's one column — and walks the rows in ascending order by itself, so nothing between threads needs
// ordering. Kept rows keep their order, so a row's destination never lies above it and destinations ascend: inside the
// thread rows p .. p + N - 1 are loaded before any of them is stored, every store goes to a row already loaded, and a
// later load reads a higher row than any store so far has written. A destination that is not below its row moves nothing
// (an unmoved row keeps its bytes; anything else would be a map the select kernel never writes). K rows are rotated back
// by table row p - d with the shift kernel's arithmetic: fp64 products, fp32 sum, kv_store8.
struct H2oCompactArgs {
  uint8_t *k, *v;
  float* score;          // [layers][kv_heads][max_ctx], null = none to move
  const int32_t* dst;    // [layers][kv_heads][max_ctx]
  const float *cs, *sn;  // fp32 [max_ctx][D / 2]
  int layers, kv_heads, D, max_ctx, first, n_cached, n_discard;
};
constexpr int COMPACT_K_AHEAD = 4, COMPACT_V_AHEAD = 8;

template <int KVD, int N>
__device__ __forceinline__ void compact_k_rows(void* kc, size_t lo0, size_t row, int half, int col, int p,
                                               const int32_t* dst, const float* cs, const float* sn) {
  int d[N];
  float a[N][8], b[N][8];
  float4_t c[N][2], s[N][2];
#pragma unroll
  for (int u = 0; u < N; ++u) d[u] = dst[p + u];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    if (d[u] < 0 || d[u] >= p + u) continue;
    const size_t at = lo0 + (size_t)(p + u) * row;
    kv_load8_f32<KVD>(kc, at, a[u]);
    kv_load8_f32<KVD>(kc, at + half, b[u]);
    const size_t tr = (size_t)(p + u - d[u]) * half + col;
    c[u][0] = *(const float4_t*)(cs + tr), c[u][1] = *(const float4_t*)(cs + tr + 4);
    s[u][0] = *(const float4_t*)(sn + tr), s[u][1] = *(const float4_t*)(sn + tr + 4);
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    if (d[u] < 0 || d[u] >= p + u) continue;
    float lo[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double aj = (double)a[u][j], bj = (double)b[u][j];
      const double cj = (double)c[u][j >> 2][j & 3], sj = (double)s[u][j >> 2][j & 3];
      lo[j] = (float)(aj * cj + bj * sj);
      hi[j] = (float)(bj * cj - aj * sj);
    }
    const size_t at = lo0 + (size_t)d[u] * row;
    kv_store8<KVD>(kc, at, lo);
    kv_store8<KVD>(kc, at + half, hi);
  }
}

template <typename W, int N>
__device__ __forceinline__ void compact_copy_rows(uint8_t* base, size_t at0, size_t row_bytes, int p, const int32_t* dst) {
  int d[N];
  W w[N];
#pragma unroll
  for (int u = 0; u < N; ++u) d[u] = dst[p + u];
#pragma unroll
  for (int u = 0; u < N; ++u)
    if (d[u] >= 0 && d[u] < p + u) w[u] = *(const W*)(base + at0 + (size_t)(p + u) * row_bytes);
#pragma unroll
  for (int u = 0; u < N; ++u)
    if (d[u] >= 0 && d[u] < p + u) *(W*)(base + at0 + (size_t)d[u] * row_bytes) = w[u];
}

// blockIdx.y == 0: K threads, one per (layer, kv head, 8-element chunk of the head's first half); 1: V threads, one per
// (layer, kv head, 16-byte chunk of the head); 2: one thread per (layer, kv head) for the score row, which also clears
// the n_discard rows the compaction frees (the next steps add to them)
template <int KVD>
__global__ __launch_bounds__(256) void h2o_compact_kernel(const H2oCompactArgs g) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const size_t row = (size_t)g.kv_heads * g.D;
  constexpr int ES = KVD == WOQ_FP8_E4M3 ? 1 : 2;
  if (blockIdx.y == 0) {
    const int per_head = g.D / 16;
    if (t >= g.layers * g.kv_heads * per_head) return;
    const int lh = t / per_head, ch = t % per_head, l = lh / g.kv_heads, h = lh % g.kv_heads;
    const int half = g.D / 2;
    const size_t lo0 = (size_t)l * g.max_ctx * row + (size_t)h * g.D + 8 * ch;
    const int32_t* dst = g.dst + (size_t)lh * g.max_ctx;
    int p = g.first;
    for (; p + COMPACT_K_AHEAD <= g.n_cached; p += COMPACT_K_AHEAD)
      compact_k_rows<KVD, COMPACT_K_AHEAD>(g.k, lo0, row, half, 8 * ch, p, dst, g.cs, g.sn);
    for (; p < g.n_cached; ++p) compact_k_rows<KVD, 1>(g.k, lo0, row, half, 8 * ch, p, dst, g.cs, g.sn);
  } else if (blockIdx.y == 1) {
    const int per_head = g.D * ES / 16;
    if (t >= g.layers * g.kv_heads * per_head) return;
    const int lh = t / per_head, ch = t % per_head, l = lh / g.kv_heads, h = lh % g.kv_heads;
    const size_t row_bytes = row * ES;
    const size_t at0 = ((size_t)l * g.max_ctx * row + (size_t)h * g.D) * ES + (size_t)16 * ch;
    const int32_t* dst = g.dst + (size_t)lh * g.max_ctx;
    int p = g.first;
    for (; p + COMPACT_V_AHEAD <= g.n_cached; p += COMPACT_V_AHEAD)
      compact_copy_rows<u32x4, COMPACT_V_AHEAD>(g.v, at0, row_bytes, p, dst);
    for (; p < g.n_cached; ++p) compact_copy_rows<u32x4, 1>(g.v, at0, row_bytes, p, dst);
  } else {
    if (t >= g.layers * g.kv_heads || g.score == nullptr) return;
    const int32_t* dst = g.dst + (size_t)t * g.max_ctx;
    uint8_t* sc = (uint8_t*)(g.score + (size_t)t * g.max_ctx);
    int p = g.first;
    for (; p + COMPACT_V_AHEAD <= g.n_cached; p += COMPACT_V_AHEAD)
      compact_copy_rows<unsigned int, COMPACT_V_AHEAD>(sc, 0, 4, p, dst);
    for (; p < g.n_cached; ++p) compact_copy_rows<unsigned int, 1>(sc, 0, 4, p, dst);
    for (p = max(g.n_cached - g.n_discard, 0); p < g.n_cached; ++p) ((float*)sc)[p] = 0.f;
  }
}

__global__ void h2o_zero_kernel(unsigned int* p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0u;
}

const char* h2o_shape_problem(int kv_dtype, int heads, int kv_heads, int D, int max_ctx) {
  if (kv_dtype != WOQ_F16 && kv_dtype != WOQ_BF16 && kv_dtype != WOQ_FP8_E4M3)
    return "QBits: kv_dtype must be fp16, bf16 or fp8_e4m3";
  if (heads < 1 || kv_heads < 1 || heads % kv_heads != 0 || heads / kv_heads > H2O_GMAX)
    return "QBits: H2O takes at most 16 query heads per kv head";
  if (D != 64 && D != 128) return "QBits: H2O takes head_dim 64 or 128";
  if (max_ctx < 1) return "QBits: H2O: bad max_ctx";
  return nullptr;
}

// KERNEL<KVD, HD> for the runtime (kv_dtype, D); the shape was checked by h2o_shape_problem
#define H2O_DISPATCH(KERNEL, grid, args)                                                              \
  do {                                                                                                \
    if (D == 64) {                                                                                    \
      if (kv_dtype == WOQ_F16) hipLaunchKernelGGL((KERNEL<WOQ_F16, 64>), grid, dim3(256), 0, st, args);   \
      else if (kv_dtype == WOQ_BF16) hipLaunchKernelGGL((KERNEL<WOQ_BF16, 64>), grid, dim3(256), 0, st, args); \
      else hipLaunchKernelGGL((KERNEL<WOQ_FP8_E4M3, 64>), grid, dim3(256), 0, st, args);              \
    } else {                                                                                          \
      if (kv_dtype == WOQ_F16) hipLaunchKernelGGL((KERNEL<WOQ_F16, 128>), grid, dim3(256), 0, st, args);  \
      else if (kv_dtype == WOQ_BF16) hipLaunchKernelGGL((KERNEL<WOQ_BF16, 128>), grid, dim3(256), 0, st, args); \
      else hipLaunchKernelGGL((KERNEL<WOQ_FP8_E4M3, 128>), grid, dim3(256), 0, st, args);             \
    }                                                                                                 \
  } while (0)

}  // namespace

size_t h2o_decode_scratch_bytes(int kv_heads, int max_ctx) {
  return h2o_cnt_bytes(kv_heads) + (h2o_part_floats(kv_heads, max_ctx) + (size_t)kv_heads * H2O_GMAX * max_ctx) * 4;
}

void launch_h2o_zero(void* p, size_t bytes, hipStream_t st) {
  const size_t n = bytes / 4;
  if (n == 0) return;
  const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(h2o_zero_kernel, dim3(blocks), dim3(256), 0, st, (unsigned int*)p, n);
}

int launch_h2o_score_decode(const float* qkv, const void* kcache, int kv_dtype, int heads, int kv_heads, int D, int max_ctx,
                            const int32_t* pos, const float* cs, const float* sn, const float* q_norm, float eps,
                            float* score, void* scratch, hipStream_t st) {
  if (const char* why = h2o_shape_problem(kv_dtype, heads, kv_heads, D, max_ctx)) return fail(why);
  if (qkv == nullptr || kcache == nullptr || pos == nullptr || cs == nullptr || sn == nullptr || score == nullptr ||
      scratch == nullptr)
    return fail("QBits: H2O decode score: null buffer");
  H2oDecodeArgs g;
  g.qkv = qkv, g.kcache = kcache, g.pos = pos, g.cs = cs, g.sn = sn, g.q_norm = q_norm, g.eps = eps, g.score = score;
  g.count = (unsigned int*)scratch;
  g.part = (float*)((uint8_t*)scratch + h2o_cnt_bytes(kv_heads));
  g.logit = g.part + h2o_part_floats(kv_heads, max_ctx);
  g.heads = heads, g.kv_heads = kv_heads, g.max_ctx = max_ctx;
  const dim3 grid((unsigned)kv_heads, (unsigned)h2o_slices(max_ctx));
  H2O_DISPATCH(h2o_score_decode_kernel, grid, g);
  return 0;
}

int launch_h2o_score_prompt(const _Float16* qkv, int T, int start, int heads, int kv_heads, int D, const void* kcache,
                            int kv_dtype, int max_ctx, float* lse, float* score, hipStream_t st) {
  if (const char* why = h2o_shape_problem(kv_dtype, heads, kv_heads, D, max_ctx)) return fail(why);
  if (qkv == nullptr || kcache == nullptr || lse == nullptr || score == nullptr || T < 1 || start < 0 ||
      (long long)start + T > max_ctx)
    return fail("QBits: H2O prompt score: bad arguments");
  const H2oPromptArgs g = {qkv, kcache, lse, score, T, start, heads, kv_heads, max_ctx};
  const dim3 grid1((unsigned)((T + 63) / 64), (unsigned)heads);
  H2O_DISPATCH(h2o_prompt_lse_kernel, grid1, g);
  const dim3 grid2((unsigned)((start + T + 63) / 64), (unsigned)kv_heads);
  H2O_DISPATCH(h2o_prompt_colsum_kernel, grid2, g);
  return 0;
}

static const char* h2o_evict_problem(int layers, int kv_heads, int max_ctx, int n_keep, int n_discard, int recent,
                                     int n_cached) {
  if (layers < 1 || kv_heads < 1 || max_ctx < 1) return "QBits: H2O: bad cache geometry";
  if (n_keep < 0 || n_discard < 1 || recent < 0) return "QBits: H2O needs n_keep >= 0, n_discard >= 1 and recent >= 0";
  if ((long long)n_keep + n_discard + recent > n_cached)
    return "QBits: H2O: n_keep + n_discard + recent exceeds the cached positions";
  if (n_cached > max_ctx) return "QBits: H2O: n_cached exceeds max_ctx";
  return nullptr;
}

int launch_h2o_select(const float* score, int32_t* dst, int layers, int kv_heads, int max_ctx, int n_keep, int n_discard,
                      int recent, int n_cached, hipStream_t st) {
  if (const char* why = h2o_evict_problem(layers, kv_heads, max_ctx, n_keep, n_discard, recent, n_cached)) return fail(why);
  if (score == nullptr || dst == nullptr) return fail("QBits: H2O select: null buffer");
  hipLaunchKernelGGL(h2o_select_kernel, dim3((unsigned)(layers * kv_heads)), dim3(256), 0, st, score, dst, max_ctx, n_keep,
                     n_cached - recent, n_discard, n_cached);
  return 0;
}

int launch_h2o_compact(void* kseq, void* vseq, float* score, const int32_t* dst, int kv_dtype, int layers, int kv_heads,
                       int D, int max_ctx, const float* cs, const float* sn, int n_keep, int n_discard, int n_cached,
                       hipStream_t st) {
  if (const char* why = h2o_evict_problem(layers, kv_heads, max_ctx, n_keep, n_discard, 0, n_cached)) return fail(why);
  if (kseq == nullptr || vseq == nullptr || dst == nullptr || cs == nullptr || sn == nullptr || D < 16 || (D % 16) != 0)
    return fail("QBits: H2O compact: bad arguments");
  const int es = kv_dtype == WOQ_FP8_E4M3 ? 1 : 2;
  const long long most = (long long)layers * kv_heads * (D * es / 16);  // the V threads: at least as many as K's
  if (most > 0x7fffffffll - 256) return fail("QBits: H2O compact: the cache has too many columns for one launch");
  const H2oCompactArgs g = {(uint8_t*)kseq, (uint8_t*)vseq, score, dst, cs, sn, layers, kv_heads, D, max_ctx, n_keep, n_cached,
                            n_discard};
  const dim3 grid((unsigned)((most + 255) / 256), 3);
  switch (kv_dtype) {
    case WOQ_F16: hipLaunchKernelGGL(h2o_compact_kernel<WOQ_F16>, grid, dim3(256), 0, st, g); break;
    case WOQ_BF16: hipLaunchKernelGGL(h2o_compact_kernel<WOQ_BF16>, grid, dim3(256), 0, st, g); break;
    case WOQ_FP8_E4M3: hipLaunchKernelGGL(h2o_compact_kernel<WOQ_FP8_E4M3>, grid, dim3(256), 0, st, g); break;
    default: return fail("QBits: kv_dtype must be fp16, bf16 or fp8_e4m3");
  }
  return 0;
}

}  // namespace woq

// ---- the four kernels on caller buffers (include/woq_hip.h) --------------------------------------------------------------
extern "C" {

size_t woq_h2o_decode_scratch_bytes(int kv_heads, int max_ctx) {
  return kv_heads < 1 || max_ctx < 1 ? 0 : woq::h2o_decode_scratch_bytes(kv_heads, max_ctx);
}

int woq_h2o_score_decode(const void* qkv_f32, const void* kcache, int kv_dtype, int heads, int kv_heads, int head_dim,
                         int max_ctx, const void* pos_dev, const void* cos_dev, const void* sin_dev, const void* q_norm,
                         float eps, void* score, void* scratch, void* stream) {
  WOQ_TRY
  if (const int rc = woq::launch_h2o_score_decode((const float*)qkv_f32, kcache, kv_dtype, heads, kv_heads, head_dim, max_ctx,
                                                  (const int32_t*)pos_dev, (const float*)cos_dev, (const float*)sin_dev,
                                                  (const float*)q_norm, eps, (float*)score, scratch, (hipStream_t)stream))
    return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

int woq_h2o_score_prompt(const void* qkv_f16, int T, int start, int heads, int kv_heads, int head_dim, const void* kcache,
                         int kv_dtype, int max_ctx, void* lse, void* score, void* stream) {
  WOQ_TRY
  if (const int rc = woq::launch_h2o_score_prompt((const _Float16*)qkv_f16, T, start, heads, kv_heads, head_dim, kcache,
                                                  kv_dtype, max_ctx, (float*)lse, (float*)score, (hipStream_t)stream))
    return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

int woq_h2o_select(const void* score, void* dst, int layers, int kv_heads, int max_ctx, int n_keep, int n_discard,
                   int recent, int n_cached, void* stream) {
  WOQ_TRY
  if (const int rc = woq::launch_h2o_select((const float*)score, (int32_t*)dst, layers, kv_heads, max_ctx, n_keep, n_discard,
                                            recent, n_cached, (hipStream_t)stream))
    return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

int woq_h2o_compact(void* kcache, void* vcache, void* score, const void* dst, int kv_dtype, int layers, int kv_heads,
                    int head_dim, int max_ctx, const void* cos_dev, const void* sin_dev, int n_keep, int n_discard,
                    int n_cached, void* stream) {
  WOQ_TRY
  if (const int rc = woq::launch_h2o_compact(kcache, vcache, (float*)score, (const int32_t*)dst, kv_dtype, layers, kv_heads,
                                             head_dim, max_ctx, (const float*)cos_dev, (const float*)sin_dev, n_keep,
                                             n_discard, n_cached, (hipStream_t)stream))
    return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

}  // extern "C"
