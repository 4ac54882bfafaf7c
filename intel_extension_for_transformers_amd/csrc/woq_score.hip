// woq_score.hip — the log-probability the model assigns to tokens the caller SUPPLIES (woq_engine_prefill_scored):
// lm_head over every row of the prompt pass instead of the last one, on the matrix cores, and the record of
// woq_logprob.hip per row. Per block of at most 256 rows (the logits scratch is 256 x vocab x 4 bytes, whatever the
// prompt's length), four launches:
//   1. score_pack_kernel, one workgroup per row: final RMSNorm of the fp32 residual row (the formula and the summation
//      order of lm_head_kernel's prologue, woq_ops.hip) written as TWO 16-bit rows in the head's own type,
//      hi = cvt(x), lo = cvt(x - hi), K padded with zeros to a multiple of 32;
//   2. head_gemm_kernel: logits[r][v] = sum_k (hi[r][k] + lo[r][k]) * W[v][k], fp32 accumulation
//      (v_mfma_f32_16x16x32_f16 / _bf16), 128 x 128 output tile per workgroup of 256 threads, K in steps of 32 through
//      LDS, each weight fragment read once and multiplied against hi and lo;
//   3. + 4. logprob_partial_kernel / logprob_merge_kernel with a row dimension (launch_logprob_rows).
// Numerics. lm_head is dense fp16 / bf16 and exact in its stored type; the hi + lo pair carries the activation to about
// 2^-22 (fp16) / 2^-16 (bf16) of its magnitude, and every product hi * W, lo * W is exact in fp32. The logits therefore
// sit at fp32-accumulation distance from the exact product (the hi + lo idiom of woq_gemm_f16.hip's fp32 class, with two
// products because only one side needs splitting). A normalised value beyond the fp16 range (65504) overflows hi.
// Edges. Rows past M and ids past the vocabulary are masked at the loads (zeros) and at the stores; W is read in place,
// 16 bytes at a time, hence hidden % 8 == 0 and a 16-byte aligned W (score_shape_problem).
#include "woq_device.h"
#include "woq_host.h"
#include "../../include/woq_hip_experimental.h"

namespace woq {
namespace {

constexpr int SC_TILE = 128;          // output tile: rows x ids per workgroup
constexpr int SC_BK = 32;             // K per LDS stage = one MFMA's K
constexpr int SC_PITCH = SC_BK + 8;   // LDS row pitch in 16-bit elements (80 bytes: 16-byte aligned, rows spread over banks)
constexpr int SC_THREADS = 256;
constexpr int SC_STAGE = SC_TILE * (SC_BK / 8) / SC_THREADS;  // 16-byte chunks a thread stages per operand and K step

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int score_kpad(int hidden) { return (hidden + SC_BK - 1) / SC_BK * SC_BK; }

template <bool BF16>
__device__ __forceinline__ uint16_t cvt16(float v) {
  return BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
}
template <bool BF16>
__device__ __forceinline__ float back16(uint16_t b) {
  return BF16 ? bf16_bits_to_f32(b) : f16_bits_to_f32(b);
}

// one workgroup per row. hi / lo: [rows][kp] 16-bit
template <bool BF16>
__global__ __launch_bounds__(256) void score_pack_kernel(const float* __restrict__ hidden_rows,
                                                         const float* __restrict__ norm_w, float eps, int hidden, int kp,
                                                         uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
  __shared__ float part[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* x = hidden_rows + (size_t)blockIdx.x * hidden;
  float ss = 0.f;
  for (int i = tid; i < hidden; i += 256) {
    const float v = x[i];
    ss = fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  if (lane == 0) part[wid] = ss;
  __syncthreads();
  const float inv = 1.0f / sqrtf((part[0] + part[1] + part[2] + part[3]) / (float)hidden + eps);
  uint16_t* h = hi + (size_t)blockIdx.x * kp;
  uint16_t* l = lo + (size_t)blockIdx.x * kp;
  for (int i = tid; i < kp; i += 256) {
    uint16_t hb = 0, lb = 0;
    if (i < hidden) {
      const float xn = x[i] * inv * norm_w[i];
      hb = cvt16<BF16>(xn);
      lb = cvt16<BF16>(xn - back16<BF16>(hb));
    }
    h[i] = hb, l[i] = lb;
  }
}

template <bool BF16>
__device__ __forceinline__ float4_t mfma16(const u32x4& a, const u32x4& b, float4_t c) {
  if constexpr (BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, a), __builtin_bit_cast(half8_t, b), c, 0, 0, 0);
}

// grid (row tiles, id tiles): the row tiles of one id tile are neighbours in launch order, so a weight tile leaves HBM once.
// a_hi / a_lo [M][kp] (kp % 32 == 0, zero beyond hidden), W [vocab][hidden], out [M][ldo].
// Operand maps (16x16x32): lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j = 0..7
// — with B = W^T both are eight K-contiguous elements of a row; the result has col = l & 15, row = 4 (l >> 4) + reg.
template <bool BF16>
__global__ __launch_bounds__(SC_THREADS) void head_gemm_kernel(const uint16_t* __restrict__ a_hi,
                                                               const uint16_t* __restrict__ a_lo, int kp,
                                                               const uint16_t* __restrict__ W, int hidden, int vocab, int M,
                                                               float* __restrict__ out, size_t ldo) {
  __shared__ __attribute__((aligned(16))) uint16_t s_hi[SC_TILE * SC_PITCH];
  __shared__ __attribute__((aligned(16))) uint16_t s_lo[SC_TILE * SC_PITCH];
  __shared__ __attribute__((aligned(16))) uint16_t s_w[SC_TILE * SC_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int m0 = blockIdx.x * SC_TILE, v0 = blockIdx.y * SC_TILE;
  const int wm = (wid >> 1) * 64, wn = (wid & 1) * 64;  // the wave's 64 x 64 quarter of the tile
  const u32x4 zero = {0u, 0u, 0u, 0u};
  u32x4 r_hi[SC_STAGE], r_lo[SC_STAGE], r_w[SC_STAGE];
  // global -> registers: chunk c of the tile's 128 rows x 4 chunks; rows past M / ids past vocab / k past hidden read 0
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < SC_STAGE; ++i) {
      const int c = tid + i * SC_THREADS, row = c >> 2, k = k0 + (c & 3) * 8;
      const int ar = m0 + row, vr = v0 + row;
      r_hi[i] = zero, r_lo[i] = zero, r_w[i] = zero;
      if (ar < M) {
        r_hi[i] = *(const u32x4*)(a_hi + (size_t)ar * kp + k);
        r_lo[i] = *(const u32x4*)(a_lo + (size_t)ar * kp + k);
      }
      if (vr < vocab && k + 8 <= hidden) r_w[i] = *(const u32x4*)(W + (size_t)vr * hidden + k);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < SC_STAGE; ++i) {
      const int c = tid + i * SC_THREADS, o = (c >> 2) * SC_PITCH + (c & 3) * 8;
      *(u32x4*)(s_hi + o) = r_hi[i];
      *(u32x4*)(s_lo + o) = r_lo[i];
      *(u32x4*)(s_w + o) = r_w[i];
    }
  };
  float4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};
  const int frag = (lane & 15) * SC_PITCH + (lane >> 4) * 8;
  fetch(0);
  for (int k0 = 0; k0 < kp; k0 += SC_BK) {
    __syncthreads();  // the previous stage's reads are done
    stash();
    __syncthreads();
    if (k0 + SC_BK < kp) fetch(k0 + SC_BK);  // in flight under the MFMAs
    u32x4 b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = *(const u32x4*)(s_w + (wn + j * 16) * SC_PITCH + frag);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u32x4 ah = *(const u32x4*)(s_hi + (wm + i * 16) * SC_PITCH + frag);
      const u32x4 al = *(const u32x4*)(s_lo + (wm + i * 16) * SC_PITCH + frag);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[i][j] = mfma16<BF16>(ah, b[j], acc[i][j]);
        acc[i][j] = mfma16<BF16>(al, b[j], acc[i][j]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int v = v0 + wn + j * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
        if (row < M && v < vocab) out[(size_t)row * ldo + v] = acc[i][j][r];
      }
    }
}

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
struct ScoreScratch {
  uint16_t *hi, *lo;
  float* logits;
  void* lp_ws;
  size_t bytes;
};
ScoreScratch score_scratch(void* ws, int hidden, int vocab) {
  const size_t pack = align256((size_t)SCORE_BLOCK_ROWS * score_kpad(hidden) * 2);
  const size_t logits = align256((size_t)SCORE_BLOCK_ROWS * vocab * 4);
  char* p = (char*)ws;
  ScoreScratch s;
  s.hi = (uint16_t*)p, s.lo = (uint16_t*)(p + pack), s.logits = (float*)(p + 2 * pack), s.lp_ws = p + 2 * pack + logits;
  s.bytes = 2 * pack + logits + (size_t)SCORE_BLOCK_ROWS * logprob_workspace_bytes(vocab);
  return s;
}

}  // namespace

const char* score_shape_problem(const void* W, int w_dtype, int hidden, int vocab) {
  if (w_dtype != WOQ_F16 && w_dtype != WOQ_BF16) return "QBits: the scored head takes an fp16 or bf16 lm_head";
  if (hidden < 8 || hidden % 8 != 0) return "QBits: the scored head takes hidden sizes that are multiples of 8";
  if (((uintptr_t)W & 15) != 0) return "QBits: the scored head takes a 16-byte aligned lm_head";
  if (!logprob_vocab_ok(vocab)) return "QBits: the log-probability record covers vocabularies of up to 418816 ids";
  return nullptr;
}

size_t score_workspace_bytes(int hidden, int vocab) { return score_scratch(nullptr, hidden, vocab).bytes; }

int launch_score_rows(const float* hidden_rows, const float* norm_w, float eps, const void* W, int w_dtype, int hidden,
                      int vocab, const int32_t* targets, int M, int row0, int max_rows, void* ws, float* chosen,
                      int32_t* top_id, float* top_lp, hipStream_t st) {
  if (const char* why = score_shape_problem(W, w_dtype, hidden, vocab)) return woq::fail(why);
  const ScoreScratch s = score_scratch(ws, hidden, vocab);
  const int kp = score_kpad(hidden);
  const bool bf16 = w_dtype == WOQ_BF16;
  for (int r0 = 0; r0 < M; r0 += SCORE_BLOCK_ROWS) {
    const int rows = M - r0 < SCORE_BLOCK_ROWS ? M - r0 : SCORE_BLOCK_ROWS;
    const float* x = hidden_rows + (size_t)r0 * hidden;
    const dim3 grid((rows + SC_TILE - 1) / SC_TILE, (vocab + SC_TILE - 1) / SC_TILE);
    if (bf16) {
      hipLaunchKernelGGL(score_pack_kernel<true>, dim3(rows), dim3(256), 0, st, x, norm_w, eps, hidden, kp, s.hi, s.lo);
      hipLaunchKernelGGL(head_gemm_kernel<true>, grid, dim3(SC_THREADS), 0, st, s.hi, s.lo, kp, (const uint16_t*)W, hidden,
                         vocab, rows, s.logits, (size_t)vocab);
    } else {
      hipLaunchKernelGGL(score_pack_kernel<false>, dim3(rows), dim3(256), 0, st, x, norm_w, eps, hidden, kp, s.hi, s.lo);
      hipLaunchKernelGGL(head_gemm_kernel<false>, grid, dim3(SC_THREADS), 0, st, s.hi, s.lo, kp, (const uint16_t*)W, hidden,
                         vocab, rows, s.logits, (size_t)vocab);
    }
    const int rc = launch_logprob_rows(s.logits, (size_t)vocab, vocab, rows, targets + r0, row0 + r0, max_rows, s.lp_ws,
                                       chosen, top_id, top_lp, st);
    if (rc) return rc;
  }
  return 0;
}

}  // namespace woq

extern "C" {

WOQ_API int woq_probe_score_rows(const float* hidden_rows, const float* norm_w, float eps, const void* W, int w_dtype,
                                 int hidden, int vocab, const int32_t* targets, int M, float* chosen_out,
                                 int32_t* top_id_out, float* top_lp_out, void* stream) {
  WOQ_TRY
  WOQ_CHECK(hidden_rows && norm_w && W && targets && chosen_out && top_id_out && top_lp_out && M >= 1 && vocab >= 1,
            "QBits: bad score probe arguments");
  if (const char* why = woq::score_shape_problem(W, w_dtype, hidden, vocab)) return woq::fail(why);
  const hipStream_t st = (hipStream_t)stream;
  void* ws = nullptr;
  WOQ_HIP(hipMallocAsync(&ws, woq::score_workspace_bytes(hidden, vocab), st));
  const int rc = woq::launch_score_rows(hidden_rows, norm_w, eps, W, w_dtype, hidden, vocab, targets, M, 0, M, ws,
                                        chosen_out, top_id_out, top_lp_out, st);
  WOQ_HIP(hipFreeAsync(ws, st));
  if (rc) return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

}  // extern "C"
