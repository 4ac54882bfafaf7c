// woq_score_key.h — the order-preserving integer key of an fp32 score, shared by the token tail's kernels
// (woq_sample.hip: argmax, radix select, candidate sort; woq_logprob.hip: the top-20 record). A (key << 32 | ~id) pair
// compares as (score descending, id ascending) under one unsigned 64-bit maximum.
#pragma once
#include "woq_device.h"

namespace woq {

// order-preserving key of a score: larger score <-> larger key; NaN -> 0 (below -inf, never a candidate); -0 == +0
__device__ __forceinline__ uint32_t score_key(float s) {
  if (s != s) return 0u;
  const uint32_t u = __float_as_uint(s + 0.0f);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t k) {
  return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

}  // namespace woq
