// woq_rtn.h — the package's integer round-to-nearest rule at (bits, sym | asym), stated once (DESIGN.md "RTN";
// tests/quant_reference.py is its float64 statement). rintf = round half to even.
//
//   sym   s = max|w| / qmax (0 -> 1),                       code = clip(rne(w / s), -off, qmax),     value = code s
//   asym  s = (max(mx, 0) - min(mn, 0)) / levels (0 -> 1),  z = clip(rne(-min(mn, 0) / s), 0, levels),
//         c = clip(rne(w / s) + z, 0, levels),              code = c - off,                          value = (c - z) s
//         the range always holds zero, so a group on one side of zero is within half a step like any other
//
// rtn_kernel (woq_pack.hip) writes the blob's codes with it; the calibration searches take their candidates through it:
// gptq_sweep_kernel (woq_gptq.hip), awq_scale_delta_kernel and awq_clip_kernel (woq_awq.hip). They are correct only
// if it is the same rule bit for bit, which is why it lives here. AutoRound's quantiser (woq_autoround.hip) is this
// rule with V, alpha and beta put in and float clamps; it takes rtn_range from here and keeps its own expressions.
// TEQ's quantiser (woq_teq.hip) is this rule on w a[k]; its gradient also takes from rtn_params whether s was replaced.
// Every function turns contraction off for itself: each step is rounded on its own whatever the caller's setting.
#pragma once
#include <hip/hip_runtime.h>

namespace woq {

struct RtnRange {
  int qmax, levels, off;  // bits = 4: 7 / 15 / 8; 8: 127 / 255 / 128; 3: 3 / 7 / 4; 2: 1 / 3 / 2
};
__device__ __forceinline__ RtnRange rtn_range(int bits) {
  return {(1 << (bits - 1)) - 1, (1 << bits) - 1, 1 << (bits - 1)};
}

// the rule's parameters of a group whose values span [mn, mx] with largest magnitude amax -> whether the step came out
// zero and was replaced by 1: a gradient through s (woq_teq.hip) has to know, everyone else ignores it
__device__ __forceinline__ bool rtn_params(const RtnRange& r, int asym, float mx, float mn, float amax, float& s, int& z) {
#pragma clang fp contract(off)
  z = 0;
  bool replaced;
  if (!asym) {
    s = amax / (float)r.qmax;
    replaced = s == 0.f;
    if (replaced) s = 1.f;
  } else {
    const float hi = fmaxf(mx, 0.f), lo = fminf(mn, 0.f);
    s = (hi - lo) / (float)r.levels;
    replaced = s == 0.f;
    if (replaced) s = 1.f;
    z = max(0, min(r.levels, (int)rintf(-lo / s)));
  }
  return replaced;
}

// v under (s, z): the rule's code, in the signed domain woq_repack_quantized_weight takes, and that code's dequantised
// value, one fp32 product. One statement of both, so that a caller of both (the GPTQ sweep) divides and rounds once.
__device__ __forceinline__ void rtn_quant(const RtnRange& r, int asym, float v, float s, int z, int& code, float& deq) {
#pragma clang fp contract(off)
  if (!asym) {
    code = max(-r.off, min(r.qmax, (int)rintf(v / s)));
    deq = (float)code * s;
  } else {
    const int c = max(0, min(r.levels, (int)rintf(v / s) + z));
    deq = (float)(c - z) * s;
    code = c - r.off;
  }
}
__device__ __forceinline__ int rtn_code(const RtnRange& r, int asym, float v, float s, int z) {
  int code;
  float deq;
  rtn_quant(r, asym, v, s, z, code, deq);
  return code;
}
__device__ __forceinline__ float rtn_deq(const RtnRange& r, int asym, float v, float s, int z) {
  int code;
  float deq;
  rtn_quant(r, asym, v, s, z, code, deq);
  return deq;
}

// ---- host: what the entry points that take (bits, group) check ---------------------------------------------------------
inline bool rtn_bits_ok(int bits) { return bits == 2 || bits == 3 || bits == 4 || bits == 8; }

// the group size as the kernels take it: <= 0 or > K means one group per column
inline int rtn_group(int K, int group) { return (group <= 0 || group > K) ? K : group; }

// the number of groups of `group` > 0 rows (the last may be short), 0 where there are more than a grid's y dimension
// takes (65535)
inline int rtn_group_count(int K, int group) {
  const int n_groups = (K + group - 1) / group;
  return n_groups <= 65535 ? n_groups : 0;
}

}  // namespace woq
