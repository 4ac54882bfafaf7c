// woq_moe.h — what the product kernels of both forms of the routed expert block take (woq_moe.hip, woq_moe_prompt.hip).
#pragma once
#include "woq_gemv_common.h"
#include "woq_host.h"

namespace woq {

struct MoeGemmArgs {
  // the first 14 dwords, which the build's kernarg preload count covers
  const uint8_t* blobs;  // expert e's blob at blobs + e * stride
  size_t stride, off_q[2], off_scale, off_zp[2];  // [plane]: woq_host.h MoePlanes
  int K, N, tiles_k, n_groups, group, scale_type;
  // table kinds, grouped: the digit planes and wmul of lut_args_for, as the decode GEMV takes them | prompt: the 16 table
  // values as fp16, d[0] their low bytes and d[1] their high bytes (moe_prompt_lut)
  LutArgs lut;
  const void* x;  // gate/up: activations [T, ldx] of x_dtype; down: fp32 rows [sorted slot][ldx]
  int x_dtype, ldx, top_k;
  const int32_t* sorted;
  const MoeBlock* blocks;
  const int32_t* nblocks;
  float* out;  // gate/up: SiLU(g) * u [sorted slot][ldo] (raw: [g | u]); down: y [sorted slot][ldo]
  int ldo, half_tiles;
  int e5m2;      // fp8 blobs: the codes are e5m2
  int lds_rows;  // grouped only: the digit rows the fp8 launch's LDS holds, min(16, T k)
  int tiles_n;   // prompt only
};

// the blob part and the weight kind from the call's gate/up or down header, which has passed moe_header_problem; a
// table kind's `lut` is the form's to add
MoeGemmArgs moe_gemm_args(const MoeCall& m, bool gate_up, MoeWeightKind& kind);
// a product's role over a plan. Gate/up: rows of m.x gathered by token into out[sorted slot][ldo]; down: the fp32 rows
// h[sorted slot][I] into y[sorted slot][H]
void moe_bind_gate_up(MoeGemmArgs& g, const MoeCall& m, const MoeRoutePlan& p, float* out, int ldo);
void moe_bind_down(MoeGemmArgs& d, const MoeCall& m, const MoeRoutePlan& p, const float* h, float* y);

// the expert id of slot s, -1 outside [0, E): such a slot is dropped
template <bool IDX64>
__device__ __forceinline__ int moe_slot_id(const void* topk_idx, int s, int E) {
  const long long v = IDX64 ? (long long)((const int64_t*)topk_idx)[s] : (long long)((const int32_t*)topk_idx)[s];
  return (v >= 0 && v < (long long)E) ? (int)v : -1;
}

}  // namespace woq
