// woq_kv_codec.h — KV element codecs of the matrix-core attention kernels: eight consecutive cache elements
// (fp16 | bf16 | e4m3) <-> eight fp16 lanes. Shared by the prompt pass (woq_prefill.hip: rope_append_kernel,
// attn_prefill_kernel) and the grouped decode attention (woq_attn_decode.hip: attn_decode_mfma_kernel).
#pragma once
#include "woq_device.h"

namespace woq {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// eight e4m3 bytes -> eight fp16, exact (every e4m3 value is an fp16): gfx950's packed converter, one instruction per
// pair (round 4; the f32 detour cost three per pair, ~100 VALU per 32-position sub-tile of the long-context decode)
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ _Float16 __attribute__((ext_vector_type(8))) fp8x8_to_h8(
    unsigned int __attribute__((ext_vector_type(2))) raw) {
  const h2v a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(raw.x, 1.0f, false);
  const h2v b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(raw.x, 1.0f, true);
  const h2v c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(raw.y, 1.0f, false);
  const h2v d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(raw.y, 1.0f, true);
  return (_Float16 __attribute__((ext_vector_type(8)))){a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// 8 consecutive cache elements -> 8 fp16
template <int KVD>
__device__ __forceinline__ h8 kv_load8(const void* base, size_t elem) {
  if constexpr (KVD == WOQ_F16) {
    return *(const h8*)((const _Float16*)base + elem);
  } else if constexpr (KVD == WOQ_FP8_E4M3) {
    const u32x2 raw = *(const u32x2*)((const uint8_t*)base + elem);
    return fp8x8_to_h8(raw);
  } else {
    const u32x4 raw = *(const u32x4*)((const uint16_t*)base + elem);
    h8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (_Float16)bf16_bits_to_f32((uint16_t)(raw[j >> 1] >> (16 * (j & 1))));
    return r;
  }
}
// 8 consecutive cache elements -> 8 fp32, exact for every cache type (bf16 does not pass through fp16, whose range is
// narrower): what a kernel that re-stores the values with kv_store8 reads (woq_kv_shift.hip)
template <int KVD>
__device__ __forceinline__ void kv_load8_f32(const void* base, size_t elem, float (&v)[8]) {
  if constexpr (KVD == WOQ_BF16) {
    const u32x4 raw = *(const u32x4*)((const uint16_t*)base + elem);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf16_bits_to_f32((uint16_t)(raw[j >> 1] >> (16 * (j & 1))));
  } else {
    const h8 r = kv_load8<KVD>(base, elem);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)r[j];
  }
}
// 8 fp32 -> 8 consecutive cache elements (fp16 saturates at the format's largest finite value)
template <int KVD>
__device__ __forceinline__ void kv_store8(void* base, size_t elem, const float (&v)[8]) {
  if constexpr (KVD == WOQ_FP8_E4M3) {
    u32x2 w8;
    w8.x = f32x2_to_fp8x2(v[0], v[1]) | (f32x2_to_fp8x2(v[2], v[3]) << 16);
    w8.y = f32x2_to_fp8x2(v[4], v[5]) | (f32x2_to_fp8x2(v[6], v[7]) << 16);
    *(u32x2*)((uint8_t*)base + elem) = w8;
    return;
  }
  u32x4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t lo, hi;
    if constexpr (KVD == WOQ_F16) {
      lo = f32_to_f16_bits(fminf(fmaxf(v[2 * j], -65504.f), 65504.f));
      hi = f32_to_f16_bits(fminf(fmaxf(v[2 * j + 1], -65504.f), 65504.f));
    } else {
      lo = f32_to_bf16_bits(v[2 * j]);
      hi = f32_to_bf16_bits(v[2 * j + 1]);
    }
    w[j] = lo | (hi << 16);
  }
  *(u32x4*)((uint16_t*)base + elem) = w;
}

}  // namespace woq
