// woq_gemv_launch.h — host side shared by the decode-GEMV launchers (woq_gemv.hip, woq_gemv_i8.hip, woq_gemv_xq.hip,
// woq_gemv_attn.hip, woq_gemv_fp8.hip): the decoded view of a blob, the selector that turns a blob's quantisation form
// into template arguments, and the K-range plan of chained launches. Host code only.
#pragma once
#include <algorithm>
#include <type_traits>

#include "woq_gemv_common.h"
#include "woq_host.h"

namespace woq {

// ---- one decoded view of a blob -----------------------------------------------------------------------------------
struct BlobView {
  const u32x4* q;
  const void* scales;
  const uint8_t* zp;       // null = symmetric
  const int32_t* shuffle;  // GPTQ act-order: activation index of every weight row, or null
  int K, N, tiles_k, tiles_n, n_groups;
  int tpg_shift;  // scale_mode 0, several groups: log2(128-k tiles per group), else 0
  int smode;      // 0 = one scale per group of whole tiles (or a single group), 1 = one per 32-k block (woq_blob.h)
  bool asym, s32, sbf16;  // zero points present; fp32 scales; bf16 scales (else fp16; ignored for fp32 scales)
  int ndig;               // 0 = int4 codes; 1 | 2 | 3 = a 4-bit table type as that many digit planes (lut)
  LutArgs lut;
};

// Fills `v` from (blob, header); blob may be null where only the shape is asked about (the pointers are then null).
// Returns false when the tiles per group are no power of two: the MFMA kernels find a tile's group by a shift, so
// only the generic kernel (which divides) takes such a blob.
inline bool blob_view(const void* blob, const woq_blob_header& h, BlobView& v) {
  const uint8_t* b = (const uint8_t*)blob;
  v.q = b ? (const u32x4*)(b + h.off_q) : nullptr;
  v.scales = b ? b + h.off_scale : nullptr;
  v.zp = b && h.off_zp ? b + h.off_zp : nullptr;
  v.shuffle = b && h.off_shuffle ? (const int32_t*)(b + h.off_shuffle) : nullptr;
  v.K = h.K;
  v.N = h.N;
  v.tiles_k = h.Kpad / WOQ_TILE_K;
  v.tiles_n = h.Npad / WOQ_TILE_N;
  v.n_groups = h.n_groups;
  v.smode = (int)h.scale_mode;
  v.asym = h.off_zp != 0;
  v.s32 = h.scale_type == WOQ_F32;
  v.sbf16 = h.scale_type == WOQ_BF16;
  v.ndig = lut_args_for(h.weight_type, h.compute_type, v.lut);
  v.tpg_shift = 0;
  if (h.scale_mode == 0 && h.n_groups > 1) {
    int tpg = h.group / WOQ_TILE_K;
    if (tpg < 1 || (tpg & (tpg - 1)) != 0) return false;
    while (tpg > 1) {
      tpg >>= 1;
      ++v.tpg_shift;
    }
  }
  return true;
}

// ---- one selector for the quantisation form -----------------------------------------------------------------------
// Calls f(SMODE, ASYM, S32, NDIG) with the run-time form as std::integral_constant arguments and returns its result.
// The legal set: scale mode 0 | 1, fp32 scales or not, and either int4 codes (NDIG 0, with or without zero points) or a
// table type of 1 | 2 | 3 digit planes, which is symmetric. INT4_ONLY (the act-order form, the fused qkv + attention
// launch, the fp8 planes) leaves the table types out. Anything else fails with `bad`.
template <bool INT4_ONLY = false, typename F>
int select_qform(int smode, bool asym, bool s32, int ndig, const char* bad, F&& f) {
  using std::false_type;
  using std::true_type;
  auto scales = [&](auto AS, auto ND) {
    if (smode == 0) return s32 ? f(std::integral_constant<int, 0>{}, AS, true_type{}, ND)
                               : f(std::integral_constant<int, 0>{}, AS, false_type{}, ND);
    if (smode == 1) return s32 ? f(std::integral_constant<int, 1>{}, AS, true_type{}, ND)
                               : f(std::integral_constant<int, 1>{}, AS, false_type{}, ND);
    return woq::fail(bad);
  };
  if (ndig == 0) return asym ? scales(true_type{}, std::integral_constant<int, 0>{})
                             : scales(false_type{}, std::integral_constant<int, 0>{});
  if constexpr (!INT4_ONLY) {
    if (!asym && ndig == 1) return scales(false_type{}, std::integral_constant<int, 1>{});
    if (!asym && ndig == 2) return scales(false_type{}, std::integral_constant<int, 2>{});
    if (!asym && ndig == 3) return scales(false_type{}, std::integral_constant<int, 3>{});
  }
  return woq::fail(bad);
}

// f(TPW, CB) the same way: 4 | 8 tiles per wave, 1 | 2 column tiles per workgroup (the tile and XQ kernels' shapes)
template <typename F>
int select_tpw_cb(int tpw, int cb, F&& f) {
  const std::integral_constant<int, 1> c1;
  const std::integral_constant<int, 2> c2;
  const std::integral_constant<int, 4> t4;
  const std::integral_constant<int, 8> t8;
  if (cb == 2) return tpw == 4 ? f(t4, c2) : f(t8, c2);
  return tpw == 4 ? f(t4, c1) : f(t8, c1);
}

// ---- one K-range plan per family ----------------------------------------------------------------------------------
// A K range one launch cannot hold is split into `chunks` equal ranges of `per` tiles run as chained launches: chunk
// c > 0 adds onto chunk c - 1's fp32 output through the residual input, so only linear epilogues chain.
constexpr int K_PLAN_MAX_CHUNKS = 8;
struct KPlan {
  int chunks = 0;  // 0 = the family does not take this K range
  int tiles_k = 0, per = 0;
  int nw[K_PLAN_MAX_CHUNKS], tpw[K_PLAN_MAX_CHUNKS];  // waves x tiles per wave of chunk c
};
// geo(tiles, nw, tpw) -> bool: the family's geometry rule for one launch over `tiles` K tiles
template <typename Geo>
KPlan plan_k_ranges(int tiles_k, bool chainable, Geo geo) {
  KPlan p;
  int nw, tpw;
  for (int s = 1; s <= (chainable ? K_PLAN_MAX_CHUNKS : 1); ++s) {
    const int per = (tiles_k + s - 1) / s;
    if (!geo(per, nw, tpw)) continue;
    for (int c = 0; c < s && c * per < tiles_k; ++c)  // the last chunk may be shorter
      if (!geo(std::min(per, tiles_k - c * per), p.nw[c], p.tpw[c])) return p;
    p.chunks = s, p.tiles_k = tiles_k, p.per = per;
    break;
  }
  return p;
}
// body(c, kt_begin, kt_count, last) -> rc for every chunk of the plan, in order; stops at the first non-zero rc
template <typename F>
int for_each_k_chunk(const KPlan& p, F&& body) {
  for (int c = 0; c < p.chunks; ++c) {
    const int kt_begin = c * p.per, kt_count = std::min(p.per, p.tiles_k - kt_begin);
    if (kt_count <= 0) break;
    const int rc = body(c, kt_begin, kt_count, c == p.chunks - 1 || kt_begin + kt_count >= p.tiles_k);
    if (rc) return rc;
  }
  return 0;
}

}  // namespace woq
