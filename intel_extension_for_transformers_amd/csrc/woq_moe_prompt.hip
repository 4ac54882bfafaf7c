// woq_moe_prompt.hip — the prompt form of the routed expert block (woq_moe.hip states the definition): the same four
// stages for MANY rows per expert, on the fp16 matrix instruction v_mfma_f32_16x16x32_f16.
//
//  1. plan, three launches, for up to MOE_PROMPT_MAX_SLOTS slots s = t k + j in segments of 1024:
//       count    one workgroup per segment: histogram of the segment's ids over the experts in LDS (integer atomics: the
//                counts do not depend on the order) -> counts[segment][E]; pos_of[s] = -1 for an id outside [0, E)
//       scan     one workgroup: expert totals, their exclusive scan, counts[segment][e] <- first sorted position of
//                expert e's slots of that segment, and the block table {expert, first, rows <= MOE_PROMPT_ROWS} + count
//       scatter  one workgroup per segment: expert e's thread walks the segment's ids (LDS, a broadcast read) in
//                ascending order from counts[segment][e] -> sorted[], pos_of[]. Stable, so deterministic.
//     The host never learns the routing: the product grids are sized for ceil(S / 128) + min(E, S) blocks and a
//     workgroup past the count returns.
//  2. gate/up and 3. down: one kernel, moe_prompt_gemm_kernel<GU, SMODE, ASYM>. A workgroup of four waves takes one table
//     block (<= 128 rows of one expert) by 128 weight columns; a wave owns ALL the rows by two 16-column blob tiles — a
//     gate tile and the matching up tile (the workgroup then yields 64 columns of SiLU(g) * u), or two adjacent down
//     tiles — so every weight word is fetched and unpacked once per workgroup and meets all eight row tiles.
//       K is walked one blob tile (128 k) at a time. The block's rows are gathered through sorted[] (gate/up: the token
//     slot / top_k of x; down: the slot's own fp32 h row), multiplied by an exact power of two chosen PER ROW AND TILE
//     from the tile's largest magnitude (|x| 2^(15 - e) < 2^15), rounded once to fp16 and written to LDS in the A-fragment
//     image of the dense prompt GEMM (woq_gemm_f16.hip): 256-byte rows, 16-byte chunk c (8 k, in the nibble-extraction
//     order {0,2,4,6,1,3,5,7}) of row r in slot c ^ (r & 15), so every ds_read_b128 group covers the 64 banks once. Two
//     images: the next tile's weight words and activation rows are requested before this tile's MFMAs and converted
//     behind them; one barrier per tile.
//       Weights go from blob words to fp16 B fragments in registers, as dq8s of woq_gemm_f16.hip does it: a three-input
//     bit op per nibble pair gives fp16 (1024 + u | 64 + u), one packed add of -(base + zp) gives q - zp exactly.
//     scale_mode 0 has ONE scale per tile and column, so the operand stays the exact integer and the scale is applied in
//     fp32; scale_mode 1 (four 32-k scales a tile) multiplies by the scale relative to 2^E > the tile's largest scale of
//     that column (an exact power of two, so a scale of 5e-6 or a bf16 scale outside fp16's range stays normal).
//       A tile's products are accumulated in fresh fp32 fragments and folded into the running fp32 accumulators with
//     2^(e - 15)[row] * (scale | 2^E)[column]. The table types (nf4 / fp4) and the int8 composite differ in this step
//     alone: moe_prompt_lut8 selects fp16(table[code]) per nibble, the int8 operand is 16 (hi - zhi) + (lo - zlo) of the
//     two planes' words (exact in fp16), an fp8 code byte of the same two planes its exact fp16 value (moe_prompt_fp8);
//     scales as for int4. One fp16 product per operand pair, fp32 accumulation: the contract of the
//     dense prompt GEMM's bf16 / fp16 / int8 compute modes. Row tiles past the block's rows are skipped wave-uniformly.
//  4. combine: woq_moe.hip's launch_moe_combine.
// The host front is woq_moe.hip's: the workspace layout, the entry points' checks and launch_moe_forward, which under
// MOE_PROMPT calls launch_moe_prompt_plan and launch_moe_prompt_product below.
// No split-K, no floating-point atomics, a fixed summation order: the same inputs give the same bytes.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "woq_moe.h"

namespace woq {
namespace {

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int MP_SEG = MOE_PLAN_SEG;                  // slots of one plan segment = threads of a plan workgroup
constexpr int MP_ROWS = MOE_PROMPT_ROWS;              // rows of a table block
constexpr int MP_WAVES = 4, MP_CT = 2;                // waves of a workgroup, column tiles of a wave
constexpr int MP_IMAGE = MP_ROWS * WOQ_TILE_K * 2;    // bytes of one A image: 128 rows x 128 k fp16
constexpr int MP_LDS = 2 * MP_IMAGE + 2 * MP_ROWS * 4;  // two images + two sets of row factors
static_assert(MP_ROWS == 128, "the staging map and the eight row tiles of a wave assume 128-row blocks");

// ---- 1. plan ---------------------------------------------------------------------------------------------------------
template <bool IDX64>
__global__ __launch_bounds__(MP_SEG) void moe_prompt_count_kernel(const void* __restrict__ topk_idx, int S, int E,
                                                                  int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ pos_of) {
  __shared__ int32_t cnt[MOE_MAX_EXPERTS];
  const int tid = threadIdx.x, seg = blockIdx.x, s = seg * MP_SEG + tid;
  if (tid < E) cnt[tid] = 0;
  __syncthreads();
  if (s < S) {
    const int e = moe_slot_id<IDX64>(topk_idx, s, E);
    if (e >= 0)
      atomicAdd(&cnt[e], 1);  // an integer count: the result does not depend on the order
    else
      pos_of[s] = -1;
  }
  __syncthreads();
  if (tid < E) counts[(size_t)seg * E + tid] = cnt[tid];
}

__global__ __launch_bounds__(MP_SEG) void moe_prompt_scan_kernel(int nseg, int E, int32_t* __restrict__ counts,
                                                                 MoeBlock* __restrict__ blocks,
                                                                 int32_t* __restrict__ nblocks) {
  __shared__ int32_t tot[MOE_MAX_EXPERTS], off[MOE_MAX_EXPERTS], bb[MOE_MAX_EXPERTS];
  const int e = threadIdx.x;
  if (e < E) {
    int c = 0;
    for (int g = 0; g < nseg; ++g) c += counts[(size_t)g * E + e];
    tot[e] = c;
  }
  __syncthreads();
  if (e == 0) {
    int run = 0, nb = 0;
    for (int i = 0; i < E; ++i) {
      off[i] = run, bb[i] = nb;
      run += tot[i], nb += (tot[i] + MP_ROWS - 1) / MP_ROWS;
    }
    *nblocks = nb;
  }
  __syncthreads();
  if (e >= E) return;
  int run = off[e];
  for (int g = 0; g < nseg; ++g) {
    const int c = counts[(size_t)g * E + e];
    counts[(size_t)g * E + e] = run;
    run += c;
  }
  for (int r = 0, nb = bb[e]; r < tot[e]; r += MP_ROWS, ++nb)
    blocks[nb] = MoeBlock{e, off[e] + r, min(MP_ROWS, tot[e] - r), 0};
}

template <bool IDX64>
__global__ __launch_bounds__(MP_SEG) void moe_prompt_scatter_kernel(const void* __restrict__ topk_idx, int S, int E,
                                                                    const int32_t* __restrict__ counts,
                                                                    int32_t* __restrict__ sorted,
                                                                    int32_t* __restrict__ pos_of) {
  __shared__ int32_t ids[MP_SEG];
  const int tid = threadIdx.x, seg = blockIdx.x, s0 = seg * MP_SEG;
  const int n = min(MP_SEG, S - s0);
  ids[tid] = tid < n ? moe_slot_id<IDX64>(topk_idx, s0 + tid, E) : -1;
  __syncthreads();
  if (tid >= E) return;
  int p = counts[(size_t)seg * E + tid];
  for (int i = 0; i < n; ++i) {  // every thread reads the same LDS word: a broadcast
    if (ids[i] == tid) {
      sorted[p] = s0 + i;
      pos_of[s0 + i] = p;
      ++p;
    }
  }
}

// ---- 2 / 3. the grouped product --------------------------------------------------------------------------------------
template <int SMODE, int NP>
struct MoePromptB {  // one K tile of one wave's weight operand, as loaded; NP nibble planes
  u32x4 w[MP_CT][NP];
  float sc[MP_CT][SMODE == 1 ? 4 : 1];
  uint32_t uz[MP_CT][NP][SMODE == 1 ? 2 : 1];
};

// 8 signed nibbles of one blob word -> 8 fp16 (q - zp) [* r], k order {0,2,4,6,1,3,5,7}: dq8s of woq_gemm_f16.hip
template <bool MUL>
__device__ __forceinline__ h8 moe_prompt_dq8(uint32_t w, h2 nlo, h2 nhi, h2 r) {
  const uint32_t y = w >> 8;
  h2 f0 = __builtin_bit_cast(h2, (w & 0x000f000fu) ^ 0x64086408u) + nlo;
  h2 f1 = __builtin_bit_cast(h2, (w & 0x00f000f0u) ^ 0x54805480u) + nhi;
  h2 f2 = __builtin_bit_cast(h2, (y & 0x000f000fu) ^ 0x64086408u) + nlo;
  h2 f3 = __builtin_bit_cast(h2, (y & 0x00f000f0u) ^ 0x54805480u) + nhi;
  if constexpr (MUL) f0 *= r, f1 *= r, f2 *= r, f3 *= r;
  return __builtin_bit_cast(h8, (u32x4){__builtin_bit_cast(uint32_t, f0), __builtin_bit_cast(uint32_t, f1),
                                        __builtin_bit_cast(uint32_t, f2), __builtin_bit_cast(uint32_t, f3)});
}

// 8 table codes of one blob word -> the 8 fp16 table values in moe_prompt_dq8's element order. lut_quad looks up a byte
// per code in either byte plane of the fp16 table; v_perm_b32 pairs the low and high bytes of k-offsets (0, 2) | (1, 3)
// of the low nibbles and (4, 6) | (5, 7) of the high ones.
__device__ __forceinline__ h8 moe_prompt_lut8(const LutArgs& L, uint32_t w) {
  uint32_t lo[2], hi[2];
  lut_quad<2>(L, w & 0x0f0f0f0fu, lo);
  lut_quad<2>(L, (w >> 4) & 0x0f0f0f0fu, hi);
  return __builtin_bit_cast(h8, (u32x4){__builtin_amdgcn_perm(lo[1], lo[0], 0x06020400u),
                                        __builtin_amdgcn_perm(hi[1], hi[0], 0x06020400u),
                                        __builtin_amdgcn_perm(lo[1], lo[0], 0x07030501u),
                                        __builtin_amdgcn_perm(hi[1], hi[0], 0x07030501u)});
}

// 8 fp8 codes of one word of each nibble plane, code = (hi << 4) | (lo ^ 8) (include/woq_blob.h woq_fp8_headers), -> 8
// fp16 in moe_prompt_dq8's element order. Byte b of a word holds k = b in its low nibble and k = b + 4 in its high one, so
// the low nibbles give the codes of k 0..3 and the high ones those of k 4..7; v_perm_b32 puts codes (0, 2) | (4, 6) |
// (1, 3) | (5, 7) into the HIGH bytes of a half pair. An e5m2 code is the high byte of the fp16 of the same value, exactly
// (subnormals, both zeros). An e4m3 code s eeee mmm becomes s 0eeee mmm0000000: the fp16 of value 2^-8 — normal codes
// through the exponent bias (15 against 7), subnormal ones (eeee = 0) as fp16 subnormals with the same significand, -0 as
// -0 — and the packed multiply by 2^8 (times the relative scale under scale_mode 1: then the one rounding of the
// operand) restores the value before it meets the MFMA; no operand is left subnormal by the format change itself.
template <bool E5M2>
__device__ __forceinline__ h8 moe_prompt_fp8(uint32_t hi, uint32_t lo, _Float16 mul) {
  const uint32_t c03 = ((hi & 0x0f0f0f0fu) << 4) | ((lo & 0x0f0f0f0fu) ^ 0x08080808u);
  const uint32_t c47 = (hi & 0xf0f0f0f0u) | (((lo >> 4) & 0x0f0f0f0fu) ^ 0x08080808u);
  u32x4 t = {__builtin_amdgcn_perm(0u, c03, 0x020c000cu), __builtin_amdgcn_perm(0u, c47, 0x020c000cu),
             __builtin_amdgcn_perm(0u, c03, 0x030c010cu), __builtin_amdgcn_perm(0u, c47, 0x030c010cu)};
  if constexpr (!E5M2) t = (t & 0x80008000u) | ((t >> 1) & 0x3f803f80u);
  return __builtin_bit_cast(h8, t) * mul;
}

// GU: the gate/up launch (gate tile + up tile per wave, SiLU * mul epilogue, rows gathered by token) | the down launch
// WK (woq_host.h MoeWeightKind) picks the blob words -> fp16 B fragment step and nothing else:
//   MOE_W_TABLE  fp16(table[code]) per nibble (moe_prompt_lut8): exact for fp4_e2m1, one rounding of the value otherwise
//   MOE_W_INT8   16 (hi - zhi) + (lo - zlo) from the two planes' words, an integer of magnitude <= 255: exact in fp16
//   MOE_W_FP8    the exact fp16 value of the code byte of the two planes' words (moe_prompt_fp8); MP_W_FP8_E5M2 its e5m2 form
// either times the relative scale under scale_mode 1, as the int4 operand is.
constexpr int MP_W_FP8_E5M2 = MOE_W_FP8 + 1;
// RAW (the backward's recompute, gate/up only): the epilogue stores the fp32 g and u themselves, row [g (I) | u (I)] of
// [sorted slot][ldo = 2 I], instead of SiLU(g) * u
template <bool GU, int SMODE, bool ASYM, int WK, bool RAW = false>
__global__ __launch_bounds__(MP_WAVES * 64, 2) void moe_prompt_gemm_kernel(const MoeGemmArgs a) {
  static_assert(GU || !RAW, "the raw epilogue belongs to the gate/up launch");
  constexpr int NS = SMODE == 1 ? 2 : 1;  // scales of a tile, column and lane: its 32-k block of either 64-k half
  constexpr bool FP8 = WK == MOE_W_FP8 || WK == MP_W_FP8_E5M2;
  constexpr int NP = WK == MOE_W_INT8 || FP8 ? 2 : 1;
  static_assert(!((WK == MOE_W_TABLE || FP8) && ASYM), "the table and fp8 types are symmetric");
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];  // [2][MP_IMAGE] images, [2][MP_ROWS] factors
  float* unsc = (float*)(smem + 2 * MP_IMAGE);

  const int b = (int)blockIdx.y;
  if (b >= *a.nblocks) return;
  const MoeBlock blk = a.blocks[b];
  const int expert = __builtin_amdgcn_readfirstlane(blk.expert), first = __builtin_amdgcn_readfirstlane(blk.first);
  const int R = __builtin_amdgcn_readfirstlane(blk.rows);
  const int nrt = (R + 15) >> 4;       // live row tiles
  const int nst = (nrt + 1) & ~1;      // staged row tiles: the MFMA loop takes them in pairs
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;

  const uint8_t* blob = a.blobs + (size_t)expert * a.stride;
  const u32x4* q[NP];
  const uint8_t* zps[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) q[p] = (const u32x4*)(blob + a.off_q[p]), zps[p] = blob + a.off_zp[p];
  const void* scales = blob + a.off_scale;
  // this wave's column tiles (clamped for the loads; `live` decides the stores)
  int tn[MP_CT];
  bool live[MP_CT];
  const int wt = (int)blockIdx.x * MP_WAVES + wid;
  if constexpr (GU) {
    live[0] = live[1] = wt < a.half_tiles;
    tn[0] = min(wt, a.half_tiles - 1), tn[1] = tn[0] + a.half_tiles;
  } else {
#pragma unroll
    for (int c = 0; c < MP_CT; ++c) live[c] = wt * MP_CT + c < a.tiles_n, tn[c] = min(wt * MP_CT + c, a.tiles_n - 1);
  }

  // staging map: thread = (row group rg, chunk c16); item i = row 16 i + rg, i.e. one row tile per item
  const int c16 = tid & 15, rg = tid >> 4;
  int src[8];  // the item's source row (gate/up: the token; down: the sorted slot), -1 = no row
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = 16 * i + rg;
    src[i] = -1;
    if (row < R) src[i] = GU ? a.sorted[first + row] / a.top_k : first + row;
  }
  const bool x32 = !GU || a.x_dtype == WOQ_F32, xbf = a.x_dtype == WOQ_BF16;

  // Staging runs in two halves of four row tiles (half g: items 4 g .. 4 g + 3), each requested before one half of the
  // tile's MFMAs and converted behind it: 32 registers in flight instead of 64.
  u32x4 raw[4][2];
  auto stage_load = [&](int kt, int g) {  // K % 4 == 0: a group of four elements lies inside K or outside it
    const int k = kt * WOQ_TILE_K + c16 * 8;
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const int i = 4 * g + ii;
      raw[ii][0] = raw[ii][1] = u32x4{0u, 0u, 0u, 0u};
      if (i >= nst || src[i] < 0) continue;
      const size_t so = (size_t)src[i] * a.ldx + k;
      if (x32) {
        const float* p = (const float*)a.x + so;
        if (k + 4 <= a.K) raw[ii][0] = *(const u32x4*)p;
        if (k + 8 <= a.K) raw[ii][1] = *(const u32x4*)(p + 4);
      } else {
        const uint16_t* p = (const uint16_t*)a.x + so;
        if (k + 4 <= a.K) {
          const uint2 v = *(const uint2*)p;
          raw[ii][0].x = v.x, raw[ii][0].y = v.y;
        }
        if (k + 8 <= a.K) {
          const uint2 v = *(const uint2*)(p + 4);
          raw[ii][0].z = v.x, raw[ii][0].w = v.y;
        }
      }
    }
  };
  auto stage_write = [&](int buf, int g) {
    unsigned char* img = smem + buf * MP_IMAGE;
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const int i = 4 * g + ii;
      if (i >= nst) break;  // wave-uniform
      float f[8];
      if (x32) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = __uint_as_float(raw[ii][j >> 2][j & 3]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint16_t bits = (uint16_t)(raw[ii][0][j >> 1] >> (16 * (j & 1)));
          const float fb = bf16_bits_to_f32(bits), fh = f16_bits_to_f32(bits);
          f[j] = xbf ? fb : fh;
        }
      }
      float amax = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
      // the 16 lanes of a DPP row hold the 16 chunks of one activation row: four butterfly steps leave the row's maximum
      amax = fmaxf(amax, WOQ_DPP_F32(amax, 0xB1));
      amax = fmaxf(amax, WOQ_DPP_F32(amax, 0x4E));
      amax = fmaxf(amax, WOQ_DPP_F32(amax, 0x141));
      amax = fmaxf(amax, WOQ_DPP_F32(amax, 0x140));
      int e = 0;  // amax < 2^e  =>  |x| 2^(15 - e) < 2^15
      if (amax > 0.f && amax < INFINITY) e = max(-100, min(100, __builtin_amdgcn_frexp_expf(amax)));
      const float sfix = ldexpf(1.f, 15 - e);
      const int row = 16 * i + rg;
      h8 hh;
#pragma unroll
      for (int e8 = 0; e8 < 8; ++e8) hh[e8] = (_Float16)(f[e8 < 4 ? 2 * e8 : 2 * (e8 - 4) + 1] * sfix);
      *(h8*)(img + row * 256 + ((c16 ^ (row & 15)) << 4)) = hh;
      if (c16 == 0) unsc[buf * MP_ROWS + row] = row < R ? ldexpf(1.f, e - 15) : 0.f;
    }
  };

  // plane p carries zero points under ASYM; the int8 composite's LO plane (p == 1) always does
  auto load_uz = [&](int p, size_t si) { return !FP8 && (ASYM || p == 1) ? (uint32_t)zps[p][si] : 8u; };
  auto load_b = [&](int kt, MoePromptB<SMODE, NP>& bw) {
#pragma unroll
    for (int c = 0; c < MP_CT; ++c) {
#pragma unroll
      for (int p = 0; p < NP; ++p)
        bw.w[c][p] = __builtin_nontemporal_load(q[p] + ((size_t)tn[c] * a.tiles_k + kt) * 64 + lane);
      if constexpr (SMODE == 0) {
        const int grp = a.n_groups == 1 ? 0 : min(kt * WOQ_TILE_K / a.group, a.n_groups - 1);
        const size_t si = ((size_t)tn[c] * a.n_groups + grp) * 16 + i16;
        bw.sc[c][0] = load_f32(scales, si, a.scale_type);
#pragma unroll
        for (int p = 0; p < NP; ++p) bw.uz[c][p][0] = load_uz(p, si);
      } else {
        const size_t si = (((size_t)tn[c] * a.tiles_k + kt) * 16 + i16) * 4;
#pragma unroll
        for (int s = 0; s < 4; ++s) bw.sc[c][s] = load_f32(scales, si + s, a.scale_type);
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int h = 0; h < 2; ++h) bw.uz[c][p][h] = load_uz(p, si + 2 * h + (kq >> 1));
      }
    }
  };

  float4_t acc[8][MP_CT];
#pragma unroll
  for (int rt = 0; rt < 8; ++rt)
#pragma unroll
    for (int c = 0; c < MP_CT; ++c) acc[rt][c] = (float4_t){0.f, 0.f, 0.f, 0.f};
  // A fragment of (64-k half h, part p) = blob word hp = 2 h + p: chunk 8 h + 2 kq + p of row 16 rt + i16
  int a_off[4];
#pragma unroll
  for (int hp = 0; hp < 4; ++hp) a_off[hp] = i16 * 256 + ((((hp >> 1) * 8 + kq * 2 + (hp & 1)) ^ i16) << 4);

  float cs[MP_CT];   // fp32 column factor of the tile in hand
  h8 bf[4][MP_CT];   // its B fragments
  auto unpack = [&](const MoePromptB<SMODE, NP>& bw) {
#pragma unroll
    for (int c = 0; c < MP_CT; ++c) {
      h2 r2[NS], nlo[NP][NS], nhi[NP][NS];
      if constexpr (SMODE == 0) {
        cs[c] = bw.sc[c][0];
        r2[0] = (h2){(_Float16)1.f, (_Float16)1.f};
      } else {
        const float mx = fmaxf(fmaxf(fabsf(bw.sc[c][0]), fabsf(bw.sc[c][1])), fmaxf(fabsf(bw.sc[c][2]), fabsf(bw.sc[c][3])));
        int E2 = 0;  // mx < 2^E2: the relative scales lie in (-1, 1), the largest of them in [1/2, 1)
        if (mx > 0.f && mx < INFINITY) E2 = max(-120, min(120, __builtin_amdgcn_frexp_expf(mx)));
        cs[c] = ldexpf(1.f, E2);
        const float inv = ldexpf(1.f, -E2);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const _Float16 rr = (_Float16)((kq < 2 ? bw.sc[c][2 * h] : bw.sc[c][2 * h + 1]) * inv);
          r2[h] = (h2){rr, rr};
        }
      }
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const float uz = (float)(bw.uz[c][p][s] & 0xffu);
          const _Float16 l = (_Float16)(-(1024.f + uz)), hg = (_Float16)(-(64.f + uz));
          nlo[p][s] = (h2){l, l}, nhi[p][s] = (h2){hg, hg};
        }
#pragma unroll
      for (int hp = 0; hp < 4; ++hp) {
        const int s = SMODE == 0 ? 0 : (hp >> 1);
        if constexpr (WK == MOE_W_INT4) {
          bf[hp][c] = moe_prompt_dq8<SMODE == 1>(bw.w[c][0][hp], nlo[0][s], nhi[0][s], r2[s]);
        } else if constexpr (FP8) {
          constexpr bool E5M2 = WK == MP_W_FP8_E5M2;
          bf[hp][c] = moe_prompt_fp8<E5M2>(bw.w[c][0][hp], bw.w[c][1][hp], r2[s].x * (_Float16)(E5M2 ? 1.f : 256.f));
        } else {
          h8 v;
          if constexpr (WK == MOE_W_TABLE)
            v = moe_prompt_lut8(a.lut, bw.w[c][0][hp]);
          else
            v = moe_prompt_dq8<false>(bw.w[c][0][hp], nlo[0][s], nhi[0][s], r2[s]) * (_Float16)16.f +
                moe_prompt_dq8<false>(bw.w[c][NP - 1][hp], nlo[NP - 1][s], nhi[NP - 1][s], r2[s]);
          if constexpr (SMODE == 1) v *= (h8){r2[s].x, r2[s].x, r2[s].x, r2[s].x, r2[s].x, r2[s].x, r2[s].x, r2[s].x};
          bf[hp][c] = v;
        }
      }
    }
  };
  auto compute = [&](int buf, int g) {  // row tiles 4 g .. 4 g + 3, in pairs
    const unsigned char* img = smem + buf * MP_IMAGE;
    const float* un = unsc + buf * MP_ROWS;
#pragma unroll
    for (int rp = 2 * g; rp < 2 * g + 2; ++rp) {  // unrolled: acc stays in registers
      if (2 * rp >= nrt) break;                   // wave-uniform
      float4_t t[2][MP_CT];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int c = 0; c < MP_CT; ++c) t[u][c] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int hp = 0; hp < 4; ++hp)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const h8 af = *(const h8*)(img + (2 * rp + u) * 4096 + a_off[hp]);
#pragma unroll
          for (int c = 0; c < MP_CT; ++c) t[u][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[hp][c], t[u][c], 0, 0, 0);
        }
      // D: lane (column i16, rows 4 kq + j) of the 16 x 16 fragment
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float4_t rs = *(const float4_t*)(un + (2 * rp + u) * 16 + kq * 4);
#pragma unroll
        for (int c = 0; c < MP_CT; ++c)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[2 * rp + u][c][j] = fmaf(t[u][c][j], rs[j] * cs[c], acc[2 * rp + u][c][j]);
      }
    }
  };

  // ---- K loop: one blob tile a trip, the next tile's operands requested before this tile's MFMAs ----
  MoePromptB<SMODE, NP> b0, b1;
  load_b(0, b0);
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    stage_load(0, g);
    stage_write(0, g);
  }
  __syncthreads();
#pragma unroll 1
  for (int kt = 0; kt < a.tiles_k; ++kt) {
    const int buf = kt & 1;
    const bool more = kt + 1 < a.tiles_k;
    if (more) load_b(kt + 1, b1);
    unpack(b0);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      if (more) stage_load(kt + 1, g);
      compute(buf, g);
      if (more) stage_write(buf ^ 1, g);
    }
    __syncthreads();  // image buf ^ 1 is complete; every read of image buf is done
    if (more) b0 = b1;
  }

  // ---- epilogue ----
#pragma unroll
  for (int rt = 0; rt < 8; ++rt) {
    if (rt >= nrt) break;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = rt * 16 + kq * 4 + j;
      if (row >= R) continue;
      float* orow = a.out + (size_t)(first + row) * a.ldo;
      if constexpr (GU) {
        const float g = acc[rt][0][j], u = acc[rt][1][j];
        if constexpr (RAW) {
          if (live[0]) orow[wt * 16 + i16] = g, orow[(a.half_tiles + wt) * 16 + i16] = u;
        } else {
          if (live[0]) orow[wt * 16 + i16] = g / (1.0f + expf(-g)) * u;  // wt < half_tiles: a column inside I
        }
      } else {
#pragma unroll
        for (int c = 0; c < MP_CT; ++c) {
          const int n = (wt * MP_CT + c) * 16 + i16;
          if (live[c] && n < a.N) orow[n] = acc[rt][c][j];
        }
      }
    }
  }
}

template <bool GU, int SMODE, bool ASYM, int WK, bool RAW>
int moe_prompt_launch_one(const MoeGemmArgs& a, dim3 grid, hipStream_t st) {
  if (const int rc = allow_dynamic_lds<moe_prompt_gemm_kernel<GU, SMODE, ASYM, WK, RAW>>(MP_LDS)) return rc;
  hipLaunchKernelGGL((moe_prompt_gemm_kernel<GU, SMODE, ASYM, WK, RAW>), grid, dim3(MP_WAVES * 64), MP_LDS, st, a);
  return 0;
}
template <bool GU, int SMODE, bool ASYM, bool RAW>
int moe_prompt_launch_kind(const MoeGemmArgs& a, MoeWeightKind kind, dim3 grid, hipStream_t st) {
  if (kind == MOE_W_INT8) return moe_prompt_launch_one<GU, SMODE, ASYM, MOE_W_INT8, RAW>(a, grid, st);
  if constexpr (!ASYM) {  // moe_header_problem admits no table or fp8 blob with zero points
    if constexpr (!RAW) {  // the backward has no fused fp8 arm (woq_moe_backward refuses fp8 blobs)
      if (kind == MOE_W_FP8)
        return a.e5m2 ? moe_prompt_launch_one<GU, SMODE, false, MP_W_FP8_E5M2, false>(a, grid, st)
                      : moe_prompt_launch_one<GU, SMODE, false, MOE_W_FP8, false>(a, grid, st);
    }
    if (kind == MOE_W_TABLE) return moe_prompt_launch_one<GU, SMODE, false, MOE_W_TABLE, RAW>(a, grid, st);
  }
  if (RAW && kind == MOE_W_FP8) return fail("QBits: the raw gate/up product is not built for fp8 expert blobs");
  return moe_prompt_launch_one<GU, SMODE, ASYM, MOE_W_INT4, RAW>(a, grid, st);
}
template <bool GU, bool RAW = false>
int moe_prompt_launch_gemm(const MoeGemmArgs& a, bool smode1, bool asym, MoeWeightKind kind, dim3 grid, hipStream_t st) {
  if (!smode1)
    return asym ? moe_prompt_launch_kind<GU, 0, true, RAW>(a, kind, grid, st)
                : moe_prompt_launch_kind<GU, 0, false, RAW>(a, kind, grid, st);
  return asym ? moe_prompt_launch_kind<GU, 1, true, RAW>(a, kind, grid, st)
              : moe_prompt_launch_kind<GU, 1, false, RAW>(a, kind, grid, st);
}

// the fp16 table of a table weight type as two byte planes (what lut_quad looks up): d[0][c / 4] byte c % 4 = the low
// byte of fp16(table[c]), d[1] the high byte
LutArgs moe_prompt_lut(uint32_t weight_type) {
  static const float nf4[16] = WOQ_LUT_NF4, e2m1[16] = WOQ_LUT_FP4_E2M1, bnb[16] = WOQ_LUT_FP4_BNB;
  const float* tab = weight_type == WOQ_W_NF4 ? nf4 : (weight_type == WOQ_W_FP4_E2M1 ? e2m1 : bnb);
  LutArgs L = {};
  L.wmul = 1.f;
  for (int c = 0; c < 16; ++c) {
    const _Float16 v = (_Float16)tab[c];
    uint16_t bits;
    memcpy(&bits, &v, 2);
    L.d[0][c >> 2] |= (uint32_t)(bits & 0xffu) << (8 * (c & 3));
    L.d[1][c >> 2] |= (uint32_t)(bits >> 8) << (8 * (c & 3));
  }
  return L;
}

}  // namespace

void launch_moe_prompt_plan(const void* topk_idx, bool idx_is_int64, int S, int E, const MoeRoutePlan& p, hipStream_t st) {
  const dim3 pgrid((unsigned)p.nseg), pblock(MP_SEG);
  if (idx_is_int64)
    hipLaunchKernelGGL(moe_prompt_count_kernel<true>, pgrid, pblock, 0, st, topk_idx, S, E, p.counts, p.pos_of);
  else
    hipLaunchKernelGGL(moe_prompt_count_kernel<false>, pgrid, pblock, 0, st, topk_idx, S, E, p.counts, p.pos_of);
  hipLaunchKernelGGL(moe_prompt_scan_kernel, dim3(1), pblock, 0, st, p.nseg, E, p.counts, p.blocks, p.nblocks);
  if (idx_is_int64)
    hipLaunchKernelGGL(moe_prompt_scatter_kernel<true>, pgrid, pblock, 0, st, topk_idx, S, E, p.counts, p.sorted, p.pos_of);
  else
    hipLaunchKernelGGL(moe_prompt_scatter_kernel<false>, pgrid, pblock, 0, st, topk_idx, S, E, p.counts, p.sorted, p.pos_of);
}

int launch_moe_prompt_product(MoeRole role, const MoeCall& m, const MoeRoutePlan& p, const float* h, float* out,
                              hipStream_t st) {
  const bool gu = role != MOE_DOWN;
  const woq_blob_header& hdr = gu ? *m.gate_up_hdr : *m.down_hdr;
  MoeWeightKind kind;
  MoeGemmArgs a = moe_gemm_args(m, gu, kind);
  if (kind == MOE_W_TABLE) a.lut = moe_prompt_lut(hdr.weight_type);
  const bool smode1 = hdr.scale_mode == 1, asym = hdr.off_zp != 0;
  if (!gu) {
    moe_bind_down(a, m, p, h, out);
    const unsigned dx = (unsigned)((a.tiles_n + MP_WAVES * MP_CT - 1) / (MP_WAVES * MP_CT));
    return moe_prompt_launch_gemm<false>(a, smode1, asym, kind, dim3(dx, (unsigned)p.max_blocks), st);
  }
  const int I = m.down_hdr->K;
  moe_bind_gate_up(a, m, p, out, role == MOE_GATE_UP_RAW ? 2 * I : I);
  const dim3 grid((unsigned)((I / 16 + MP_WAVES - 1) / MP_WAVES), (unsigned)p.max_blocks);
  return role == MOE_GATE_UP_RAW ? moe_prompt_launch_gemm<true, true>(a, smode1, asym, kind, grid, st)
                                 : moe_prompt_launch_gemm<true, false>(a, smode1, asym, kind, grid, st);
}

}  // namespace woq
