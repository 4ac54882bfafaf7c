// woq_moe.hip — the routed expert block of a sparse mixture-of-experts layer over int4, nf4 / fp4, int8 and fp8 blobs:
//   out[t] = sum_j topk_w[t][j] * down_e( SiLU(gate_e x_t) * up_e x_t ),  e = topk_idx[t][j],  j = 0 .. k-1 in that order
// with E gate/up blobs (K = H, N = 2 I, columns [0, I) gate and [I, 2 I) up) and E down blobs (K = I, N = H), each kind
// at one uniform byte stride and under one header. The definition is HF's MixtralExperts / Qwen3MoeExperts forward (a
// one-hot mask, nonzero() on the host, two F.linear and an index_add_ per hit expert); an id outside [0, E) drops its
// slot there and here.
//
// Four launches whose shapes depend on (T, k, E, H, I) alone — the routing never reaches the host:
//  1. plan (one workgroup): histogram of the ids over experts in LDS, exclusive scan, a STABLE scatter of the slot ids
//     s = t k + j into expert order (sorted[], and its inverse pos_of[], -1 for a dropped slot), and a table of blocks
//     {expert, first sorted slot, rows <= 16} with its count. The count is not known to the host, so launches 2 and 3
//     size their grids for the bound ceil(T k / 16) + min(E, T k) and a workgroup past the count returns.
//  2. gate/up: a workgroup = one block of <= 16 rows x one pair of 16-column tiles (gate tile tn, up tile tn + I / 16).
//  3. down: the same inner loop with K = I, one 16-column tile per workgroup, fp32 rows y[sorted slot][H].
//  4. combine: out[t][n] = sum_j w[t][j] y[pos_of[t k + j]][n], j ascending, rounded once to the output type.
// No floating-point atomics and a fixed summation order everywhere: the same inputs give the same bytes.
//
// The inner loop (2 and 3). The blob tile is the B fragment of v_mfma_i32_16x16x64_i8 (include/woq_blob.h) and int4_b
// makes the operand in three VALU instructions. The A operand is woq_gemv_i8.hip's: an activation row becomes the exact
// 22-bit + sign fixed point relative to its maximum, carried as three int8 limb rows plus a ones row — four activation
// rows per MFMA row set, four row sets per block. K is walked in chunks of 1024 (8 tiles): the workgroup stages the
// chunk of its <= 16 rows as limbs in LDS (wave w: rows w, w + 4, ...; a row's fixed-point scale is per chunk, so an
// I of 14336 never has to fit at once), then its four waves interleave over the chunk's tiles (wave w: tiles w, w + 4).
// A wave requests its two tiles' weight words before the staging, so they fly under it; each tile's words are loaded once
// and meet all row sets. Per-group scales (and zero points: sum_k (q - zp) x = sum_k q x - zp sum_k x, the second sum
// from an MFMA against ones) are applied in fp32 after limb_combine, per tile (scale_mode 0) or per 32-k block
// (scale_mode 1: each 64-k MFMA is issued twice, the other 32-k half's A operand read from a block of zeros). The
// waves' partial sums meet in LDS and are added in wave order. fp8 blobs take launches 2 and 3 through a kernel of their
// own on the fp8 MFMA, moe_fp8_gemm_kernel below.
//
// Also here, the host front of both forms (this one, MOE_GROUPED, and woq_moe_prompt.hip's MOE_PROMPT): the workspace
// layout (moe_layout), the argument builder and role binders of the products (woq_moe.h), the forward driver
// (launch_moe_forward) and the checks of the three entry points (moe_entry_checks; the backward's is woq_moe_bwd.hip).
#include <math.h>

#include <algorithm>
#include <string>

#include "woq_moe.h"

namespace woq {
namespace {

constexpr int MOE_KC = 1024;              // k per staged chunk
constexpr int MOE_TPC = MOE_KC / 128;     // weight tiles per chunk
constexpr int MOE_RB = MOE_KC + 16;       // bytes of a limb row in LDS (+16: rows on distinct banks)
constexpr int MOE_WAVES = 4;
constexpr int MOE_TPW = MOE_TPC / MOE_WAVES;  // tiles of a chunk per wave
constexpr int MOE_PLAN_THREADS = 1024;

// ---- 1. plan ---------------------------------------------------------------------------------------------------------
template <bool IDX64>
__global__ __launch_bounds__(MOE_PLAN_THREADS) void moe_plan_kernel(const void* __restrict__ topk_idx, int S, int E,
                                                                    int32_t* __restrict__ sorted,
                                                                    int32_t* __restrict__ pos_of,
                                                                    MoeBlock* __restrict__ blocks,
                                                                    int32_t* __restrict__ nblocks) {
  __shared__ int32_t ids[MOE_MAX_SLOTS];
  __shared__ int32_t cnt[MOE_MAX_EXPERTS], off[MOE_MAX_EXPERTS];
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int e = tid; e < E; e += nthr) cnt[e] = 0;
  __syncthreads();
  for (int s = tid; s < S; s += nthr) {
    const int e = moe_slot_id<IDX64>(topk_idx, s, E);
    ids[s] = e;
    if (e >= 0)
      atomicAdd(&cnt[e], 1);  // an integer count: the result does not depend on the order
    else
      pos_of[s] = -1;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0, nb = 0;
    for (int e = 0; e < E; ++e) {
      const int c = cnt[e];
      off[e] = run;
      for (int r = 0; r < c; r += MOE_BLOCK_ROWS) blocks[nb++] = MoeBlock{e, run + r, min(MOE_BLOCK_ROWS, c - r), 0};
      run += c;
    }
    *nblocks = nb;
  }
  __syncthreads();
  // stable: expert e's thread walks the slots in ascending order (every thread reads the same LDS word: a broadcast)
  for (int e = tid; e < E; e += nthr) {
    if (cnt[e] == 0) continue;
    int p = off[e];
    for (int s = 0; s < S; ++s) {
      if (ids[s] == e) {
        sorted[p] = s;
        pos_of[s] = p;
        ++p;
      }
    }
  }
}

// ---- 2 / 3. the grouped product --------------------------------------------------------------------------------------
__device__ __forceinline__ float moe_scale(const void* s, size_t i, int st) {
  if (st == WOQ_F32) return ((const float*)s)[i];
  const uint16_t b = ((const uint16_t*)s)[i];
  return st == WOQ_BF16 ? bf16_bits_to_f32(b) : f16_bits_to_f32(b);
}

constexpr int MOE_WK_INT8 = 4, MOE_WK_FP8 = 5;  // (fp8: moe_fp8_gemm_kernel below)

// What moe_gemm_kernel and moe_fp8_gemm_kernel share: the staging of an activation row up to its gathered fixed-point
// bytes. Their block prologues, chunk prefetches and cross-wave sums are written out in each: as shared functions they
// cost the gate/up launches registers (profiles/r28_moe_refactor.txt).
// Row m of the block, k0 .. k0 + 1023 of it, as fp32: lane l holds k0 + 256 j + 4 l .. + 3 in xv[j]. GU: the row of
// a.x (of x_dtype) of the slot's token; else the slot's own fp32 row. Buffer loads return zero past the xlen elements
// that lie inside K: that is what keeps the padding out of the sums
template <bool GU>
__device__ __forceinline__ void moe_load_row(const MoeGemmArgs& a, int first, int m, int k0, int xlen, int lane,
                                             float4_t (&xv)[4]) {
  const int src = GU ? __builtin_amdgcn_readfirstlane(a.sorted[first + m]) / a.top_k : first + m;
  const size_t row_off = (size_t)src * a.ldx + k0;
  if (GU && a.x_dtype != WOQ_F32) {
    const rsrc_t rx = make_rsrc((const uint16_t*)a.x + row_off, xlen * 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint2 r = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rx, lane * 8 + j * 512, 0, 0));
      const uint16_t hb[4] = {(uint16_t)r.x, (uint16_t)(r.x >> 16), (uint16_t)r.y, (uint16_t)(r.y >> 16)};
      float f[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float fb = bf16_bits_to_f32(hb[i]), fh = f16_bits_to_f32(hb[i]);
        f[i] = a.x_dtype == WOQ_BF16 ? fb : fh;
      }
      xv[j] = (float4_t){f[0], f[1], f[2], f[3]};
    }
  } else {
    const rsrc_t rx = make_rsrc((const float*)a.x + row_off, xlen * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      xv[j] = __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(rx, lane * 16 + j * 1024, 0, 0));
  }
}

// The exponent e of a staged row: amax < 2^e  =>  |x| * 2^(21 - e) < 2^21, so that the fp32 sum with 1.5 * 2^23 stays
// inside [2^23, 2^24), where ulp = 1, and its mantissa IS round(x * 2^(21 - e)) + 2^22 (offset binary, 22 bits + sign)
__device__ __forceinline__ int moe_row_exponent(const float4_t (&xv)[4]) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    amax = fmaxf(fmaxf(amax, fabsf(xv[j].x)), fmaxf(fabsf(xv[j].y), fmaxf(fabsf(xv[j].z), fabsf(xv[j].w))));
  amax = wave_max_dpp(amax);
  int e = 0;
  if (amax > 0.f && amax < INFINITY) e = max(-100, min(100, __builtin_amdgcn_frexp_expf(amax)));
  return e;
}
// wb[n] = byte n of the four values' bits fl32(x * sfix + 1.5 * 2^23) + OFF, sfix = 2^(21 - e), gathered into one word:
// v_perm_b32(hi, lo, sel) picks bytes of {hi:lo}, 0x0c = zero
template <uint32_t OFF>
__device__ __forceinline__ void moe_fixed_bytes(float4_t x, float sfix, uint32_t (&wb)[3]) {
  const uint32_t va = __float_as_uint(fmaf(x.x, sfix, 12582912.f)) + OFF;
  const uint32_t vb = __float_as_uint(fmaf(x.y, sfix, 12582912.f)) + OFF;
  const uint32_t vc = __float_as_uint(fmaf(x.z, sfix, 12582912.f)) + OFF;
  const uint32_t vd = __float_as_uint(fmaf(x.w, sfix, 12582912.f)) + OFF;
  wb[0] = __builtin_amdgcn_perm(vb, va, 0x0c0c0400u) | __builtin_amdgcn_perm(vd, vc, 0x04000c0cu);
  wb[1] = __builtin_amdgcn_perm(vb, va, 0x0c0c0501u) | __builtin_amdgcn_perm(vd, vc, 0x05010c0cu);
  wb[2] = __builtin_amdgcn_perm(vb, va, 0x0c0c0602u) | __builtin_amdgcn_perm(vd, vc, 0x06020c0cu);
}

// GU: the gate/up launch (two column tiles, SiLU * mul epilogue, rows gathered by token) | the down launch
// WK, the weight kind: 0 = int4 | 1, 2, 3 = a table type (nf4 / fp4) as that many digit planes | MOE_WK_INT8 = the int8
// composite. Only the B operand differs:
//   table  the nibbles are codes: lut_b turns a 64-k half into NDIG int8 digit operands, one MFMA per plane against the
//          same A operand, f = f0 + 2^8 f1 + 2^16 f2 after limb_combine, LutArgs::wmul folded into the scale. The digit
//          operands do not depend on the row set, so here the tile loop is the OUTER one: they are built once per tile,
//          column tile and half, just before the MFMAs of all live row sets, and only the weight words stay resident.
//   int8   both planes' words of a tile are requested together; both meet the same A registers and the two int32
//          fragments are added as 16 hi + lo BEFORE limb_combine (exact: a limb sum is below 2^21, 17 of them below
//          2^26), so a tile costs the fp32 roundings of an int4 tile. The zero points 16 zhi + zlo enter through the ones
//          row as one integer: the LO plane always carries one, the HI plane only under ASYM.
template <bool GU, int SMODE, bool ASYM, int WK>
__global__ __launch_bounds__(MOE_WAVES * 64) void moe_gemm_kernel(const MoeGemmArgs a) {
  constexpr int CB = GU ? 2 : 1;
  constexpr int NS = SMODE == 1 ? 4 : 1;  // scales of a tile and column
  constexpr int NDIG = WK >= 1 && WK <= 3 ? WK : 0;
  constexpr bool I8 = WK == MOE_WK_INT8;
  constexpr int NP = I8 ? 2 : 1;         // nibble planes
  constexpr bool ZP = ASYM || I8;        // a zero-point term through the ones row
  static_assert(!(NDIG > 0 && ASYM), "the table types are symmetric");
  __shared__ __attribute__((aligned(16))) unsigned char strip[MOE_BLOCK_ROWS * 3 * MOE_RB];  // [row][limb][MOE_RB]
  __shared__ __attribute__((aligned(16))) unsigned char zero_blk[64], ones_blk[64];
  __shared__ float unsc_s[MOE_BLOCK_ROWS];  // per row: 2^(e - 25) of the staged chunk
  __shared__ float slab[MOE_WAVES][4][CB][64];

  const int b = (int)blockIdx.y;
  if (b >= *a.nblocks) return;
  const MoeBlock blk = a.blocks[b];
  const int expert = __builtin_amdgcn_readfirstlane(blk.expert), first = __builtin_amdgcn_readfirstlane(blk.first);
  const int R = __builtin_amdgcn_readfirstlane(blk.rows);
  const int nrs = (R + 3) >> 2;  // live row sets
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;
  if (tid < 16) {
    ((uint32_t*)zero_blk)[tid] = 0u;
    ((uint32_t*)ones_blk)[tid] = 0x01010101u;
    unsc_s[tid] = 0.f;
  }

  const uint8_t* blob = a.blobs + (size_t)expert * a.stride;
  const u32x4* q[NP];
  const uint8_t* zps[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) q[p] = (const u32x4*)(blob + a.off_q[p]), zps[p] = blob + a.off_zp[p];
  const void* scales = blob + a.off_scale;
  int tn[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) tn[cb] = (int)blockIdx.x + cb * a.half_tiles;

  float acc[4][CB];
#pragma unroll
  for (int rs = 0; rs < 4; ++rs)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[rs][cb] = 0.f;
  const i32x4 izero = {0, 0, 0, 0};
  const i32x4 b_ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
  const int a_m = i16 >> 2, a_part = i16 & 3;

  const int nchunks = (a.tiles_k + MOE_TPC - 1) / MOE_TPC;
#pragma unroll 1
  for (int c = 0; c < nchunks; ++c) {
    // ---- this wave's tiles of the chunk: weight words, scales, zero points — requested before the staging ----
    u32x4 w[MOE_TPW][CB][NP];
    float sc[MOE_TPW][CB][NS];
    int uz[MOE_TPW][CB][NS];  // zero point + 8; int8: 16 zhi + zlo + 8, the composite's zero point in LO-plane units
auto load_qparams = [&](int ti, int cb, int s, size_t si) {
      sc[ti][cb][s] = moe_scale(scales, si, a.scale_type);
      if constexpr (NDIG > 0) sc[ti][cb][s] *= a.lut.wmul;
      if constexpr (I8)
        uz[ti][cb][s] = 16 * ((ASYM ? (int)zps[0][si] : 8) - 8) + (int)zps[1][si];
      else if constexpr (ASYM)
        uz[ti][cb][s] = (int)zps[0][si];
    };
#pragma unroll
    for (int ti = 0; ti < MOE_TPW; ++ti) {
      const int kt = c * MOE_TPC + wid + ti * MOE_WAVES;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
        for (int p = 0; p < NP; ++p) w[ti][cb][p] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int s = 0; s < NS; ++s) sc[ti][cb][s] = 0.f, uz[ti][cb][s] = 8;
        if (kt >= a.tiles_k) continue;
#pragma unroll
        for (int p = 0; p < NP; ++p)
          w[ti][cb][p] = __builtin_nontemporal_load(q[p] + ((size_t)tn[cb] * a.tiles_k + kt) * 64 + lane);
        if constexpr (SMODE == 0) {
          const int grp = a.n_groups == 1 ? 0 : min(kt * 128 / a.group, a.n_groups - 1);
          load_qparams(ti, cb, 0, ((size_t)tn[cb] * a.n_groups + grp) * 16 + i16);
        } else {
          const size_t si = (((size_t)tn[cb] * a.tiles_k + kt) * 16 + i16) * 4;
#pragma unroll
          for (int s = 0; s < 4; ++s) load_qparams(ti, cb, s, si + s);
        }
      }
    }

    // ---- stage the chunk of the block's rows as limbs (stage_row of woq_gemv_i8.hip, XJ = 4) ----
    __syncthreads();  // the previous chunk's operand reads (first chunk: the constant blocks' stores) are done
    const int k0 = c * MOE_KC;
    const int xlen = max(0, min(MOE_KC, a.K - k0));
    for (int m = wid; m < R; m += MOE_WAVES) {
      float4_t xv[4];
      moe_load_row<GU>(a, first, m, k0, xlen, lane, xv);
      const int e = moe_row_exponent(xv);
      const float sfix = ldexpf(1.f, 21 - e);
      if (lane == 0) unsc_s[m] = ldexpf(1.f, e - 25);  // undoes the fixed-point scale and the 16 * q weight bytes
      unsigned char* r0 = strip + (size_t)(3 * m) * MOE_RB + lane * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t wb[3];
        moe_fixed_bytes<0u>(xv[j], sfix, wb);
        *(uint32_t*)(r0 + j * 256) = wb[0] ^ 0x80808080u;           // limb 0: b0 - 128
        *(uint32_t*)(r0 + MOE_RB + j * 256) = wb[1] ^ 0x80808080u;  // limb 1: b1 - 128
        *(uint32_t*)(r0 + 2 * MOE_RB + j * 256) = wb[2];            // limb 2: b2 in [0, 127]
      }
    }
    __syncthreads();

    // ---- inner products: MFMA row r = lane & 15 -> activation row (r >> 2) of the set, part r & 3 (limb 0..2 | ones);
    // D: lane quarter kq holds activation row kq of the set for column lane & 15 ----
    // this lane's A operand of row set rs: tile tt's first half at a_base + tt * st_t, its second st_h further
    auto a_operand = [&](int rs, const unsigned char*& a_base, int& st_t, int& st_h) {
      const int row_a = 4 * rs + a_m;
      const bool a_live = row_a < R;
      const bool a_data = a_live && a_part != 3;
      a_base = !a_live ? zero_blk + kq * 16
                       : (a_part == 3 ? ones_blk + kq * 16 : strip + (size_t)(3 * row_a + a_part) * MOE_RB + kq * 16);
      st_t = a_data ? 128 : 0, st_h = a_data ? 64 : 0;
    };
    // f0 + 2^8 f1 + 2^16 f2 of one A operand against the digit operands, most significant plane first
    auto digit_dot = [&](const i32x4& av, const i32x4 (&bd)[NDIG > 0 ? NDIG : 1], i32x4 (&d)[NDIG > 0 ? NDIG : 1],
                         bool add) {
#pragma unroll
      for (int j = 0; j < NDIG; ++j) d[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bd[j], add ? d[j] : izero, 0, 0, 0);
    };
    auto digit_sum = [&](const i32x4 (&d)[NDIG > 0 ? NDIG : 1]) {
      float f = limb_combine(d[NDIG > 0 ? NDIG - 1 : 0]);
#pragma unroll
      for (int j = NDIG - 2; j >= 0; --j) f = fmaf(f, 256.f, limb_combine(d[j]));
      return f;
    };
    if constexpr (NDIG > 0) {
#pragma unroll
      for (int ti = 0; ti < MOE_TPW; ++ti) {
        const int tt = wid + ti * MOE_WAVES;  // tile of the chunk
        if (c * MOE_TPC + tt >= a.tiles_k) continue;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          const u32x4 wv = w[ti][cb][0];
          if constexpr (SMODE == 0) {
            i32x4 b0[NDIG], b1[NDIG];
            lut_b<NDIG>(a.lut, wv.x, wv.y, b0);
            lut_b<NDIG>(a.lut, wv.z, wv.w, b1);
#pragma unroll
            for (int rs = 0; rs < 4; ++rs) {
              if (rs >= nrs) break;
              const unsigned char* a_base;
              int st_t, st_h;
              a_operand(rs, a_base, st_t, st_h);
              i32x4 d[NDIG];
              digit_dot(*(const i32x4*)(a_base + tt * st_t), b0, d, false);
              digit_dot(*(const i32x4*)(a_base + tt * st_t + st_h), b1, d, true);
              acc[rs][cb] = fmaf(sc[ti][cb][0] * unsc_s[4 * rs + kq], digit_sum(d), acc[rs][cb]);
            }
          } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              i32x4 bq[NDIG];
              lut_b<NDIG>(a.lut, h == 0 ? wv.x : wv.z, h == 0 ? wv.y : wv.w, bq);
#pragma unroll
              for (int rs = 0; rs < 4; ++rs) {
                if (rs >= nrs) break;
                const unsigned char* a_base;
                int st_t, st_h;
                a_operand(rs, a_base, st_t, st_h);
                const float un = unsc_s[4 * rs + kq];
#pragma unroll
                for (int g2 = 0; g2 < 2; ++g2) {  // lanes kq < 2 feed the half's first 32-k block, kq >= 2 its second
                  const bool mine = (kq < 2) == (g2 == 0);
                  const unsigned char* ap = mine ? a_base + tt * st_t + h * st_h : zero_blk;
                  i32x4 d[NDIG];
                  digit_dot(*(const i32x4*)ap, bq, d, false);
                  acc[rs][cb] = fmaf(sc[ti][cb][2 * h + g2] * un, digit_sum(d), acc[rs][cb]);
                }
              }
            }
          }
        }
      }
    } else {
#pragma unroll
      for (int rs = 0; rs < 4; ++rs) {  // unrolled: acc[rs] stays in registers
        if (rs >= nrs) break;
        const unsigned char* a_base;
        int st_t, st_h;
        a_operand(rs, a_base, st_t, st_h);
        const float un = unsc_s[4 * rs + kq];
#pragma unroll
        for (int ti = 0; ti < MOE_TPW; ++ti) {
          const int tt = wid + ti * MOE_WAVES;  // tile of the chunk
          if (c * MOE_TPC + tt >= a.tiles_k) continue;
          if constexpr (SMODE == 0) {
            const i32x4 a0 = *(const i32x4*)(a_base + tt * st_t);
            const i32x4 a1 = *(const i32x4*)(a_base + tt * st_t + st_h);
            float sx = 0.f;  // sum_k x~_k of this tile (zero points only), in fixed-point units
            if constexpr (ZP) {
              i32x4 ds = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b_ones, izero, 0, 0, 0);
              ds = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b_ones, ds, 0, 0, 0);
              sx = limb_combine(ds);
            }
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
              i32x4 d[NP];
#pragma unroll
              for (int p = 0; p < NP; ++p) {
                const u32x4 wv = w[ti][cb][p];
                i32x4 b0, b1;
                int4_b(wv.x, wv.y, b0);
                int4_b(wv.z, wv.w, b1);
                d[p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0, izero, 0, 0, 0);
                d[p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1, d[p], 0, 0, 0);
              }
              if constexpr (I8) d[0] = d[0] * 16 + d[1];  // 16 hi + lo
              float f = limb_combine(d[0]);
              // b_ones carries 1 where the weights carry 16 * q: the zero point enters as 16 * zp
              if constexpr (ZP) f = fmaf(-16.f * (float)(uz[ti][cb][0] - 8), sx, f);
              acc[rs][cb] = fmaf(sc[ti][cb][0] * un, f, acc[rs][cb]);
            }
          } else {
            // the two 32-k halves of a 64-k MFMA belong to different groups: lanes kq < 2 feed the first, kq >= 2 the second
            const unsigned char* a_lo = kq < 2 ? a_base : zero_blk;
            const unsigned char* a_hi = kq < 2 ? zero_blk : a_base;
            const int lo_t = kq < 2 ? st_t : 0, lo_h = kq < 2 ? st_h : 0;
            const int hi_t = kq < 2 ? 0 : st_t, hi_h = kq < 2 ? 0 : st_h;
            i32x4 al[2], ah[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              al[h] = *(const i32x4*)(a_lo + tt * lo_t + h * lo_h);
              ah[h] = *(const i32x4*)(a_hi + tt * hi_t + h * hi_h);
            }
            float sx[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (ZP) {
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                sx[2 * h] = limb_combine(__builtin_amdgcn_mfma_i32_16x16x64_i8(al[h], b_ones, izero, 0, 0, 0));
                sx[2 * h + 1] = limb_combine(__builtin_amdgcn_mfma_i32_16x16x64_i8(ah[h], b_ones, izero, 0, 0, 0));
              }
            }
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                i32x4 bq[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                  const u32x4 wv = w[ti][cb][p];
                  int4_b(h == 0 ? wv.x : wv.z, h == 0 ? wv.y : wv.w, bq[p]);
                }
#pragma unroll
                for (int g2 = 0; g2 < 2; ++g2) {
                  const int s = 2 * h + g2;  // 32-k block of the tile
                  i32x4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(g2 == 0 ? al[h] : ah[h], bq[0], izero, 0, 0, 0);
                  if constexpr (I8)  // 16 hi + lo
                    d = d * 16 + __builtin_amdgcn_mfma_i32_16x16x64_i8(g2 == 0 ? al[h] : ah[h], bq[1], izero, 0, 0, 0);
                  float f = limb_combine(d);
                  if constexpr (ZP) f = fmaf(-16.f * (float)(uz[ti][cb][s] - 8), sx[s], f);
                  acc[rs][cb] = fmaf(sc[ti][cb][s] * un, f, acc[rs][cb]);
                }
              }
            }
          }
        }
      }
    }
  }

  // ---- the waves' partial sums, added in wave order; epilogue ----
#pragma unroll
  for (int rs = 0; rs < 4; ++rs)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) slab[wid][rs][cb][lane] = acc[rs][cb];
  __syncthreads();
  const int row = tid >> 4, col = tid & 15;
  if (row >= R) return;
  const int e_rs = row >> 2, e_l = (row & 3) * 16 + col;
  float v[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    v[cb] = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < MOE_WAVES; ++w2) v[cb] += slab[w2][e_rs][cb][e_l];
  }
  const int n = (int)blockIdx.x * 16 + col;
  if constexpr (GU) {
    a.out[(size_t)(first + row) * a.ldo + n] = v[0] / (1.0f + expf(-v[0])) * v[CB - 1];  // n < I: I % 16 == 0
  } else {
    if (n < a.N) a.out[(size_t)(first + row) * a.ldo + n] = v[0];
  }
}

// ---- 2 / 3 for fp8 expert blobs: the grouped product on the fp8 matrix cores -------------------------------------------
// w = value(code) * scale with an 8-bit float code (e4m3 / e5m2): the int8 route above does not apply, the code byte is
// no integer. v_mfma_f32_16x16x32_fp8_fp8 / _fp8_bf8 reads it as it is (woq_gemv_fp8.hip states the arithmetic): the
// B operand is code = (hi << 4) | (lo ^ 8) of the composite's two nibble planes, about one VALU per weight; the A operand
// is the activation as SIX balanced base-16 digits d_j in [-8, 7] of v = round(x 2^(21 - e)), e per row and 1024-k
// chunk, each an exact e4m3 value; every product is exact, the sums run in the MFMA's fp32 accumulator and
// sum_j 16^j S_j is taken in fp32. The work split is moe_gemm_kernel's: a workgroup = one table block x one 16-column
// tile (gate/up: the pair tn, tn + I / 16), four waves interleaved over the tiles of a chunk, weight words requested
// before the staging and fetched once per workgroup, partial sums added in wave order.
//   Staging. u = v + 0x888888 has the nibbles d_j + 8 (a balanced digit is a plain digit of the number shifted by
// eight in every place), and u is one integer add away from the bits of fl32(x 2^(21 - e) + 1.5 2^23). Byte n of four
// neighbouring u's is gathered into one word by v_perm_b32, and its low / high nibbles go through a 16-entry byte table
// (lut_quad: nibble -> the e4m3 byte of nibble - 8): about 11 VALU per activation for all six digits, against about 30
// for the convert-and-pack form of the dense GEMV. Digit rows lie in LDS as [row][digit][MOE_RB].
//   Row-set packing, chosen wave-uniformly from the block's row count R:
//     R <= 2  (decode) the GEMV's: MFMA row r = 6 m + j holds digit j of row m, ONE MFMA pair per 32 k and column tile;
//             the six digit sums of a row sit in two lane quarters and are weighted by 16^j 2^(e - 21) and summed over
//             the quarters once, after the last chunk.
//     R > 2   row set j holds digit j of all 16 rows: six MFMA pairs per 32 k, no idle MFMA row at R = 16, and the
//             recombination is lane-local over six accumulator fragments. With [row][digit] rows of 1040 B the sixteen
//             lanes of a quarter read 16 B at a stride of 6240 B: 4 (6 i + kq) mod 64 covers every bank four times, the
//             minimum for a 1 KB request.
//     One row under the second packing would issue six MFMA pairs where one does: the launch would be bound by the
//     matrix pipe, not by the weight stream, which is why decode blocks keep the first (not measured: the second
//     packing was never run at R <= 2).
//   LDS is dynamic: one zero row + 6 min(16, T k) digit rows of 1040 B, the attribute set once for the 16-row maximum
//   (100880 B + 8.3 KB static: one workgroup of four waves per CU). A decode call asks for what its rows need — T k = 2:
//   13.5 KB; T k = 8: 51 KB — and keeps the two workgroups per CU that the kernel's registers allow (138 - 190 VGPRs +
//   up to 48 accumulation registers: two waves per SIMD).
//   Scales: scale_mode 0 per tile in fp32 after the recombination; scale_mode 1 as woq_gemv_fp8.hip: each 64-k half is
//   issued once per 32-k block with the other block's two lane quarters reading the zero row, at the same offsets.
//   Dead MFMA rows read the zero row too (digit byte 0 = +0.0), buffer loads return zero past K, tiles past tiles_k are
//   skipped: nothing but the block's own rows and the slice's own k reaches an accumulator.
typedef long i64_t;
constexpr int MOE_F8_DIG = 6;
constexpr int moe_fp8_lds_bytes(int rows) { return (1 + MOE_F8_DIG * rows) * MOE_RB; }

template <bool E5M2>
__device__ __forceinline__ float4_t moe_mfma_f8(i64_t a, i64_t b, float4_t c) {
  if constexpr (E5M2)
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_bf8(a, b, c, 0, 0, 0);  // A: e4m3 digits, B: e5m2 codes
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
}
// the 16 code bytes of one lane and 64-k half; k order of a dword pair: low nibbles, high nibbles (woq_blob.h)
__device__ __forceinline__ void moe_fp8_codes(uint32_t h0, uint32_t h1, uint32_t l0, uint32_t l1, i64_t& bq0, i64_t& bq1) {
  const uint32_t b0 = ((h0 & 0x0f0f0f0fu) << 4) | ((l0 & 0x0f0f0f0fu) ^ 0x08080808u);
  const uint32_t b1 = (h0 & 0xf0f0f0f0u) | (((l0 >> 4) & 0x0f0f0f0fu) ^ 0x08080808u);
  const uint32_t b2 = ((h1 & 0x0f0f0f0fu) << 4) | ((l1 & 0x0f0f0f0fu) ^ 0x08080808u);
  const uint32_t b3 = (h1 & 0xf0f0f0f0u) | (((l1 >> 4) & 0x0f0f0f0fu) ^ 0x08080808u);
  bq0 = (i64_t)(((unsigned long)b1 << 32) | b0), bq1 = (i64_t)(((unsigned long)b3 << 32) | b2);
}
// the codes of 64-k half h of one tile, from its two planes' words w[cb][0 | 1], for every column tile
template <int CB>
__device__ __forceinline__ void moe_fp8_tile_codes(const u32x4 (&w)[CB][2], int h, i64_t (&bq0)[CB], i64_t (&bq1)[CB]) {
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const u32x4 wh = w[cb][0], wl = w[cb][1];
    moe_fp8_codes(h == 0 ? wh.x : wh.z, h == 0 ? wh.y : wh.w, h == 0 ? wl.x : wl.z, h == 0 ? wl.y : wl.w, bq0[cb], bq1[cb]);
  }
}
// a lane's 16 digit bytes at p as the A operands of the two 32-k MFMAs of a 64-k half
__device__ __forceinline__ void moe_fp8_a(const unsigned char* p, i64_t& a_lo, i64_t& a_hi) {
  const u32x4 av = *(const u32x4*)p;
  a_lo = (i64_t)(((unsigned long)av.y << 32) | av.x), a_hi = (i64_t)(((unsigned long)av.w << 32) | av.z);
}

template <bool GU, int SMODE, bool E5M2>
__global__ __launch_bounds__(MOE_WAVES * 64) void moe_fp8_gemm_kernel(const MoeGemmArgs a) {
  constexpr int CB = GU ? 2 : 1;
  constexpr int NS = SMODE == 1 ? 4 : 1;
  constexpr int ND = MOE_F8_DIG;
  extern __shared__ __attribute__((aligned(16))) unsigned char f8_lds[];  // [zero row][row][digit][MOE_RB]
  __shared__ __attribute__((aligned(16))) float unsc_s[MOE_BLOCK_ROWS];  // per row: 2^(e - 21) of the staged chunk
  __shared__ float slab[MOE_WAVES][CB][MOE_BLOCK_ROWS][16];
  unsigned char* zrow = f8_lds;
  unsigned char* strip = f8_lds + MOE_RB;

  const int b = (int)blockIdx.y;
  if (b >= *a.nblocks) return;
  const MoeBlock blk = a.blocks[b];
  const int expert = __builtin_amdgcn_readfirstlane(blk.expert), first = __builtin_amdgcn_readfirstlane(blk.first);
  const int R = min(__builtin_amdgcn_readfirstlane(blk.rows), a.lds_rows);  // (a block has at most min(16, T k) rows)
  const bool pair = R <= 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;
  for (int j = tid; j < MOE_RB / 4; j += MOE_WAVES * 64) ((uint32_t*)zrow)[j] = 0u;
  if (tid < MOE_BLOCK_ROWS) unsc_s[tid] = 0.f;

  const uint8_t* blob = a.blobs + (size_t)expert * a.stride;
  const u32x4* q[2] = {(const u32x4*)(blob + a.off_q[0]), (const u32x4*)(blob + a.off_q[1])};
  const void* scales = blob + a.off_scale;
  int tn[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) tn[cb] = (int)blockIdx.x + cb * a.half_tiles;

  // nibble n -> the e4m3 byte of n - 8: -8 .. -1 = d0 ce cc ca c8 c4 c0 b8, 0 .. 7 = 00 38 40 44 48 4a 4c 4e
  const LutArgs dig = {{{0xcacccED0u, 0xb8c0c4c8u, 0x44403800u, 0x4e4c4a48u}, {0, 0, 0, 0}, {0, 0, 0, 0}}, 1.f};

  // this lane's A operand: the strip row of MFMA row i16 (digit 0 under the second packing, whose digit j lies
  // `dstep` * j further), or the zero row; both at + kq * 16, so that tile and half offsets are immediates
  const bool a_live = pair ? i16 < ND * R : i16 < R;
  const unsigned char* a_row = (a_live ? strip + (size_t)(pair ? i16 : ND * i16) * MOE_RB : zrow) + kq * 16;
  const int dstep = a_live ? MOE_RB : 0;
  const unsigned char* z_row = zrow + kq * 16;
  // scale_mode 1: 32-k block g of a half = lane quarters 2 g, 2 g + 1
  const unsigned char* a_blk[2] = {kq < 2 ? a_row : z_row, kq < 2 ? z_row : a_row};
  const int d_blk[2] = {kq < 2 ? dstep : 0, kq < 2 ? 0 : dstep};

  float acc[4][CB];    // second packing: rows 4 kq + i of column i16
  float tot[2][CB];    // first packing: rows 0, 1 of column i16, this lane quarter's digits
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    tot[0][cb] = tot[1][cb] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][cb] = 0.f;
  }
  const float4_t fzero = {0.f, 0.f, 0.f, 0.f};

  const int nchunks = (a.tiles_k + MOE_TPC - 1) / MOE_TPC;
#pragma unroll 1
  for (int c = 0; c < nchunks; ++c) {
    // ---- this wave's tiles of the chunk: both planes' words and the scales, requested before the staging ----
    u32x4 w[MOE_TPW][CB][2];
    float sc[MOE_TPW][CB][NS];
#pragma unroll
    for (int ti = 0; ti < MOE_TPW; ++ti) {
      const int kt = c * MOE_TPC + wid + ti * MOE_WAVES;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        w[ti][cb][0] = w[ti][cb][1] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int s = 0; s < NS; ++s) sc[ti][cb][s] = 0.f;
        if (kt >= a.tiles_k) continue;
#pragma unroll
        for (int p = 0; p < 2; ++p)
          w[ti][cb][p] = __builtin_nontemporal_load(q[p] + ((size_t)tn[cb] * a.tiles_k + kt) * 64 + lane);
        if constexpr (SMODE == 0) {
          const int grp = a.n_groups == 1 ? 0 : min(kt * 128 / a.group, a.n_groups - 1);
          sc[ti][cb][0] = moe_scale(scales, ((size_t)tn[cb] * a.n_groups + grp) * 16 + i16, a.scale_type);
        } else {
          const size_t si = (((size_t)tn[cb] * a.tiles_k + kt) * 16 + i16) * 4;
#pragma unroll
          for (int s = 0; s < 4; ++s) sc[ti][cb][s] = moe_scale(scales, si + s, a.scale_type);
        }
      }
    }

    // ---- stage the chunk of the block's rows as digit rows ----
    __syncthreads();  // the previous chunk's operand reads (first chunk: the zero row's stores) are done
    const int k0 = c * MOE_KC;
    const int xlen = max(0, min(MOE_KC, a.K - k0));
    for (int m = wid; m < R; m += MOE_WAVES) {
      float4_t xv[4];
      moe_load_row<GU>(a, first, m, k0, xlen, lane, xv);
      const int e = moe_row_exponent(xv);
      const float sfix = ldexpf(1.f, 21 - e);
      if (lane == 0) unsc_s[m] = ldexpf(1.f, e - 21);
      unsigned char* r0 = strip + (size_t)(ND * m) * MOE_RB + lane * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // the bits of the fixed-point sum are 0x4B000000 + v + 2^22; + 0x488888 - 0x4B000000 leaves u = v + 0x888888 < 2^24
        uint32_t wb[3];
        moe_fixed_bytes<0x00488888u - 0x4B000000u>(xv[j], sfix, wb);
#pragma unroll
        for (int n = 0; n < 3; ++n) {
          uint32_t lo[1], hi[1];
          lut_quad<1>(dig, wb[n] & 0x0f0f0f0fu, lo);
          lut_quad<1>(dig, (wb[n] >> 4) & 0x0f0f0f0fu, hi);
          *(uint32_t*)(r0 + (size_t)(2 * n) * MOE_RB + j * 256) = lo[0];
          *(uint32_t*)(r0 + (size_t)(2 * n + 1) * MOE_RB + j * 256) = hi[0];
        }
      }
    }
    __syncthreads();

    if (pair) {
      // D: lane quarter kq holds MFMA rows 4 kq + i = (activation row, digit); their weights 16^digit 2^(e - 21)
      float c0[4], c1[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * kq + i, m = r / ND, dg = r - m * ND;
        const float p = ldexpf(1.f, 4 * dg);
        c0[i] = (m == 0 && R > 0) ? p * unsc_s[0] : 0.f;
        c1[i] = (m == 1 && R > 1) ? p * unsc_s[1] : 0.f;
      }
#pragma unroll
      for (int ti = 0; ti < MOE_TPW; ++ti) {
        const int tt = wid + ti * MOE_WAVES;  // tile of the chunk
        if (c * MOE_TPC + tt >= a.tiles_k) continue;
        float4_t d[CB][NS];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
          for (int s = 0; s < NS; ++s) d[cb][s] = fzero;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          i64_t bq0[CB], bq1[CB], a_lo, a_hi;
          moe_fp8_tile_codes(w[ti], h, bq0, bq1);
#pragma unroll
          for (int g = 0; g < (SMODE == 1 ? 2 : 1); ++g) {
            moe_fp8_a((SMODE == 1 ? a_blk[g] : a_row) + tt * 128 + h * 64, a_lo, a_hi);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
              float4_t& dd = d[cb][SMODE == 1 ? 2 * h + g : 0];
              dd = moe_mfma_f8<E5M2>(a_lo, bq0[cb], dd);
              dd = moe_mfma_f8<E5M2>(a_hi, bq1[cb], dd);
            }
          }
        }
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            const float4_t dd = d[cb][s];
            tot[0][cb] = fmaf(sc[ti][cb][s], fmaf(dd.x, c0[0], fmaf(dd.y, c0[1], fmaf(dd.z, c0[2], dd.w * c0[3]))), tot[0][cb]);
            tot[1][cb] = fmaf(sc[ti][cb][s], fmaf(dd.x, c1[0], fmaf(dd.y, c1[1], fmaf(dd.z, c1[2], dd.w * c1[3]))), tot[1][cb]);
          }
      }
    } else {
      const float4_t un = *(const float4_t*)(unsc_s + 4 * kq);
#pragma unroll
      for (int ti = 0; ti < MOE_TPW; ++ti) {
        const int tt = wid + ti * MOE_WAVES;
        if (c * MOE_TPC + tt >= a.tiles_k) continue;
        // sum_j 16^j S_j of one scale block, most significant digit first, into the running sums
        auto fold = [&](const float4_t (&S)[ND], int cb, float s) {
          float4_t f = S[ND - 1];
#pragma unroll
          for (int j = ND - 2; j >= 0; --j) f = f * 16.f + S[j];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i][cb] = fmaf(s * un[i], f[i], acc[i][cb]);
        };
        if constexpr (SMODE == 0) {
          float4_t S[CB][ND];
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int j = 0; j < ND; ++j) S[cb][j] = fzero;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            i64_t bq0[CB], bq1[CB], a_lo, a_hi;
            moe_fp8_tile_codes(w[ti], h, bq0, bq1);
#pragma unroll
            for (int j = 0; j < ND; ++j) {
              moe_fp8_a(a_row + j * dstep + tt * 128 + h * 64, a_lo, a_hi);
#pragma unroll
              for (int cb = 0; cb < CB; ++cb) {
                S[cb][j] = moe_mfma_f8<E5M2>(a_lo, bq0[cb], S[cb][j]);
                S[cb][j] = moe_mfma_f8<E5M2>(a_hi, bq1[cb], S[cb][j]);
              }
            }
          }
#pragma unroll
          for (int cb = 0; cb < CB; ++cb) fold(S[cb], cb, sc[ti][cb][0]);
        } else {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            i64_t bq0[CB], bq1[CB], a_lo, a_hi;
            moe_fp8_tile_codes(w[ti], h, bq0, bq1);
#pragma unroll
            for (int g = 0; g < 2; ++g) {
              float4_t S[CB][ND];
#pragma unroll
              for (int j = 0; j < ND; ++j) {
                moe_fp8_a(a_blk[g] + j * d_blk[g] + tt * 128 + h * 64, a_lo, a_hi);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                  S[cb][j] = moe_mfma_f8<E5M2>(a_lo, bq0[cb], fzero);
                  S[cb][j] = moe_mfma_f8<E5M2>(a_hi, bq1[cb], S[cb][j]);
                }
              }
#pragma unroll
              for (int cb = 0; cb < CB; ++cb) fold(S[cb], cb, sc[ti][cb][2 * h + g]);
            }
          }
        }
      }
    }
  }

  // ---- the waves' partial sums, added in wave order; epilogue ----
  if (pair) {
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const float t0 = reduce_kq(tot[0][cb]), t1 = reduce_kq(tot[1][cb]);
      if (lane < 16) slab[wid][cb][0][lane] = t0, slab[wid][cb][1][lane] = t1;
    }
  } else {
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 4; ++i) slab[wid][cb][4 * kq + i][i16] = acc[i][cb];
  }
  __syncthreads();
  const int row = tid >> 4, col = tid & 15;
  if (row >= R) return;
  float v[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    v[cb] = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < MOE_WAVES; ++w2) v[cb] += slab[w2][cb][row][col];
  }
  const int n = (int)blockIdx.x * 16 + col;
  if constexpr (GU) {
    a.out[(size_t)(first + row) * a.ldo + n] = v[0] / (1.0f + expf(-v[0])) * v[CB - 1];  // n < I: I % 16 == 0
  } else {
    if (n < a.N) a.out[(size_t)(first + row) * a.ldo + n] = v[0];
  }
}

// ---- 4. combine ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ y, const int32_t* __restrict__ pos_of,
                                                          const float* __restrict__ topk_w, int top_k, int H,
                                                          void* __restrict__ out, int out_dtype, int ldo) {
  const int t = (int)blockIdx.y, n = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (n >= H) return;
  float acc = 0.f;
  for (int j = 0; j < top_k; ++j) {
    const int p = pos_of[t * top_k + j];
    if (p >= 0) acc = fmaf(topk_w[t * top_k + j], y[(size_t)p * H + n], acc);  // a dropped slot contributes zero
  }
  store_f32(out, (size_t)t * ldo + n, out_dtype, acc);
}

template <bool GU, int SMODE, bool ASYM>
void moe_launch_kind(const MoeGemmArgs& a, int wk, dim3 grid, hipStream_t st) {
  const dim3 block(MOE_WAVES * 64);
  if (wk == 0) hipLaunchKernelGGL((moe_gemm_kernel<GU, SMODE, ASYM, 0>), grid, block, 0, st, a);
  if (wk == MOE_WK_INT8) hipLaunchKernelGGL((moe_gemm_kernel<GU, SMODE, ASYM, MOE_WK_INT8>), grid, block, 0, st, a);
  if constexpr (!ASYM) {  // moe_header_problem admits no table blob with zero points
    if (wk == 1) hipLaunchKernelGGL((moe_gemm_kernel<GU, SMODE, false, 1>), grid, block, 0, st, a);
    if (wk == 2) hipLaunchKernelGGL((moe_gemm_kernel<GU, SMODE, false, 2>), grid, block, 0, st, a);
    if (wk == 3) hipLaunchKernelGGL((moe_gemm_kernel<GU, SMODE, false, 3>), grid, block, 0, st, a);
  }
}

template <bool GU, int SMODE, bool E5M2>
int moe_launch_fp8(const MoeGemmArgs& a, dim3 grid, hipStream_t st) {
  constexpr auto kern = moe_fp8_gemm_kernel<GU, SMODE, E5M2>;
  if (const int rc = allow_dynamic_lds<kern>(moe_fp8_lds_bytes(MOE_BLOCK_ROWS))) return rc;
  hipLaunchKernelGGL(kern, grid, dim3(MOE_WAVES * 64), moe_fp8_lds_bytes(a.lds_rows), st, a);
  return 0;
}

// `wk`: the kernel's weight kind, from moe_gemm_args
template <bool GU>
int moe_launch_gemm(const MoeGemmArgs& a, bool smode1, bool asym, int wk, dim3 grid, hipStream_t st) {
  if (wk == MOE_WK_FP8) {  // symmetric: moe_header_problem
    if (smode1) return a.e5m2 ? moe_launch_fp8<GU, 1, true>(a, grid, st) : moe_launch_fp8<GU, 1, false>(a, grid, st);
    return a.e5m2 ? moe_launch_fp8<GU, 0, true>(a, grid, st) : moe_launch_fp8<GU, 0, false>(a, grid, st);
  }
  if (!smode1 && !asym) moe_launch_kind<GU, 0, false>(a, wk, grid, st);
  if (!smode1 && asym) moe_launch_kind<GU, 0, true>(a, wk, grid, st);
  if (smode1 && !asym) moe_launch_kind<GU, 1, false>(a, wk, grid, st);
  if (smode1 && asym) moe_launch_kind<GU, 1, true>(a, wk, grid, st);
  return 0;
}

void moe_launch_plan(const void* topk_idx, bool idx_is_int64, int S, int E, const MoeRoutePlan& p, hipStream_t st) {
  const auto kern = idx_is_int64 ? moe_plan_kernel<true> : moe_plan_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(1), dim3(MOE_PLAN_THREADS), 0, st, topk_idx, S, E, p.sorted, p.pos_of, p.blocks, p.nblocks);
}

// the grouped form's launch_moe_prompt_product (which has no raw gate/up)
int moe_launch_product(MoeRole role, const MoeCall& m, const MoeRoutePlan& p, const float* h, float* out, hipStream_t st) {
  if (role == MOE_GATE_UP_RAW) return fail("QBits: the grouped form has no raw gate/up product");
  const bool gu = role == MOE_GATE_UP;
  const woq_blob_header& hdr = gu ? *m.gate_up_hdr : *m.down_hdr;
  MoeWeightKind kind;
  MoeGemmArgs a = moe_gemm_args(m, gu, kind);
  const int ndig = lut_args_for(hdr.weight_type, hdr.compute_type, a.lut);  // 0, and an empty table, for the integer kinds
  const int wk = kind == MOE_W_TABLE ? ndig : (kind == MOE_W_INT8 ? MOE_WK_INT8 : (kind == MOE_W_FP8 ? MOE_WK_FP8 : 0));
  if (gu) {
    moe_bind_gate_up(a, m, p, out, m.down_hdr->K);
    return moe_launch_gemm<true>(a, hdr.scale_mode == 1, hdr.off_zp != 0, wk,
                                 dim3((unsigned)a.half_tiles, (unsigned)p.max_blocks), st);
  }
  moe_bind_down(a, m, p, h, out);
  return moe_launch_gemm<false>(a, hdr.scale_mode == 1, hdr.off_zp != 0, wk, dim3((unsigned)a.tiles_n, (unsigned)p.max_blocks),
                                st);
}

}  // namespace

MoeGemmArgs moe_gemm_args(const MoeCall& m, bool gate_up, MoeWeightKind& kind) {
  const woq_blob_header& h = gate_up ? *m.gate_up_hdr : *m.down_hdr;
  MoeGemmArgs a = {};
  a.blobs = (const uint8_t*)(gate_up ? m.gate_up_blobs : m.down_blobs);
  a.stride = gate_up ? m.gate_up_stride : m.down_stride;
  const MoePlanes p = moe_blob_planes(h);
  for (int i = 0; i < 2; ++i) a.off_q[i] = p.off_q[i], a.off_zp[i] = p.off_zp[i];
  a.off_scale = p.off_scale, kind = p.kind;
  a.K = h.K, a.N = h.N, a.tiles_k = h.Kpad / WOQ_TILE_K, a.tiles_n = h.Npad / WOQ_TILE_N;
  a.n_groups = h.n_groups, a.group = h.group, a.scale_type = (int)h.scale_type;
  a.e5m2 = h.weight_type == WOQ_W_FP8_E5M2;
  return a;
}

static void moe_bind(MoeGemmArgs& a, const MoeCall& m, const MoeRoutePlan& p, float* out) {
  a.top_k = m.top_k, a.sorted = p.sorted, a.blocks = p.blocks, a.nblocks = p.nblocks, a.out = out;
  a.lds_rows = std::min(MOE_BLOCK_ROWS, m.T * m.top_k);
}
void moe_bind_gate_up(MoeGemmArgs& g, const MoeCall& m, const MoeRoutePlan& p, float* out, int ldo) {
  moe_bind(g, m, p, out);
  g.x = m.x, g.x_dtype = m.x_dtype, g.ldx = m.ldx;
  g.ldo = ldo, g.half_tiles = m.down_hdr->K / 16;
}
void moe_bind_down(MoeGemmArgs& d, const MoeCall& m, const MoeRoutePlan& p, const float* h, float* y) {
  moe_bind(d, m, p, y);
  d.x = h, d.x_dtype = WOQ_F32, d.ldx = m.down_hdr->K;
  d.ldo = m.down_hdr->N, d.half_tiles = 0;
}

const char* moe_header_problem(const woq_blob_header& h, size_t stride, bool int4_only) {
  if (h.magic != WOQ_BLOB_MAGIC) return "QBits: woq_moe_forward: not a WQH1 packed weight";
  const bool table = woq_weight_is_table(h.weight_type);
  const bool fp8 = woq_weight_is_fp8(h.weight_type);
  if (h.weight_type != WOQ_W_INT4_CLIP && int4_only)
    return "QBits: the engine's sparse layer takes int4 / int3 / int2 expert blobs";
  if (h.weight_type != WOQ_W_INT4_CLIP && h.weight_type != WOQ_W_INT8 && !table && !fp8)
    return "QBits: woq_moe_forward takes int4 / int3 / int2, nf4 / fp4, int8 and fp8 expert blobs";
  if (h.off_shuffle != 0) return "QBits: woq_moe_forward: act-order expert blobs are not built";
  if (h.K <= 0 || h.N <= 0 || h.Kpad % WOQ_TILE_K != 0 || h.Npad % WOQ_TILE_N != 0 || h.n_groups <= 0 || h.group <= 0 ||
      h.scale_mode > 1u || h.scale_type > (uint32_t)WOQ_F16)
    return "QBits: woq_moe_forward: corrupt blob header";
  if (h.scale_mode == 0 && h.n_groups > 1 && h.group % WOQ_TILE_K != 0) return "QBits: woq_moe_forward: corrupt blob header";
  if ((table || fp8) && h.off_zp != 0) return "QBits: woq_moe_forward: corrupt blob header";  // these types are symmetric
  if (fp8) {  // the composite's sections must lie where woq_fp8_headers puts them
    woq_blob_header o, hi, lo;
    if (woq_fp8_headers(&o, &hi, &lo, h.K, h.N, h.group, h.weight_type, h.scale_type, h.compute_type, 0) != 0 ||
        o.off_q != h.off_q || o.off_scale != h.off_scale || o.total_bytes != h.total_bytes)
      return "QBits: woq_moe_forward: corrupt blob header";
  }
  if (h.weight_type == WOQ_W_INT8) {  // the composite's sections must lie where woq_int8_headers puts them
    woq_blob_header o, hi, lo;
    if (woq_int8_headers(&o, &hi, &lo, h.K, h.N, h.group, h.scale_type, h.compute_type, h.off_zp != 0, 0) != 0 ||
        o.off_q != h.off_q || o.off_scale != h.off_scale || o.off_zp != h.off_zp || o.total_bytes != h.total_bytes)
      return "QBits: woq_moe_forward: corrupt blob header";
  }
  if (stride < h.total_bytes || stride % 16 != 0)
    return "QBits: woq_moe_forward: the expert stride is smaller than a blob or no multiple of 16";
  return nullptr;
}

MoePlanes moe_blob_planes(const woq_blob_header& h) {
  MoePlanes p = {};
  if (h.weight_type == WOQ_W_INT8) {
    woq_blob_header o, hi, lo;
    woq_int8_headers(&o, &hi, &lo, h.K, h.N, h.group, h.scale_type, h.compute_type, h.off_zp != 0, 0);
    p.kind = MOE_W_INT8;
    p.off_q[0] = h.off_q + hi.off_q, p.off_q[1] = h.off_scale + lo.off_q;
    p.off_scale = h.off_scale + lo.off_scale;
    p.off_zp[0] = hi.off_zp ? h.off_q + hi.off_zp : 0, p.off_zp[1] = h.off_scale + lo.off_zp;
    return p;
  }
  if (woq_weight_is_fp8(h.weight_type)) {  // both planes carry the scales s; no zero point is read
    woq_blob_header o, hi, lo;
    woq_fp8_headers(&o, &hi, &lo, h.K, h.N, h.group, h.weight_type, h.scale_type, h.compute_type, 0);
    p.kind = MOE_W_FP8;
    p.off_q[0] = h.off_q + hi.off_q, p.off_q[1] = h.off_scale + lo.off_q;
    p.off_scale = h.off_scale + lo.off_scale;
    return p;
  }
  p.kind = woq_weight_is_table(h.weight_type) ? MOE_W_TABLE : MOE_W_INT4;
  p.off_q[0] = h.off_q, p.off_scale = h.off_scale, p.off_zp[0] = h.off_zp;
  return p;
}

void launch_moe_combine(const float* y, const int32_t* pos_of, const float* topk_w, int T, int top_k, int H, void* out,
                        int out_dtype, int ldo, hipStream_t st) {
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((H + 255) / 256), (unsigned)T), dim3(256), 0, st, y, pos_of, topk_w,
                     top_k, H, out, out_dtype, ldo);
}

MoeLayout moe_layout(MoeForm form, int T, int top_k, int E, int hidden, int inter) {
  MoeLayout w;
  const size_t S = (size_t)T * top_k, rows = form == MOE_PROMPT ? MOE_PROMPT_ROWS : MOE_BLOCK_ROWS;
  w.max_blocks = (int)((S + rows - 1) / rows + std::min<size_t>((size_t)E, S));
  w.nseg = form == MOE_PROMPT ? (int)((S + MOE_PLAN_SEG - 1) / MOE_PLAN_SEG) : 0;
  w.sorted = 0;
  w.pos_of = w.sorted + woq_round_up(S * 4, 256);
  w.blocks = w.pos_of + woq_round_up(S * 4, 256);
  w.nblocks = w.blocks + woq_round_up((size_t)w.max_blocks * sizeof(MoeBlock), 256);
  w.counts = w.nblocks + 256;
  w.h = w.counts + woq_round_up((size_t)w.nseg * E * 4, 256);
  w.y = w.h + woq_round_up(S * (size_t)inter * 4, 256);
  w.total = w.y + woq_round_up(S * (size_t)hidden * 4, 256);
  return w;
}

size_t moe_workspace_bytes(MoeForm form, int T, int top_k, int E, int hidden, int inter) {
  const bool ok = T > 0 && top_k > 0 && E > 0 && hidden > 0 && inter > 0 && E <= MOE_MAX_EXPERTS &&
                  (long long)T * top_k <= moe_max_slots(form);
  return ok ? moe_layout(form, T, top_k, E, hidden, inter).total : 0;
}

size_t moe_prompt_plan_bytes(int T, int top_k, int E) { return moe_layout(MOE_PROMPT, T, top_k, E, 0, 0).h; }

MoeRoutePlan moe_plan_tables(MoeForm form, void* workspace, int T, int top_k, int E) {
  const MoeLayout w = moe_layout(form, T, top_k, E, 0, 0);
  uint8_t* ws = (uint8_t*)workspace;
  return MoeRoutePlan{(int32_t*)(ws + w.sorted), (int32_t*)(ws + w.pos_of), (MoeBlock*)(ws + w.blocks),
                      (int32_t*)(ws + w.nblocks), (int32_t*)(ws + w.counts), w.max_blocks, w.nseg};
}

int launch_moe_forward(const MoeCall& m, MoeForm form, hipStream_t st) {
  const int H = m.down_hdr->N, I = m.down_hdr->K;
  const MoeLayout w = moe_layout(form, m.T, m.top_k, m.E, H, I);
  uint8_t* ws = (uint8_t*)m.workspace;
  const MoeRoutePlan plan = moe_plan_tables(form, ws, m.T, m.top_k, m.E);
  float* hbuf = (float*)(ws + w.h);
  float* ybuf = (float*)(ws + w.y);
  const auto product = form == MOE_PROMPT ? launch_moe_prompt_product : moe_launch_product;

  if (!m.plan_ready)  // (else the router wrote the tables)
    (form == MOE_PROMPT ? launch_moe_prompt_plan : moe_launch_plan)(m.topk_idx, m.idx_is_int64, m.T * m.top_k, m.E, plan, st);
  if (const int rc = product(MOE_GATE_UP, m, plan, nullptr, hbuf, st)) return rc;
  if (const int rc = product(MOE_DOWN, m, plan, hbuf, ybuf, st)) return rc;
  if (m.residual != nullptr) {
    if (const int rc = launch_moe_combine_residual(ybuf, plan.pos_of, m.topk_w, m.T, m.top_k, H, *m.residual, st)) return rc;
  } else {
    launch_moe_combine(ybuf, plan.pos_of, m.topk_w, m.T, m.top_k, H, m.out, m.out_dtype, m.ldo, st);
  }
  WOQ_HIP(hipGetLastError());
  return 0;
}

int moe_entry_checks(const MoeEntry& e, const MoeCall& m, size_t workspace_bytes) {
  const std::string fn = std::string("QBits: ") + e.fn;
  WOQ_CHECK(m.gate_up_hdr && m.down_hdr, fn + ": null header");
  if (const char* p = moe_header_problem(*m.gate_up_hdr, m.gate_up_stride, false)) WOQ_FAIL(p);
  if (const char* p = moe_header_problem(*m.down_hdr, m.down_stride, false)) WOQ_FAIL(p);
  const int H = m.down_hdr->N, I = m.down_hdr->K;
  WOQ_CHECK(m.gate_up_hdr->K == H && m.gate_up_hdr->N == 2 * I,
            fn + ": gate/up blobs must be [K = hidden, N = 2 * inter] against down blobs [K = inter, N = hidden]");
  WOQ_CHECK(I % 16 == 0,
            fn + ": the intermediate size must be a multiple of 16 (gate tile tn pairs with up tile tn + inter / 16)");
  WOQ_CHECK(H % 4 == 0, fn + ": the hidden size must be a multiple of 4");
  auto dtype_ok = [](int d) { return d == WOQ_F32 || d == WOQ_BF16 || d == WOQ_F16; };
  WOQ_CHECK(dtype_ok(m.x_dtype) && dtype_ok(m.out_dtype), "QBits: unsupported qbits data type.");
  if (m.T <= 0) return -1;
  const size_t need = e.workspace(m.T, m.top_k, m.E, H, I);
  WOQ_CHECK(need != 0, fn + " takes at most " + std::to_string(MOE_MAX_EXPERTS) + " experts and " +
                           std::to_string(e.max_slots) + " routed slots (T * top_k) per call");
  WOQ_CHECK(m.x && m.topk_idx && m.topk_w && m.gate_up_blobs && m.down_blobs && m.out && m.workspace, fn + ": null tensor");
  WOQ_CHECK(m.ldx >= H && m.ldo >= H, fn + ": leading dimension smaller than hidden");
  WOQ_CHECK((uintptr_t)m.x % (4 * woq_dtype_size((uint32_t)m.x_dtype)) == 0 && m.ldx % 4 == 0,
            fn + ": activation rows must be aligned to four elements");
  WOQ_CHECK((uintptr_t)m.gate_up_blobs % 16 == 0 && (uintptr_t)m.down_blobs % 16 == 0 &&
                (uintptr_t)m.workspace % e.workspace_align == 0,
            fn + (e.workspace_align == 16 ? ": blobs and workspace must be 16-byte aligned"
                                          : ": blobs must be 16-byte and the workspace 256-byte aligned"));
  WOQ_CHECK(workspace_bytes >= need, fn + ": the workspace holds " + std::to_string(workspace_bytes) +
                                         " bytes, this call needs " + std::to_string(need) + " (" + e.workspace_fn + ")");
  return 0;
}

// woq_moe_forward and woq_moe_prompt_forward past their argument lists
static int moe_forward_entry(MoeForm form, const MoeCall& m, size_t workspace_bytes, void* stream) {
  static const MoeEntry entry[2] = {
      {"woq_moe_forward", woq_moe_workspace, "woq_moe_workspace", MOE_MAX_SLOTS, 16},
      {"woq_moe_prompt_forward", woq_moe_prompt_workspace, "woq_moe_prompt_workspace", MOE_PROMPT_MAX_SLOTS, 16}};
  if (const int rc = moe_entry_checks(entry[form], m, workspace_bytes)) return rc < 0 ? 0 : rc;
  return launch_moe_forward(m, form, (hipStream_t)stream);
}

}  // namespace woq

extern "C" size_t woq_moe_workspace(int T, int top_k, int E, int hidden, int inter) {
  return woq::moe_workspace_bytes(woq::MOE_GROUPED, T, top_k, E, hidden, inter);
}
extern "C" size_t woq_moe_prompt_workspace(int T, int top_k, int E, int hidden, int inter) {
  return woq::moe_workspace_bytes(woq::MOE_PROMPT, T, top_k, E, hidden, inter);
}

extern "C" int woq_moe_forward(const void* x_dev, int x_dtype, int ldx, const void* topk_idx_dev, int idx_is_int64,
                               const float* topk_w_dev, int T, int top_k, int E, const void* gate_up_blobs_dev,
                               const woq_blob_header* gate_up_hdr, size_t gate_up_stride, const void* down_blobs_dev,
                               const woq_blob_header* down_hdr, size_t down_stride, void* out_dev, int out_dtype, int ldo,
                               void* workspace_dev, size_t workspace_bytes, void* stream) {
  WOQ_TRY
  const woq::MoeCall m = {x_dev, x_dtype, ldx, topk_idx_dev, idx_is_int64 != 0, topk_w_dev, T, top_k, E,
                          gate_up_blobs_dev, gate_up_hdr, gate_up_stride, down_blobs_dev, down_hdr, down_stride,
                          out_dev, out_dtype, ldo, workspace_dev};
  if (const int rc = woq::moe_forward_entry(woq::MOE_GROUPED, m, workspace_bytes, stream)) return rc;
  WOQ_END
}

extern "C" int woq_moe_prompt_forward(const void* x_dev, int x_dtype, int ldx, const void* topk_idx_dev, int idx_is_int64,
                                      const float* topk_w_dev, int T, int top_k, int E, const void* gate_up_blobs_dev,
                                      const woq_blob_header* gate_up_hdr, size_t gate_up_stride,
                                      const void* down_blobs_dev, const woq_blob_header* down_hdr, size_t down_stride,
                                      void* out_dev, int out_dtype, int ldo, void* workspace_dev, size_t workspace_bytes,
                                      void* stream) {
  WOQ_TRY
  const woq::MoeCall m = {x_dev, x_dtype, ldx, topk_idx_dev, idx_is_int64 != 0, topk_w_dev, T, top_k, E,
                          gate_up_blobs_dev, gate_up_hdr, gate_up_stride, down_blobs_dev, down_hdr, down_stride,
                          out_dev, out_dtype, ldo, workspace_dev};
  if (const int rc = woq::moe_forward_entry(woq::MOE_PROMPT, m, workspace_bytes, stream)) return rc;
  WOQ_END
}
