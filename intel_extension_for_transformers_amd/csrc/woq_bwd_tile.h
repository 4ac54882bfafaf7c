// woq_bwd_tile.h — what the transposed products share: the backward of the dense linear (woq_linear_bwd.hip, whose
// header comment states the arithmetic, the LDS image and its swizzle) and the grouped backward of the routed expert
// block (woq_moe_bwd.hip). One 128-row x 128-column tile of
//
//     acc[m][k] = sum_n gp[m][n] fp16((q - zp)[k][n] r[k][n])          r = fp16(s 2^-E)
//
// walked in n steps of 64 over every nibble plane: the blob tile stream, the dequantisation into the swizzled [n][k]
// fp16 image, the transposed reads and the MFMAs (bwd_tile), and the row half of the pack pass (bwd_pack_row). Which
// rows and which blob a workgroup takes, and what it does with the accumulators, stay with the caller.
#pragma once
#include "woq_device.h"

namespace woq {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int BWD_BM = 128;                // rows of the packed gradient per workgroup
constexpr int BWD_BK = 128;                // output columns per workgroup = one blob K tile
constexpr int BWD_BN = 64;                 // n per step: four blob tiles
constexpr int BWD_STAGE = BWD_BN * BWD_BK * 2;  // one [n][k] fp16 image: 16 KiB

struct BwdPlane {
  const u32x4* q;
  const void* scales;
  const uint8_t* zp;  // null: symmetric
};

// the blob geometry a tile walks; ldp = the packed image's row length (N rounded up to 64)
struct BwdGeom {
  int planes, tiles_k, tiles_n, n_groups, group, scale_type, scale_mode, ldp;
};

// ---------------------------------------------------------------------------------------------------------------
// pack pass
// ---------------------------------------------------------------------------------------------------------------
// eight consecutive elements k0 .. k0 + 7 of a row; elements at or beyond N read as 0 and are never loaded
template <int DT>
__device__ __forceinline__ void pack_load8(const void* g, size_t base, int k0, int N, bool vec, float (&v)[8]) {
  if (vec && k0 + 8 <= N) {  // 16-byte aligned rows: one (16-bit) or two (fp32) dwordx4
    if constexpr (DT == WOQ_F32) {
      const float4_t lo = *(const float4_t*)((const float*)g + base + k0);
      const float4_t hi = *(const float4_t*)((const float*)g + base + k0 + 4);
      v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
    } else {
      const u32x4 raw = *(const u32x4*)((const uint16_t*)g + base + k0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint16_t bits = (uint16_t)(raw[j >> 1] >> (16 * (j & 1)));
        v[j] = DT == WOQ_BF16 ? bf16_bits_to_f32(bits) : f16_bits_to_f32(bits);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = k0 + j < N ? load_f32(g, base + k0 + j, DT) : 0.f;
  }
}

// the exact power of two 2^-e that takes a row of largest magnitude amax into [2^13, 2^14) (the forward's rule)
__device__ __forceinline__ int bwd_row_exp(float amax) {
  int e = 0;
  if (amax > 0.f && amax < INFINITY) e = max(-100, min(100, __builtin_amdgcn_frexp_expf(amax) - 14));
  return e;
}

// the maximum of four waves' values, every thread of the 256 receiving it; red: four floats of LDS
__device__ __forceinline__ float bwd_block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// one workgroup of 256 threads: a zero row of the image, its scale 1
__device__ __forceinline__ void bwd_pack_zero_row(_Float16* dst, int ldp, float* rs) {
  const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = threadIdx.x; c < (ldp >> 3); c += 256) *(h8*)(dst + 8 * c) = zero;
  if (threadIdx.x == 0) *rs = 1.f;
}

// one workgroup of 256 threads: row `base` .. `base + N` of g (row max, then convert and store) -> dst[0, ldp), *rs = 2^e
template <int DT>
__device__ __forceinline__ void bwd_pack_row(const void* g, size_t base, int N, bool vec, _Float16* dst, int ldp,
                                             float* rs, float* red) {
  const int tid = threadIdx.x, chunks = ldp >> 3;
  float amax = 0.f;
#pragma unroll 2
  for (int c = tid; c < chunks; c += 256) {
    float v[8];
    pack_load8<DT>(g, base, 8 * c, N, vec, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
  }
  amax = bwd_block_max(amax, red);
  const int e = bwd_row_exp(amax);
  const float p2 = ldexpf(1.f, -e);  // |x| 2^-e < 2^14
  if (tid == 0) *rs = ldexpf(1.f, e);
#pragma unroll 2
  for (int c = tid; c < chunks; c += 256) {  // the second sweep finds the row in L2
    float v[8];
    pack_load8<DT>(g, base, 8 * c, N, vec, v);
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)(v[j] * p2);
    *(h8*)(dst + 8 * c) = o;
  }
}

// max(mx, |scale|) over elements first, first + stride, .. of a scale section
__device__ __forceinline__ float bwd_scale_sweep(const void* scales, int scale_type, size_t n_scale, size_t first,
                                                 size_t stride, float mx) {
  for (size_t i = first; i < n_scale; i += stride) {
    const float s = fabsf(load_f32(scales, i, scale_type));
    if (s < INFINITY) mx = fmaxf(mx, s);  // NaN and infinity do not take part
  }
  return mx;
}
// a wave's maximum into *smax (bits of a non-negative float)
__device__ __forceinline__ void bwd_scale_publish(float mx, unsigned int* smax) {
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(smax, __float_as_uint(mx));  // non-negative floats order as integers
}

// E of 2^E >= max |scale|, the smallest such power of two
__device__ __forceinline__ int bwd_scale_exp(const unsigned int* smax) {
  int E = 0;
  const float mx = __uint_as_float(*smax);
  if (mx > 0.f) {
    E = __builtin_amdgcn_frexp_expf(mx);                        // mx = f 2^E, f in [0.5, 1)
    if (__builtin_amdgcn_frexp_mantf(mx) == 0.5f) E -= 1;
  }
  return E;
}

// ---------------------------------------------------------------------------------------------------------------
// the tile
// ---------------------------------------------------------------------------------------------------------------
// byte offset of 16-byte chunk ch (0..15) of row n (0..63) in an [n][k] image
__device__ __forceinline__ int img_off(int row, int ch) {
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

__device__ __forceinline__ h4 tr_read(const unsigned char* p) {
  typedef __fp16 f4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
  return __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) f4*)p));
}

// one blob word (eight k of one column) -> fp16 (q - zp) r in k order
__device__ __forceinline__ h8 deq_word(uint32_t x, h2 sub_lo, h2 sub_hi, h2 r) {
  const uint32_t u = x ^ 0x88888888u;  // signed nibbles -> u = q + 8
  h2 a = __builtin_bit_cast(h2, (u & 0x000f000fu) | 0x64006400u);         // 1024 + u: k-offsets 0, 2
  h2 b = __builtin_bit_cast(h2, ((u >> 8) & 0x000f000fu) | 0x64006400u);  // 1, 3
  h2 c = __builtin_bit_cast(h2, (u & 0x00f000f0u) | 0x54005400u);         // 64 + u: 4, 6
  h2 d = __builtin_bit_cast(h2, ((u >> 8) & 0x00f000f0u) | 0x54005400u);  // 5, 7
  a = (a - sub_lo) * r, b = (b - sub_lo) * r, c = (c - sub_hi) * r, d = (d - sub_hi) * r;
  const uint32_t ua = __builtin_bit_cast(uint32_t, a), ub = __builtin_bit_cast(uint32_t, b);
  const uint32_t uc = __builtin_bit_cast(uint32_t, c), ud = __builtin_bit_cast(uint32_t, d);
  const u32x4 o = {__builtin_amdgcn_perm(ub, ua, 0x05040100u), __builtin_amdgcn_perm(ub, ua, 0x07060302u),
                   __builtin_amdgcn_perm(ud, uc, 0x05040100u), __builtin_amdgcn_perm(ud, uc, 0x07060302u)};
  return __builtin_bit_cast(h8, o);
}

__device__ __forceinline__ h8 deq_word_table(uint32_t x, const float* lut, float rf) {
  h8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (_Float16)(lut[(x >> nibble_shift(j)) & 0xfu] * rf);
  return o;
}

// The n loop of one workgroup of four waves: wave w accumulates rows arow[0] (16 rows, one per lane & 15) and arow[1]
// (the next 16) of the packed image against blob K tile kb of the planes pl, all 128 columns, into acc[2][8] (lane:
// column i16 of fragment kf, rows 4 kq + i of fragment mf). arow[mf] = the lane's row + 8 (lane >> 4): every address up
// to a.ldp elements on must be readable. pE = 2^-E. sm: 2 x BWD_STAGE bytes of LDS, 1 KiB aligned; lut_s (TABLE): the 16
// table values, written by the caller before the call. EVERY wave of the workgroup must arrive with EXEC all ones.
template <bool TABLE>
__device__ __forceinline__ void bwd_tile(const BwdGeom& a, const BwdPlane (&pl)[2], int kb,
                                         const _Float16* const (&arow)[2], float pE, unsigned char* sm,
                                         const float* lut_s, float4_t (&acc)[2][8]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;
  const int nsteps = a.ldp / BWD_BN, total = nsteps * a.planes;

#pragma unroll
  for (int mf = 0; mf < 2; ++mf)
#pragma unroll
    for (int kf = 0; kf < 8; ++kf) acc[mf][kf] = (float4_t){0.f, 0.f, 0.f, 0.f};

  // What one n step needs from HBM, requested two steps ahead of its use: the wave's blob tile, the raw scale words and
  // zero-point bytes of its two runs, and the wave's four gradient fragments. fetch() only issues loads (no branch around
  // a load's use, nothing that waits): the scale's type, the scale mode and a missing zero-point section are all folded
  // into addresses and into selects at the point of use.
  struct Stage {
    u32x4 wv;
    uint32_t sraw[2], zraw[2];
    h8 af[2][2];
  };
  const int esz = a.scale_type == WOQ_F32 ? 4 : 2;
  // scale / zero-point element of (column tile tn, run h) = tn * sstride + sbase[h]: everything but tn is fixed per lane
  // (the group of a run does not move with n), so the division by the group size happens once, not per step
  const size_t sstride = a.scale_mode == 0 ? (size_t)a.n_groups * 16 : (size_t)a.tiles_k * 64;
  size_t sbase[2];
  bool shigh[2];  // a 16-bit scale sits in the high half of its aligned word
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int g = (kb * 128 + h * 64 + kq * 16) / a.group;
    g = g >= a.n_groups ? a.n_groups - 1 : g;
    sbase[h] = a.scale_mode == 0 ? (size_t)g * 16 + i16 : ((((size_t)kb * 16 + i16) << 2) + 2 * h + (kq >> 1));
    shigh[h] = (sbase[h] & 1) != 0;  // sstride is even
  }
  auto scale_index = [&](int tn, int h) -> size_t { return (size_t)tn * sstride + sbase[h]; };
  auto tile_of = [&](int t, int& plane, int& s, bool& live) {
    plane = t >= nsteps ? 1 : 0, s = t - plane * nsteps;
    live = s * 4 + wid < a.tiles_n;  // wave-uniform; a tile past Npad is padding: relative scale 0
    return live ? s * 4 + wid : a.tiles_n - 1;
  };
  auto fetch = [&](Stage& S, int t) {
    int plane, s;
    bool live;
    const int tn = tile_of(t, plane, s, live);
    const BwdPlane& P = pl[plane];
    // a symmetric plane has no zero-point section: the byte is read from the scale section (in bounds: at least two
    // bytes per scale) and dropped at the point of use
    const uint8_t* zp = P.zp != nullptr ? P.zp : (const uint8_t*)P.scales;
    S.wv = P.q[((size_t)tn * a.tiles_k + kb) * 64 + lane];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const size_t si = scale_index(tn, h);
      S.sraw[h] = *(const uint32_t*)((const unsigned char*)P.scales + ((si * esz) & ~(size_t)3));  // the aligned word
      S.zraw[h] = zp[si];
    }
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
      for (int sl = 0; sl < 2; ++sl) S.af[mf][sl] = *(const h8*)(arow[mf] + s * BWD_BN + sl * 32);
  };

  // lane constants of the transposed reads: row q_ (+ 4) of the group's block, 8-byte piece p_ of its 32 bytes
  const int q_ = i16 >> 2, p_ = i16 & 3;
  int tr_row[2], tr_x[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const int row = 8 * kq + 4 * hh + q_;  // + 32 per slab: the XOR term does not see it
    tr_row[hh] = 256 * row + 8 * (p_ & 1);
    tr_x[hh] = (((row & 3) << 2) | ((row >> 2) & 3)) ^ (p_ >> 1);
  }
  const int wr_row = wid * 16 + i16;

  // one n step: dequantise the stage's tile into LDS, re-issue the stage's loads for step t + 2, then the products
  auto step = [&](Stage& S, int t) {
    unsigned char* st = sm + (t & 1) * BWD_STAGE;
    int plane, s;
    bool live;
    tile_of(t, plane, s, live);
    const bool has_zp = pl[plane].zp != nullptr;
    // this wave's blob tile -> rows [16 wid, 16 wid + 16) of the image
    float r[2];
    int uz[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t word = S.sraw[h];
      const uint32_t half = shigh[h] ? word >> 16 : word & 0xffffu;
      const float s32 = __uint_as_float(word), sbf = __uint_as_float(half << 16), sfh = f16_bits_to_f32((uint16_t)half);
      const float sv = a.scale_type == WOQ_F32 ? s32 : (a.scale_type == WOQ_BF16 ? sbf : sfh);
      r[h] = live ? sv * pE : 0.f;
      uz[h] = has_zp ? (int)S.zraw[h] : 8;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int h = w >> 1, ch = h * 8 + kq * 2 + (w & 1);
      h8 v;
      if constexpr (TABLE) {
        v = deq_word_table(S.wv[w], lut_s, r[h]);
      } else {
        const _Float16 rh = (_Float16)r[h];
        const _Float16 sl = (_Float16)(float)(1024 + uz[h]), sh = (_Float16)(float)(64 + uz[h]);
        v = deq_word(S.wv[w], (h2){sl, sl}, (h2){sh, sh}, (h2){rh, rh});
      }
      *(h8*)(st + img_off(wr_row, ch)) = v;
    }
    h8 ac[2][2];
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
      for (int sl = 0; sl < 2; ++sl) ac[mf][sl] = S.af[mf][sl];
    if (t + 2 < total) fetch(S, t + 2);  // uniform over the workgroup
    __syncthreads();
    // the 16 B fragments of the step in four phases of four (slab, then column half), two register buffers: the
    // transposed reads of phase p + 1 are in flight while the eight MFMAs of phase p run
    auto read_phase = [&](int p, h8 (&b)[4]) {
      const int sl = p >> 1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kf = 4 * (p & 1) + j;
        const h4 b0 = tr_read(st + sl * 32 * 256 + tr_row[0] + 16 * ((2 * kf) ^ tr_x[0]));
        const h4 b1 = tr_read(st + sl * 32 * 256 + tr_row[1] + 16 * ((2 * kf) ^ tr_x[1]));
        b[j] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
    };
    auto mfma_phase = [&](int p, const h8 (&b)[4]) {
      const int sl = p >> 1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kf = 4 * (p & 1) + j;
#pragma unroll
        for (int mf = 0; mf < 2; ++mf)
          acc[mf][kf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ac[mf][sl], b[j], acc[mf][kf], 0, 0, 0);
      }
    };
    h8 ba[4], bb[4];
    // (the scheduling fences keep the compiler from folding the phases back into read, wait, two MFMAs)
    read_phase(0, ba);
    read_phase(1, bb);
    __builtin_amdgcn_sched_barrier(0);
    mfma_phase(0, ba);
    __builtin_amdgcn_sched_barrier(0);
    read_phase(2, ba);
    __builtin_amdgcn_sched_barrier(0);
    mfma_phase(1, bb);
    __builtin_amdgcn_sched_barrier(0);
    read_phase(3, bb);
    __builtin_amdgcn_sched_barrier(0);
    mfma_phase(2, ba);
    __builtin_amdgcn_sched_barrier(0);
    mfma_phase(3, bb);
  };

  Stage S0, S1;
  fetch(S0, 0);
  if (total > 1) fetch(S1, 1);
  if (TABLE) __syncthreads();
  for (int t = 0; t < total; t += 2) {  // every branch here is uniform over the workgroup: EXEC stays all ones
    step(S0, t);
    if (t + 1 < total) step(S1, t + 1);
  }
}

}  // namespace woq
