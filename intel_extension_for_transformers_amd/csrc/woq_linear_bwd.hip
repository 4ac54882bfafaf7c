// woq_linear_bwd.hip — backward of the int4 linear with respect to its activations, on the matrix cores:
//
//     dX[m][k] = sum_n dY[m][n] w[k][n]            w as woq_dequantize_packed_weight defines it
//
// for an act-order blob w is indexed by blob row j and the result lands in column shuffle[j] (the transpose of the
// forward's gather; the shuffle is a permutation, so plain stores, no atomics). The reference's statement
// (autograd/functions.py:163-179) dequantises the whole weight and calls a matmul; here the blob is read as it lies,
// 0.5 B per weight, and no dequantised image of W ever reaches HBM.
//
// Arithmetic: one fp16 product per operand pair on v_mfma_f32_16x16x32_f16, fp32 accumulation over all of N (and over
// both nibble planes of an int8 composite) in one fixed order, one rounding on store.
//  * dY: a pack pass turns every row into fp16 with an exact power-of-two scale 2^e[m] (row max into [2^13, 2^14),
//    the forward's rule), zero beyond N and M, as a plain row-major image [Mpad][N rounded up to 64];
//  * w enters as fp16((q - zp) r), r = fp16(s 2^-E), 2^E the smallest power of two >= max |scale| of the blob (the
//    pack pass finds it with an integer atomic max over the scale section): the scale varies along k (by group) and
//    along the summed n, so it cannot leave the product the way the forward's column scale does. Table types: fp16 of
//    table[code] (s 2^-E) formed in fp32;
//  * epilogue: acc 2^e[m] 2^E, both exact.
//
// Reading the blob against its grain. The blob hands a lane 16 consecutive k of ONE column n (include/woq_blob.h):
// the B fragment of a product summed over k. This product sums over n, its B operand wants, per lane, one k and 8
// consecutive n. Route taken: dY is the row operand (A, 16 B row reads straight from the packed image, each wave
// its own 32 rows, no LDS), W the column operand through an LDS image read back transposed. The other route (W as the
// row operand, computing dX^T) needs the same transposed read of W's image and then stores dX column-wise, 4 rows
// per lane apart by ldo: rejected for the stores.
//  * each wave streams one 1-KiB blob tile per n step with the forward's load (one dwordx4 per lane), dequantises with
//    the forward's nibble-to-fp16 extraction (woq_gemm_f16.hip header) plus two v_perm per word that put the eight
//    values in k order, and writes its two 16-k runs as four 16-B chunks of row n of an [n][k] fp16 image: 64 rows of
//    256 B per stage. One scale and one zero point per run: a run lies in one 32-block, which covers both scale modes;
//  * the image is swizzled: chunk ch of row n sits in slot ch ^ (((n & 3) << 2) | ((n >> 2) & 3)). The B fragment of
//    (n slab of 32, 16 output columns k0..k0+15) is two ds_read_b64_tr_b16: lane group g = lane >> 4 takes the
//    4 x 16 blocks at rows 8g..8g+3 and 8g+4..8g+7, lane 4q+p of the group supplying row q, columns 4p..4p+3. Banks
//    (bank = byte address / 4 mod 64, conflicts per 32-lane half): a half holds groups g, g+1 -> rows 8g+q and
//    8g+8+q; the XOR term is 4q + x with x = 2g & 3 in {0, 2} for the one group and {2, 0} for the other, the chunk
//    is (k0/8 + (p >> 1)) ^ (4q + x): 4 (q) x 2 (x) x 2 (p >> 1) = 16 distinct chunks of 4 banks, inside a chunk the
//    8-byte half p & 1: 32 lanes x 2 banks = all 64 banks once. Conflict-free. EXEC is all ones at every transposed
//    read (no branch around the n loop; workgroups that have no tile leave before it), addresses are 8-byte aligned,
//    tiles past N are padded (their relative scale is forced to 0), never masked.
//
// Tile: 128 m x 128 k per workgroup (one blob K tile wide), 4 waves, wave w = rows [32w, 32w+32) x all 128 columns
// (2 x 8 fragments = 64 accumulator VGPRs), n step 64 = four blob tiles, one per wave, two LDS stages of 16 KiB, one
// barrier per step, every global load of a step requested two steps ahead (two register stages); the blob is read
// once per 128 rows of dY. Workgroup ids XCD-aware in 8 x 8 super-tiles as in the forward. The 16 B fragments of a step are read in four phases of four through two register buffers, fenced so that
// the transposed reads of phase p + 1 are in flight under the eight MFMAs of phase p. No split over N: every output
// element is one accumulator chain in n order, so two runs give the same bytes (a split for few-row calls is not
// built: no measurement at M <= 256 asks for it yet; at M = 512 half the CUs have no workgroup on the K = 4096 shapes).
//
// Measured (MI355X, bf16 dY, int4 sym group 128, profiles/r19_qlora_backward.txt; TFLOP/s of the whole call, pack pass
// included, at M = 2048 / 8192): qkv 4096 x 12288 558 / 664, o 4096 x 4096 473 / 561, gate-up 4096 x 22016 606 / 639,
// down 11008 x 4096 492 / 629; the torch statement (dequantise to fp32, cast, rocBLAS bf16 GEMM) 576 / 1190, 523 / 1104,
// 462 / 1189, 572 / 931. Steps to here, qkv shape at M = 2048: scale type / mode / zero-point branches around the loads
// inside the loop (every step waited out two full memory latencies) 451; branch-free loads issued together, two steps
// ahead 519; the group division hoisted out of the loop (it was ~150 of ~300 VALU instructions a step) and the pack pass
// typed and 16 bytes wide 531; phased transposed reads 558. 198 VGPRs, no scratch, two workgroups per CU.
// Open, the next lever: a step still runs load-wait -> ~150 VALU of dequantisation -> LDS write -> barrier -> reads ->
// 32 MFMAs one after the other inside a wave, and two waves per SIMD cover little of it (MFMA pipe ~25 % busy).
// Dequantising tile t + 1 into the other LDS stage in the shadow of step t's MFMAs (the stages already allow it with
// the barrier moved to the end of the step) should take the VALU off the critical path; a third workgroup per CU needs
// the register stages narrowed (170 VGPRs). Rejected: W as the row operand (see above); a dequantised image of W in
// the workspace (what this kernel exists to avoid).
//
// Workspace (woq_set_workspace; never a stream-ordered allocation, never an image of W):
//     2 Mpad Npad64 (fp16 dY image) + 4 Mpad (row scales, rounded up to 256) + 256 (the scale-max word)
// with Mpad = M rounded up to 128, Npad64 = N rounded up to 64: grows with M N, not with K N.
#include "woq_device.h"
#include "woq_host.h"

namespace woq {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int BWD_BM = 128;                // rows of dY per workgroup
constexpr int BWD_BK = 128;                // output columns per workgroup = one blob K tile
constexpr int BWD_BN = 64;                 // n per step: four blob tiles
constexpr int BWD_STAGE = BWD_BN * BWD_BK * 2;  // one [n][k] fp16 image: 16 KiB

struct BwdPlane {
  const u32x4* q;
  const void* scales;
  const uint8_t* zp;  // null: symmetric
};

struct BwdArgs {
  BwdPlane pl[2];  // int8 composite: HI then LO
  int planes;
  int K, N, tiles_k, tiles_n, n_groups, group, scale_type, scale_mode;
  uint32_t weight_type;
  const int32_t* shuffle;
  // pack pass
  const void* g;
  int g_dtype, ldg, M, Mpad;
  int g_vec;     // every row of dY starts on a 16-byte boundary
  _Float16* gp;  // [Mpad][ldp]
  int ldp;       // N rounded up to 64
  float* rs;     // [Mpad] 2^e per row
  unsigned int* smax;  // bits of max |scale| (first plane: an int8 composite's HI scales are 16 x the LO ones)
  size_t n_scale;
  int scale_blocks;
  // product
  void* out;
  int out_dtype, ldo;
  int nb_m, nb_k, sup_k, n_sup;
};

// ---------------------------------------------------------------------------------------------------------------
// pack pass. Blocks [0, Mpad): one workgroup per row of dY (row max, then convert and store; rows at or beyond M and
// columns at or beyond N are written as zeros and never read). Blocks beyond: max |scale| of the blob.
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

template <int DT>
__global__ __launch_bounds__(256) void linear_bwd_pack_kernel(const BwdArgs a) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if ((int)blockIdx.x >= a.Mpad) {
    const size_t stride = (size_t)a.scale_blocks * 256;
    float mx = 0.f;
    for (size_t i = (size_t)((int)blockIdx.x - a.Mpad) * 256 + tid; i < a.n_scale; i += stride) {
      const float s = fabsf(load_f32(a.pl[0].scales, i, a.scale_type));
      if (s < INFINITY) mx = fmaxf(mx, s);  // NaN and infinity do not take part
    }
    mx = wave_max(mx);
    if (lane == 0 && mx > 0.f) atomicMax(a.smax, __float_as_uint(mx));  // non-negative floats order as integers
    return;
  }
  const int r = blockIdx.x;
  _Float16* dst = a.gp + (size_t)r * a.ldp;
  const int chunks = a.ldp >> 3;
  if (r >= a.M) {
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = tid; c < chunks; c += 256) *(h8*)(dst + 8 * c) = zero;
    if (tid == 0) a.rs[r] = 1.f;
    return;
  }
  const size_t base = (size_t)r * a.ldg;
  const bool vec = a.g_vec != 0;
  float amax = 0.f;
#pragma unroll 2
  for (int c = tid; c < chunks; c += 256) {
    float v[8];
    pack_load8<DT>(a.g, base, 8 * c, a.N, vec, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
  }
  amax = wave_max(amax);
  if (lane == 0) red[wid] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int e = 0;
  if (amax > 0.f && amax < INFINITY) e = max(-100, min(100, __builtin_amdgcn_frexp_expf(amax) - 14));
  const float p2 = ldexpf(1.f, -e);  // |x| 2^-e < 2^14
  if (tid == 0) a.rs[r] = ldexpf(1.f, e);
#pragma unroll 2
  for (int c = tid; c < chunks; c += 256) {  // the second sweep finds the row in L2
    float v[8];
    pack_load8<DT>(a.g, base, 8 * c, a.N, vec, v);
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)(v[j] * p2);
    *(h8*)(dst + 8 * c) = o;
  }
}

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

template <bool TABLE>
__global__ __launch_bounds__(256, 2) void linear_bwd_kernel(const BwdArgs a) {
  __shared__ __attribute__((aligned(1024))) unsigned char sm[2 * BWD_STAGE];
  __shared__ float lut_s[16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;
  const int bid = (int)blockIdx.x;  // XCD-aware 8 x 8 super-tiles, as gemm_f16frag_kernel
  const int sup = ((bid >> 3) >> 6) * 8 + (bid & 7), within = (bid >> 3) & 63;
  if (sup >= a.n_sup) return;  // whole workgroups: no wave reaches the loop with a partial EXEC
  const int mb = (sup / a.sup_k) * 8 + (within >> 3), kb = (sup % a.sup_k) * 8 + (within & 7);
  if (mb >= a.nb_m || kb >= a.nb_k) return;
  if (TABLE && tid < 16) lut_s[tid] = lut_value(a.weight_type, tid);

  // 2^E >= max |scale|, the smallest such power of two
  int E = 0;
  {
    const float mx = __uint_as_float(*a.smax);
    if (mx > 0.f) {
      E = __builtin_amdgcn_frexp_expf(mx);                        // mx = f 2^E, f in [0.5, 1)
      if (__builtin_amdgcn_frexp_mantf(mx) == 0.5f) E -= 1;
    }
  }
  const float pE = ldexpf(1.f, -E);

  const int nsteps = a.ldp / BWD_BN, total = nsteps * a.planes;
  const int m0 = mb * BWD_BM + wid * 32;
  const _Float16* arow[2] = {a.gp + (size_t)(m0 + i16) * a.ldp + kq * 8, a.gp + (size_t)(m0 + 16 + i16) * a.ldp + kq * 8};

  float4_t acc[2][8];
#pragma unroll
  for (int mf = 0; mf < 2; ++mf)
#pragma unroll
    for (int kf = 0; kf < 8; ++kf) acc[mf][kf] = (float4_t){0.f, 0.f, 0.f, 0.f};

  // What one n step needs from HBM, requested two steps ahead of its use: the wave's blob tile, the raw scale words and
  // zero-point bytes of its two runs, and the wave's four dY fragments. fetch() only issues loads (no branch around a
  // load's use, nothing that waits): the scale's type, the scale mode and a missing zero-point section are all folded
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
    const BwdPlane& P = a.pl[plane];
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
    const bool has_zp = a.pl[plane].zp != nullptr;
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

  // epilogue: lane holds column i16 of fragment kf, rows 4 kq + i of fragment mf
  const float upE = ldexpf(1.f, E);
#pragma unroll
  for (int kf = 0; kf < 8; ++kf) {
    const int k = kb * BWD_BK + kf * 16 + i16;
    if (k >= a.K) continue;
    const int col = a.shuffle != nullptr ? a.shuffle[k] : k;
#pragma unroll
    for (int mf = 0; mf < 2; ++mf) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + mf * 16 + 4 * kq + i;
        if (m < a.M) store_f32(a.out, (size_t)m * a.ldo + col, a.out_dtype, acc[mf][kf][i] * a.rs[m] * upE);
      }
    }
  }
}

bool bwd_dtype_ok(int dt) { return dt == WOQ_F32 || dt == WOQ_BF16 || dt == WOQ_F16; }

struct BwdWorkspace {
  size_t image, rs, word, total;  // byte offsets, and the size
};
BwdWorkspace bwd_workspace(int M, const woq_blob_header& h) {
  const size_t Mpad = woq_round_up((size_t)M, BWD_BM), Np = woq_round_up((size_t)h.N, BWD_BN);
  BwdWorkspace w;
  w.image = 0;
  w.rs = Mpad * Np * 2;  // a multiple of 256
  w.word = w.rs + woq_round_up(Mpad * 4, 256);
  w.total = w.word + 256;
  return w;
}

BwdPlane bwd_plane(const uint8_t* base, const woq_blob_header& h) {
  BwdPlane p;
  p.q = (const u32x4*)(base + h.off_q);
  p.scales = base + h.off_scale;
  p.zp = h.off_zp ? base + h.off_zp : nullptr;
  return p;
}

}  // namespace
}  // namespace woq

extern "C" size_t woq_linear_backward_workspace(int M, const woq_blob_header* hdr) {
  if (hdr == nullptr || hdr->magic != WOQ_BLOB_MAGIC || M <= 0 || hdr->N <= 0) return 0;
  return woq::bwd_workspace(M, *hdr).total;
}

extern "C" int woq_linear_backward(const void* grad_out_dev, int grad_dtype, int ldg, const void* blob_dev,
                                   const woq_blob_header* hdr, void* grad_in_dev, int out_dtype, int ldo, int M,
                                   void* stream) {
  WOQ_TRY
  using namespace woq;
  WOQ_CHECK(hdr && hdr->magic == WOQ_BLOB_MAGIC, "QBits: not a WQH1 packed weight");
  WOQ_CHECK(bwd_dtype_ok(grad_dtype) && bwd_dtype_ok(out_dtype), "QBits: unsupported qbits data type.");
  WOQ_CHECK(!woq_weight_is_fp8(hdr->weight_type),
            "QBits: woq_linear_backward: fp8 weights are not built; they take the dequantise-and-matmul arm");
  WOQ_CHECK(hdr->K > 0 && hdr->N > 0 && hdr->Kpad % 128 == 0 && hdr->Npad % 16 == 0, "QBits: corrupt blob header");
  WOQ_CHECK(ldg >= hdr->N && ldo >= hdr->K, "QBits: gradient leading dimension smaller than N/K");
  if (M <= 0) return 0;
  WOQ_CHECK(grad_out_dev && blob_dev && grad_in_dev, "QBits: woq_linear_backward: null tensor");
  hipStream_t st = (hipStream_t)stream;
  const uint8_t* blob = (const uint8_t*)blob_dev;

  BwdArgs a = {};
  woq_blob_header h = *hdr;
  if (hdr->weight_type == WOQ_W_INT8) {
    woq_blob_header o, hi, lo;
    WOQ_CHECK(woq_int8_headers(&o, &hi, &lo, hdr->K, hdr->N, hdr->group, hdr->scale_type, hdr->compute_type,
                               hdr->off_zp != 0, hdr->off_shuffle != 0) == 0, "QBits: corrupt int8 header");
    a.pl[0] = bwd_plane(blob + hdr->off_q, hi);
    a.pl[1] = bwd_plane(blob + hdr->off_scale, lo);
    a.planes = 2;
    h = hi;
  } else {
    a.pl[0] = bwd_plane(blob, h);
    a.pl[1] = a.pl[0];
    a.planes = 1;
  }
  a.shuffle = hdr->off_shuffle ? (const int32_t*)(blob + hdr->off_shuffle) : nullptr;
  a.K = h.K, a.N = h.N, a.tiles_k = h.Kpad / 128, a.tiles_n = h.Npad / 16, a.n_groups = h.n_groups, a.group = h.group;
  a.scale_type = (int)h.scale_type, a.scale_mode = (int)h.scale_mode, a.weight_type = h.weight_type;
  a.n_scale = h.scale_mode == 0 ? (size_t)a.tiles_n * a.n_groups * 16 : (size_t)a.tiles_n * a.tiles_k * 64;
  a.scale_blocks = (int)std::min<size_t>(256, (a.n_scale + 1023) / 1024);
  a.g = grad_out_dev, a.g_dtype = grad_dtype, a.ldg = ldg, a.M = M;
  a.g_vec = ((uintptr_t)grad_out_dev % 16 == 0 && ((size_t)ldg * woq_dtype_size((uint32_t)grad_dtype)) % 16 == 0) ? 1 : 0;
  a.Mpad = (int)woq_round_up((size_t)M, BWD_BM);
  a.ldp = (int)woq_round_up((size_t)h.N, BWD_BN);
  a.out = grad_in_dev, a.out_dtype = out_dtype, a.ldo = ldo;
  a.nb_m = a.Mpad / BWD_BM, a.nb_k = a.tiles_k;
  a.sup_k = (a.nb_k + 7) / 8;
  a.n_sup = ((a.nb_m + 7) / 8) * a.sup_k;

  const BwdWorkspace w = bwd_workspace(M, h);
  unsigned char* ws = (unsigned char*)scratch_take(w.total, st, nullptr);  // the workspace or nothing
  if (ws == nullptr)
    WOQ_FAIL("QBits: woq_linear_backward: the workspace (woq_set_workspace) has no room for the " +
             std::to_string(w.total) + " bytes this call needs (woq_linear_backward_workspace)");
  a.gp = (_Float16*)(ws + w.image), a.rs = (float*)(ws + w.rs), a.smax = (unsigned int*)(ws + w.word);

  hipError_t e = hipMemsetAsync(a.smax, 0, sizeof(unsigned int), st);
  if (e == hipSuccess) {
    const dim3 pgrid((unsigned)(a.Mpad + a.scale_blocks));
    if (grad_dtype == WOQ_F32)
      hipLaunchKernelGGL(linear_bwd_pack_kernel<WOQ_F32>, pgrid, dim3(256), 0, st, a);
    else if (grad_dtype == WOQ_BF16)
      hipLaunchKernelGGL(linear_bwd_pack_kernel<WOQ_BF16>, pgrid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL(linear_bwd_pack_kernel<WOQ_F16>, pgrid, dim3(256), 0, st, a);
    const dim3 grid((unsigned)(((a.n_sup + 7) / 8) * 8 * 64));
    if (is_table_type(h.weight_type))
      hipLaunchKernelGGL(linear_bwd_kernel<true>, grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL(linear_bwd_kernel<false>, grid, dim3(256), 0, st, a);
    e = hipGetLastError();
  }
  scratch_release(ws, w.total, false, st);
  WOQ_HIP(e);
  WOQ_END
}
