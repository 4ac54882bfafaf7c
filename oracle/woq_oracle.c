/*
 * woq_oracle.c — CPU restatement of the reference's int4 weight-only-quantized linear path.
 *
 * TEST INFRASTRUCTURE ONLY. Nothing under intel_extension_for_transformers_amd/ may import,
 * link or call this file; only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
 * leg use it, and only as the checker / the reported CPU baseline.
 *
 * PARITY PINNING STATUS (see DESIGN.md "Oracle"):
 *  - optimum/INC checkpoint decode, signed-nibble convention, g_idx -> shuffle-index
 *    conversion: pinned against outputs of the reference's own Python functions executed in
 *    the build container (tests/golden/make_golden.py, fixtures in tests/golden/).
 *  - RMSNorm / RoPE / SiLU / GeLU: pinned against HF transformers modules (the reference
 *    runs stock HF code between the linears); fixtures in tests/golden/.
 *  - the GEMM itself: the reference defines it as dequantize -> fp32 matmul -> +bias
 *    (autograd/functions.py:41-63) and its own tests only check self-consistency against
 *    that definition (qbits_ut/test_weightonly.py:51-88); this file IS that definition.
 *  - BesTLA's / neural_compressor's RTN rounding rule (orc_rtn_quantize): PARITY UNPINNED —
 *    both libraries are external to /root/reference (neural-speed@2f79436, INC > 2.6) and
 *    cannot be built here; every GEMM parity test feeds identical (q, scale, zp) tensors to
 *    oracle and GPU so the rounding rule cannot cause a mismatch.
 *  - oracle/_ref (compiled reference): NOT BUILDABLE — qbits is a dispatcher over BesTLA,
 *    fetched by CMake FetchContent at configure time (qbits/dispatcher/neural_speed.cmake:1-9).
 *
 * Build: see oracle/Makefile (gcc -O2 -fopenmp -shared -fPIC).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/woq_blob.h"

#define ORC_API __attribute__((visibility("default")))

/* ---------------------------------------------------------------------------------------
 * helpers: bf16 / fp16 <-> fp32 (round-to-nearest-even), used for scale storage types and
 * for restating the bf16 store of the epilogue (qbits/dispatcher/include/bestla_customop.hpp:22-40)
 * ------------------------------------------------------------------------------------- */
static inline float bf16_to_f32(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static inline uint16_t f32_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u); /* nan */
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float f16_to_f32(uint16_t h) {
  uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu, u;
  if (exp == 0) {
    if (man == 0) {
      u = sign;
    } else {
      int e = -1;
      do {
        man <<= 1;
        ++e;
      } while (!(man & 0x400u));
      u = sign | (uint32_t)(127 - 15 - e) << 23 | (man & 0x3ffu) << 13;
    }
  } else if (exp == 31) {
    u = sign | 0x7f800000u | man << 13;
  } else {
    u = sign | (exp + 112u) << 23 | man << 13;
  }
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static inline uint16_t f32_to_f16(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0u));
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u); /* overflow -> inf (after rounding) */
  if (x < 0x33000001u) return (uint16_t)sign;               /* underflow -> 0 */
  int exp = (int)(x >> 23) - 127;
  uint32_t man = (x & 0x7fffffu) | 0x800000u;
  int shift;
  uint32_t half;
  if (exp < -14) {
    shift = 13 + (-14 - exp);
    half = 0;
  } else {
    shift = 13;
    half = (uint32_t)(exp + 15) << 10;
    man &= 0x7fffffu;
  }
  uint32_t r = man >> shift, rem = man & ((1u << shift) - 1u), mid = 1u << (shift - 1);
  if (rem > mid || (rem == mid && (r & 1u))) ++r;
  return (uint16_t)(sign | (half + r));
}

ORC_API float orc_load_scalar(const void* p, size_t idx, int dtype) {
  if (dtype == WOQ_F32) return ((const float*)p)[idx];
  if (dtype == WOQ_BF16) return bf16_to_f32(((const uint16_t*)p)[idx]);
  return f16_to_f32(((const uint16_t*)p)[idx]);
}
ORC_API void orc_store_scalar(void* p, size_t idx, int dtype, float v) {
  if (dtype == WOQ_F32)
    ((float*)p)[idx] = v;
  else if (dtype == WOQ_BF16)
    ((uint16_t*)p)[idx] = f32_to_bf16(v);
  else
    ((uint16_t*)p)[idx] = f32_to_f16(v);
}

/* ---------------------------------------------------------------------------------------
 * a13  unpack_weight — decode the INC / optimum on-disk format
 *      reference: transformers/llm/quantization/utils.py:82-125
 *   qweight int32 [K/pack, N]: field j of word i is row pack*i + j            (:109-114)
 *   qzeros  int32 [G, N/pack]: field j of word c is column pack*c + j, the
 *           stored value is zp-1 so +1 is added back                           (:86-94)
 *   8-bit: sym weight -= 128 (:116-119); asym weight/zeros shifted by -128 into int8
 *          (:103-106, :121-124); sym zeros are re-read as int8 before the +1   (:91-92)
 *   (the try/except reshape fallback :95-101 is for padded N and is not restated.)
 * outputs: w_out int8 [K, N] (4-bit: values 0..15), z_out int8 [G, N] or untouched.
 * ------------------------------------------------------------------------------------- */
ORC_API void orc_unpack_weight(const int32_t* qweight, const int32_t* qzeros, int K, int N, int G, int bits,
                               int sym, int8_t* w_out, int8_t* z_out) {
  const int pack = 32 / bits;
  const uint32_t mask = (1u << bits) - 1u;
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) {
      uint32_t word = (uint32_t)qweight[(size_t)(k / pack) * N + n];
      int32_t v = (int32_t)((word >> (bits * (k % pack))) & mask);
      if (bits == 8) v -= 128; /* sym: shift bias; asym: uint8 -> int8 offset; same arithmetic */
      w_out[(size_t)k * N + n] = (int8_t)v;
    }
  if (qzeros && z_out) {
    const int NW = (N + pack - 1) / pack;
    for (int g = 0; g < G; ++g)
      for (int n = 0; n < N; ++n) {
        uint32_t word = (uint32_t)qzeros[(size_t)g * NW + n / pack];
        int32_t v = (int32_t)((word >> (bits * (n % pack))) & mask);
        if (bits == 8) {
          if (sym) v = (int8_t)v; /* .to(torch.int8) */
          v += 1;
          if (!sym) v -= 128;
        } else {
          v += 1;
        }
        z_out[(size_t)g * N + n] = (int8_t)v;
      }
  }
}

/* a14  signed-nibble convention of QuantizedLinearQBits.set_weights_bias
 *      reference: transformers/llm/quantization/nn/modules.py:225-227
 *        int_weight = (int_weight - 8) * 16 // 16 ; gptq_zeros = (gptq_zeros - 8) * 16 // 16
 *      evaluated on int8 tensors: the *16 WRAPS in int8 and // is floor division, so the
 *      expression sign-extends the low nibble of (t - 8). For weights (0..15) that is t - 8;
 *      for zero points the INC "+1" (utils.py:93-94) can make t = 16, which comes out as -8,
 *      not +8 (pinned by tests/golden/set_weights_bias.npz). Result is always in [-8, 7]. */
ORC_API void orc_to_signed_nibble(int8_t* t, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    int8_t wrapped = (int8_t)(uint8_t)(((int)t[i] - 8) * 16); /* int8 multiply wraps */
    t[i] = (int8_t)(wrapped >> 4);                            /* floor division by 16 */
  }
}

/* test_packq.py:22-28 convert_idx — GPTQ g_idx (group id per input channel) -> shuffle indices
 * (position j of the group-sorted order holds original channel ret[j]); stable within a group.
 * This is what acquire_packed_weight_info(G_IDX) returns (test_packq.py:97-100). */
ORC_API void orc_convert_idx(const int32_t* g_idx, int K, int blocksize, int32_t* ret) {
  int ng = (K + blocksize - 1) / blocksize;
  int* counter = (int*)calloc((size_t)ng, sizeof(int));
  for (int i = 0; i < K; ++i) {
    int g = g_idx[i];
    ret[g * blocksize + counter[g]] = i;
    counter[g]++;
  }
  free(counter);
}

/* ---------------------------------------------------------------------------------------
 * RTN quantiser — PARITY UNPINNED (see header). Formula implied by the reference's own
 * re-quantisation helper quant_weight_w_scale (modules.py:264-295): q = round(w/scale + zp),
 * with the int4 "clip" range: sym scale = max|w| / 7, q in [-8,7]; asym over the range widened to
 * hold zero, lo = min(min w, 0), hi = max(max w, 0): scale = (hi - lo) / 15, zp = round(-lo / scale),
 * q in [0,15] then shifted to the signed domain (q-8, zp-8). (Without the widening a group on one
 * side of zero clips its zero point and saturates every code; tests/quant_reference.py.)
 * weight is [K,N] (transpose=0) or [N,K] (transpose=1, nn.Linear layout, qbits.cpp:90-92).
 * outputs: q int8 [K,N] signed domain, scales fp32 [G,N], zp int8 [G,N] signed domain.
 * rounding: nearbyintf (round-half-even, what torch.round does).
 * ------------------------------------------------------------------------------------- */
ORC_API void orc_rtn_quantize(const float* w, int transpose, int K, int N, int group, int asym, int8_t* q,
                              float* scales, int8_t* zp) {
  if (group <= 0 || group > K) group = K;
  int G = (K + group - 1) / group;
#pragma omp parallel for schedule(static)
  for (int n = 0; n < N; ++n)
    for (int g = 0; g < G; ++g) {
      int k0 = g * group, k1 = k0 + group > K ? K : k0 + group;
      float mx = -INFINITY, mn = INFINITY, amax = 0.f;
      for (int k = k0; k < k1; ++k) {
        float v = transpose ? w[(size_t)n * K + k] : w[(size_t)k * N + n];
        mx = v > mx ? v : mx;
        mn = v < mn ? v : mn;
        amax = fabsf(v) > amax ? fabsf(v) : amax;
      }
      float s;
      int z = 0;
      if (!asym) {
        s = amax / 7.f;
        if (s == 0.f) s = 1.f;
      } else {
        const float hi = mx > 0.f ? mx : 0.f, lo = mn < 0.f ? mn : 0.f; /* zero inside the range */
        s = (hi - lo) / 15.f;
        if (s == 0.f) s = 1.f;
        z = (int)nearbyintf(-lo / s);
        z = z < 0 ? 0 : (z > 15 ? 15 : z);
      }
      scales[(size_t)g * N + n] = s;
      if (asym) zp[(size_t)g * N + n] = (int8_t)(z - 8);
      for (int k = k0; k < k1; ++k) {
        float v = transpose ? w[(size_t)n * K + k] : w[(size_t)k * N + n];
        int qi;
        if (!asym) {
          qi = (int)nearbyintf(v / s);
          qi = qi < -8 ? -8 : (qi > 7 ? 7 : qi);
        } else {
          qi = (int)nearbyintf(v / s) + z;
          qi = qi < 0 ? 0 : (qi > 15 ? 15 : qi);
          qi -= 8;
        }
        q[(size_t)k * N + n] = (int8_t)qi;
      }
    }
}

/* a11 / modules.py:264-295 inverse: W[k][n] = (q - zp) * scale, group along K, tail group allowed. */
ORC_API void orc_dequant_raw(const int8_t* q, const float* scales, const int8_t* zp, int K, int N, int group,
                             float* w_out) {
  if (group <= 0 || group > K) group = K;
#pragma omp parallel for schedule(static)
  for (int k = 0; k < K; ++k) {
    int g = k / group;
    for (int n = 0; n < N; ++n) {
      int z = zp ? zp[(size_t)g * N + n] : 0;
      w_out[(size_t)k * N + n] = (float)(q[(size_t)k * N + n] - z) * scales[(size_t)g * N + n];
    }
  }
}

/* ---------------------------------------------------------------------------------------
 * a9  repack_quantized_weight — host restatement of the layout transform into the WQH1 blob.
 *     reference: qbits.cpp:61-77 -> bestla_packq_impl.cpp:20-41 (createStorage, setShuffleIndices,
 *     packQWeight). Layout transform only: int8 [K,N] (int4 values in the signed domain), fp32
 *     scales [G,N], int8 zp [G,N] | NULL, int32 shuffle idx [K] | NULL -> blob. Values outside
 *     [-8,7] keep their low nibble (two's complement) — the reference's behaviour for those is
 *     not observable from /root/reference (test_packq.py:57 feeds such values and only checks
 *     self-consistency), so that case is unpinned.
 * returns 0 or -1 (unsupported geometry).
 * ------------------------------------------------------------------------------------- */
ORC_API int orc_repack(const int8_t* q, const float* scales, const int8_t* zp, const int32_t* shuffle, int K,
                       int N, int group, int scale_type, int compute_type, uint8_t* blob, size_t blob_bytes) {
  woq_blob_header h;
  if (woq_header_init(&h, K, N, group, WOQ_W_INT4_CLIP, (uint32_t)scale_type, (uint32_t)compute_type,
                      zp != NULL, shuffle != NULL) != 0)
    return -1;
  if (blob_bytes < h.total_bytes) return -1;
  memset(blob, 0, h.total_bytes);
  memcpy(blob, &h, sizeof(h));
  uint8_t* qd = blob + h.off_q;
  /* padding nibble = 0 (q = 0, signed two's-complement nibbles): the memset above did it.
   * A qdata byte holds two nibbles of ONE column (woq_blob.h: a lane owns a column), so columns are independent. */
#pragma omp parallel for schedule(static)
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) {
      int shift;
      size_t b = woq_q_byte(&h, k, n, &shift);
      uint8_t u = (uint8_t)(q[(size_t)k * N + n] & 0xf); /* two's-complement nibble of q in [-8,7] */
      qd[b] = (uint8_t)((qd[b] & ~(0xfu << shift)) | (u << shift));
    }
  if (zp) { /* padding zero point: uz = 8 <-> zp = 0 (q = 0 padding nibbles then dequantise to exactly 0) */
    size_t tiles_n = (size_t)h.Npad / WOQ_TILE_N, tiles_k = (size_t)h.Kpad / WOQ_TILE_K;
    size_t n_scale = h.scale_mode == 0 ? tiles_n * (size_t)h.n_groups * 16u : tiles_n * tiles_k * 64u;
    memset(blob + h.off_zp, 8, n_scale);
  }
  /* scales / zeros: walk every 32-row block so that scale_mode 1 (expanded) is filled too */
  for (int n = 0; n < N; ++n)
    for (int kb = 0; kb < h.Kpad; kb += 32) {
      int g = kb / h.group;
      if (kb >= K) continue; /* fully padded block: scale stays 0 */
      if (g >= h.n_groups) g = h.n_groups - 1;
      size_t idx = woq_scale_index(&h, kb, n);
      orc_store_scalar(blob + h.off_scale, idx, scale_type, scales[(size_t)g * N + n]);
      if (zp) (blob + h.off_zp)[idx] = (uint8_t)(zp[(size_t)g * N + n] + 8);
    }
  if (shuffle) memcpy(blob + h.off_shuffle, shuffle, (size_t)K * 4u);
  return 0;
}

ORC_API size_t orc_packed_size(int K, int N, int group, int scale_type, int asym, int act_shuffle) {
  woq_blob_header h;
  if (woq_header_init(&h, K, N, group, WOQ_W_INT4_CLIP, (uint32_t)scale_type, WOQ_C_FP32, asym, act_shuffle) != 0)
    return 0;
  return h.total_bytes;
}

/* a11  dequantize_packed_weight: blob -> fp32 [K,N] (transpose=0) or [N,K] (transpose=1)
 *      reference: qbits.cpp:102-111 -> bestla_weightonly_dispatcher.cpp:46-64 */
ORC_API int orc_dequantize_blob(const uint8_t* blob, float* out, int transpose) {
  woq_blob_header h;
  memcpy(&h, blob, sizeof(h));
  if (h.magic != WOQ_BLOB_MAGIC) return -1;
  const uint8_t* qd = blob + h.off_q;
#pragma omp parallel for schedule(static)
  for (int k = 0; k < h.K; ++k)
    for (int n = 0; n < h.N; ++n) {
      int shift;
      size_t b = woq_q_byte(&h, k, n, &shift);
      int qv = (qd[b] >> shift) & 0xf;
      if (qv & 8) qv -= 16; /* sign-extend the nibble */
      size_t si = woq_scale_index(&h, k, n);
      float s = orc_load_scalar(blob + h.off_scale, si, (int)h.scale_type);
      int zpv = h.off_zp ? (int)(blob + h.off_zp)[si] - 8 : 0;
      float w = (float)(qv - zpv) * s;
      if (transpose)
        out[(size_t)n * h.K + k] = w;
      else
        out[(size_t)k * h.N + n] = w;
    }
  return 0;
}

/* ---------------------------------------------------------------------------------------
 * a3  qbits_woq_linear_ref_impl — THE parity definition
 *     reference: transformers/llm/quantization/autograd/functions.py:41-63
 *       W = dequantize_packed_weight(packw) [K,N] fp32
 *       if act-shuffle: x = index_select(x, 1, g_idx)
 *       out = x.float() @ W (+ bias)
 *     epilogue store: alpha*acc + beta*bias then fp32 or bf16 (bestla_customop.hpp:22-40).
 * x fp32 [M, lda]; out written as out_dtype [M, ldo]. Accumulation is done in double and rounded
 * once to fp32 — a tighter evaluation of the same sum than torch.matmul's fp32 blocked order,
 * so the oracle's own error is negligible next to the tolerance the tests state.
 * ------------------------------------------------------------------------------------- */
ORC_API int orc_woq_linear(const float* x, int lda, const uint8_t* blob, const float* bias, void* out,
                           int out_dtype, int ldo, int M) {
  woq_blob_header h;
  memcpy(&h, blob, sizeof(h));
  if (h.magic != WOQ_BLOB_MAGIC) return -1;
  const int32_t* shuf = h.off_shuffle ? (const int32_t*)(blob + h.off_shuffle) : NULL;
  if (M <= 4) {
    /* few rows (decode shapes): no [K, N] fp32 copy of W — every thread owns 16-column tiles and dequantises element
     * by element with the same formula as orc_dequantize_blob ((q - zp) * scale rounded to fp32), the same
     * k-sequential double sum per output. Full-size matrices then cost milliseconds on a many-core host. */
    const uint8_t* qd = blob + h.off_q;
    const int tiles = (h.N + 15) / 16;
#pragma omp parallel for schedule(static)
    for (int tn = 0; tn < tiles; ++tn) {
      double acc[4][16];
      for (int m = 0; m < M; ++m)
        for (int i = 0; i < 16; ++i) acc[m][i] = 0.0;
      const int n1 = tn * 16 + 16 > h.N ? h.N - tn * 16 : 16;
      for (int k = 0; k < h.K; ++k) {
        float w[16];
        for (int i = 0; i < n1; ++i) {
          int shift;
          const size_t b = woq_q_byte(&h, k, tn * 16 + i, &shift);
          int qv = (qd[b] >> shift) & 0xf;
          if (qv & 8) qv -= 16;
          const size_t si = woq_scale_index(&h, k, tn * 16 + i);
          const float sc = orc_load_scalar(blob + h.off_scale, si, (int)h.scale_type);
          const int zpv = h.off_zp ? (int)(blob + h.off_zp)[si] - 8 : 0;
          w[i] = (float)(qv - zpv) * sc;
        }
        for (int m = 0; m < M; ++m) {
          const double xv = (double)x[(size_t)m * lda + (shuf ? shuf[k] : k)];
          for (int i = 0; i < n1; ++i) acc[m][i] += xv * (double)w[i];
        }
      }
      for (int m = 0; m < M; ++m)
        for (int i = 0; i < n1; ++i) {
          float r = (float)acc[m][i];
          if (bias) r += bias[tn * 16 + i];
          orc_store_scalar(out, (size_t)m * ldo + tn * 16 + i, out_dtype, r);
        }
    }
    return 0;
  }
  float* W = (float*)malloc((size_t)h.K * h.N * sizeof(float));
  if (!W) return -1;
  orc_dequantize_blob(blob, W, 0);
  const int CBLK = 64;
  const int n_blk = (h.N + CBLK - 1) / CBLK;
#pragma omp parallel for schedule(static) collapse(2)
  for (int m = 0; m < M; ++m)
    for (int nb = 0; nb < n_blk; ++nb) {
      double acc[64];
      const int n0 = nb * CBLK, n1 = n0 + CBLK > h.N ? h.N : n0 + CBLK;
      for (int n = n0; n < n1; ++n) acc[n - n0] = 0.0;
      for (int k = 0; k < h.K; ++k) {
        double xv = (double)x[(size_t)m * lda + (shuf ? shuf[k] : k)];
        const float* wr = W + (size_t)k * h.N;
        for (int n = n0; n < n1; ++n) acc[n - n0] += xv * (double)wr[n];
      }
      for (int n = n0; n < n1; ++n) {
        float r = (float)acc[n - n0];
        if (bias) r += bias[n];
        orc_store_scalar(out, (size_t)m * ldo + n, out_dtype, r);
      }
    }
  free(W);
  return 0;
}

/* Same contraction but fp32 accumulate, k-sequential, straight from the packed nibbles with
 * on-the-fly dequantisation — the arithmetic a BesTLA fp32 core does per K-block
 * (bestla_weightonly_dispatcher.cpp:150-178: unpack int4 -> fp32, x scale, FMA, fp32 accumulate).
 * This is the function bench.py times as cpu_baseline (kind "port"): it streams the int4 blob
 * like the reference's CPU kernel does, instead of materialising W. M == 1 rows at a time. */
/* Loop order chosen for the host's vector units (AVX2 + FMA; the GPU boxes' EPYC hosts and the build container both
 * have them): for one 16-column tile, one 32-row scale block at a time, the 16 columns are the vector lanes — a blob
 * word holds 8 consecutive-k nibbles of ONE column, so word w of lanes (kq, i = 0..15) is a stride-4 gather, the
 * nibbles are sign-extended with (u ^ 8) - 8 and multiplied by the broadcast activation. Zero points enter as
 * -zp * sum(x) per block, like BesTLA's asym cores (bestla_weightonly_dispatcher.cpp:154-160,205-207). */
__attribute__((target("avx2,fma"))) ORC_API int orc_woq_gemv_stream(const float* x, const uint8_t* blob,
                                                                   const float* bias, float* out) {
  woq_blob_header h;
  memcpy(&h, blob, sizeof(h));
  if (h.magic != WOQ_BLOB_MAGIC) return -1;
  const int tiles_k = h.Kpad / WOQ_TILE_K, tiles_n = h.Npad / WOQ_TILE_N;
  const int32_t* shuf = h.off_shuffle ? (const int32_t*)(blob + h.off_shuffle) : NULL;
  float* xs = (float*)calloc((size_t)h.Kpad, sizeof(float));
  for (int k = 0; k < h.K; ++k) xs[k] = x[shuf ? shuf[k] : k];
  /* sum of the activations of every 32-row block (zero-point term) */
  float* xsum = (float*)calloc((size_t)tiles_k * 4, sizeof(float));
  for (int b32 = 0; b32 < tiles_k * 4; ++b32) {
    float t = 0.f;
    for (int r = 0; r < 32; ++r) t += xs[b32 * 32 + r];
    xsum[b32] = t;
  }
#pragma omp parallel for schedule(static)
  for (int tn = 0; tn < tiles_n; ++tn) {
    float acc[16];
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int kt = 0; kt < tiles_k; ++kt) {
      const uint32_t* tile = (const uint32_t*)(blob + h.off_q) + ((size_t)tn * tiles_k + kt) * 256u;
      for (int s = 0; s < 4; ++s) { /* 32-row blocks: the finest scale granularity */
        const int kb = kt * 128 + s * 32, hh = s >> 1;
        float part[16];
        for (int i = 0; i < 16; ++i) part[i] = 0.f;
        for (int kq2 = 0; kq2 < 2; ++kq2) {
          const int kq = 2 * (s & 1) + kq2;
          for (int p = 0; p < 2; ++p) { /* word 2 hh + p of lane (kq, i): k = kb + 16 kq2 + 8 p + jj */
            const float* xk = xs + kb + 16 * kq2 + 8 * p;
            const uint32_t* wp = tile + (size_t)(kq * 16) * 4 + hh * 2 + p;
#pragma omp simd
            for (int i = 0; i < 16; ++i) {
              const uint32_t w = wp[i * 4];
              float t = 0.f;
              for (int jj = 0; jj < 8; ++jj) {
                const int u = (int)((w >> (8 * (jj & 3) + 4 * (jj >> 2))) & 0xfu);
                t += (float)((u ^ 8) - 8) * xk[jj];
              }
              part[i] += t;
            }
          }
        }
        for (int i = 0; i < 16; ++i) {
          const size_t si = woq_scale_index(&h, kb, tn * 16 + i);
          const float sc = orc_load_scalar(blob + h.off_scale, si, (int)h.scale_type);
          const int zpv = h.off_zp ? (int)(blob + h.off_zp)[si] - 8 : 0;
          acc[i] += (part[i] - (float)zpv * xsum[kt * 4 + s]) * sc;
        }
      }
    }
    for (int i = 0; i < 16; ++i) {
      int n = tn * 16 + i;
      if (n < h.N) out[n] = acc[i] + (bias ? bias[n] : 0.f);
    }
  }
  free(xs);
  free(xsum);
  return 0;
}

/* ---------------------------------------------------------------------------------------
 * a17  ops between the linears. The reference runs stock HF transformers modules here
 *      (SURVEY.md §8 a17); these follow HF's definitions and are pinned against HF outputs
 *      generated in the build container (tests/golden/hf_ops_*.npz).
 * ------------------------------------------------------------------------------------- */
/* HF LlamaRMSNorm.forward: x * rsqrt(mean(x^2) + eps) * weight  (fp32 math).
 * NOT the Neural-Engine variant rsqrt((sum+eps)/d) (runtime/executor/src/operators/rmsnorm.cpp:117). */
ORC_API void orc_rmsnorm(const float* x, const float* weight, float eps, int rows, int d, float* out) {
  for (int r = 0; r < rows; ++r) {
    double ss = 0.0;
    for (int i = 0; i < d; ++i) ss += (double)x[(size_t)r * d + i] * x[(size_t)r * d + i];
    float inv = 1.0f / sqrtf((float)(ss / d) + eps);
    for (int i = 0; i < d; ++i) out[(size_t)r * d + i] = x[(size_t)r * d + i] * inv * weight[i];
  }
}

/* HF apply_rotary_pos_emb (rotate_half form): for head dim D, pair (i, i + D/2),
 * inv_freq_i = theta^(-2i/D), angle = pos * inv_freq_i:
 *   out[i]       = x[i] * cos - x[i + D/2] * sin
 *   out[i + D/2] = x[i + D/2] * cos + x[i] * sin
 * x: [tokens, heads, D] in place; pos: int32 [tokens]. */
ORC_API void orc_rope(float* x, const int32_t* pos, int tokens, int heads, int D, float theta) {
  int half = D / 2;
  for (int t = 0; t < tokens; ++t)
    for (int i = 0; i < half; ++i) {
      float inv_freq = 1.0f / powf(theta, (float)(2 * i) / (float)D);
      float ang = (float)pos[t] * inv_freq;
      float c = cosf(ang), s = sinf(ang);
      for (int hh = 0; hh < heads; ++hh) {
        float* p = x + ((size_t)t * heads + hh) * D;
        float a = p[i], b = p[i + half];
        p[i] = a * c - b * s;
        p[i + half] = b * c + a * s;
      }
    }
}

/* HF LlamaMLP: down(silu(gate) * up) — the elementwise part. */
ORC_API void orc_silu_mul(const float* gate, const float* up, size_t n, float* out) {
  for (size_t i = 0; i < n; ++i) out[i] = gate[i] / (1.0f + expf(-gate[i])) * up[i];
}

/* GPT-2 "gelu_new" (tanh form) and exact erf GeLU. */
ORC_API void orc_gelu_tanh(const float* x, size_t n, float* out) {
  for (size_t i = 0; i < n; ++i) {
    float v = x[i];
    out[i] = 0.5f * v * (1.0f + tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v)));
  }
}
ORC_API void orc_gelu_erf(const float* x, size_t n, float* out) {
  for (size_t i = 0; i < n; ++i) out[i] = 0.5f * x[i] * (1.0f + erff(x[i] * 0.7071067811865476f));
}

/* Single-query attention over a KV cache (decode step), grouped-query aware.
 * q [heads, D]; kcache/vcache [ctx, kv_heads, D] (already rotated); out [heads, D]. */
ORC_API void orc_attn_decode(const float* q, const float* kcache, const float* vcache, int heads, int kv_heads,
                             int D, int ctx, float* out) {
  int rep = heads / kv_heads;
  float scale = 1.0f / sqrtf((float)D);
  float* p = (float*)malloc((size_t)ctx * sizeof(float));
  for (int hh = 0; hh < heads; ++hh) {
    int kh = hh / rep;
    float mx = -INFINITY;
    for (int t = 0; t < ctx; ++t) {
      double d = 0.0;
      const float* kk = kcache + ((size_t)t * kv_heads + kh) * D;
      for (int i = 0; i < D; ++i) d += (double)q[(size_t)hh * D + i] * kk[i];
      p[t] = (float)d * scale;
      mx = p[t] > mx ? p[t] : mx;
    }
    double den = 0.0;
    for (int t = 0; t < ctx; ++t) {
      p[t] = expf(p[t] - mx);
      den += p[t];
    }
    for (int i = 0; i < D; ++i) {
      double a = 0.0;
      for (int t = 0; t < ctx; ++t) a += (double)p[t] * vcache[((size_t)t * kv_heads + kh) * D + i];
      out[(size_t)hh * D + i] = (float)(a / den);
    }
  }
  free(p);
}
