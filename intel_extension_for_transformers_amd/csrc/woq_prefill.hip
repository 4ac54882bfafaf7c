// woq_prefill.hip — the non-linear kernels of the prompt (prefill) pass of the decode engine: token embedding
// for a batch of rows, RoPE + KV-cache append, causal attention over the cache on the matrix cores, last-row gather.
//
// What they replace: stock HF module forwards the reference runs as PyTorch CPU ops around its
// qbits linears during `model.generate`'s first forward — LlamaRotaryEmbedding / apply_rotary_pos_emb (rotate_half
// form), the KV cache `torch.cat`, and LlamaAttention's softmax(QK^T / sqrt(d) + causal mask) V. The linears of the
// same pass are woq_gemm_f16.hip.
//
// Attention (attn_prefill_kernel): one workgroup = 128 query rows of one head of one sequence, 4 waves x 32 rows;
// the K / V rows of the sequence's cache — positions [0, start + row], i.e. earlier chunks and this chunk alike —
// stream through LDS in tiles of 64 positions:
//  * S^T = K Q^T per 16-position tile (v_mfma_f32_16x16x32_f16, A = K fragment read from a row-major LDS tile in a
//    16-B-slot XOR swizzle, B = Q^T fragments held in registers): the result leaves query i16 in lane i16 with
//    positions 4*kq + j — which IS the B-operand shape of the next product, so probabilities never touch LDS;
//  * online softmax in the exp2 domain, fp32, per query = per lane column (two cross-quarter shuffles per tile);
//  * O^T = V^T P^T: A = V^T fragment = two ds_read_b64 from a TRANSPOSED V tile ([d][position], written with a
//    4 x 8 register transpose and a quad-chunk XOR swizzle so both the writes and the reads are conflict-free),
//    B = the packed fp16 probabilities; the output again has query i16 in lane i16, so the running rescale is a
//    plain per-lane multiply.
// Tiles entirely above a wave's causal diagonal are skipped by that wave; the workgroups with the most tiles are
// scheduled first. One LDS buffer, two barriers per tile (a two-buffer, one-barrier variant measured 28 % slower:
// 450 vs 353 us per layer at 4 x 2048 tokens — two workgroups per CU already overlap each other's staging). fp32 accumulation throughout; Q, K, V, P enter the MFMAs as fp16.
#include <cstdlib>

#include "woq_device.h"
#include "woq_host.h"
#include "woq_kv_codec.h"
#include "../../include/woq_hip_experimental.h"

namespace woq {

// ---- embedding rows: h[m][:] = embed[token[m]][:] (fp32 residual stream) ----------------------------------------
__global__ __launch_bounds__(256) void embed_rows_kernel(const void* __restrict__ embed, int dtype,
                                                         const int32_t* __restrict__ tokens, int hidden,
                                                         float* __restrict__ out) {
  const int m = blockIdx.x;
  const size_t src = (size_t)tokens[m] * hidden;
  for (int i = threadIdx.x; i < hidden; i += 256) out[(size_t)m * hidden + i] = load_f32(embed, src + i, dtype);
}

// ---- RoPE (HF rotate_half form) on q and k, KV append ------------------------------------------------------------
// qkv fp16 [M][(heads + 2 kv_heads) * HD]: q rotated in place; k rotated -> K cache; v -> V cache.
// Row m = sequence m / T, position start + m % T. One thread = 8 consecutive d of the first half of one head slot
// (and their partners in the second half): 16-byte loads and stores throughout.
template <int KVD>
__global__ __launch_bounds__(256) void rope_append_kernel(_Float16* __restrict__ qkv, int M, int T, int start,
                                                          int heads, int kv_heads, int HD,
                                                          const float* __restrict__ cs, const float* __restrict__ sn,
                                                          void* __restrict__ kcache, void* __restrict__ vcache,
                                                          size_t seq_stride_elems) {
  const int half = HD >> 1, cph = half >> 3;  // 8-element chunks per half head
  const int nslots = heads + 2 * kv_heads;
  const size_t per_row = (size_t)nslots * cph;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)M * per_row) return;
  const int m = (int)(gid / per_row);
  const int rem = (int)(gid % per_row);
  const int slot = rem / cph, c8 = (rem % cph) * 8;
  const int seq = m / T, pos = start + m % T;
  _Float16* x = qkv + (size_t)m * nslots * HD + (size_t)slot * HD;
  const h8 xa = *(const h8*)(x + c8), xb = *(const h8*)(x + c8 + half);
  float ra[8], rb[8];
  if (slot < heads + kv_heads) {
    const float4_t c0 = *(const float4_t*)(cs + (size_t)pos * half + c8), c1 = *(const float4_t*)(cs + (size_t)pos * half + c8 + 4);
    const float4_t s0 = *(const float4_t*)(sn + (size_t)pos * half + c8), s1 = *(const float4_t*)(sn + (size_t)pos * half + c8 + 4);
    const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = (float)xa[j], b = (float)xb[j];
      ra[j] = a * cc[j] - b * ss[j];
      rb[j] = b * cc[j] + a * ss[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) ra[j] = (float)xa[j], rb[j] = (float)xb[j];
  }
  if (slot < heads) {
    kv_store8<WOQ_F16>(x, c8, ra);
    kv_store8<WOQ_F16>(x, c8 + half, rb);
  } else {
    const int kh = slot < heads + kv_heads ? slot - heads : slot - heads - kv_heads;
    void* cache = slot < heads + kv_heads ? kcache : vcache;
    const size_t e = (size_t)seq * seq_stride_elems + ((size_t)pos * kv_heads + kh) * HD;
    kv_store8<KVD>(cache, e + c8, ra);
    kv_store8<KVD>(cache, e + c8 + half, rb);
  }
}

// The same pass with a per-head RMSNorm on q and k in front of the rotation (Qwen3's q_norm / k_norm, HF Qwen3RMSNorm in
// fp32: x * rsqrt(mean(x^2) + eps) * w). A head slot is spread over cph = HD / 16 neighbouring lanes (cph a power of
// two: a group never straddles a wave), so its sum of squares is a butterfly over those lanes — no LDS, no barrier.
// Normalised and rotated in fp32 from the fp16 projections, rounded ONCE (q to fp16, k to the cache type); v untouched.
// The grid is padded to whole waves and no thread leaves early: threads past the end (whole groups: the thread count
// is a multiple of cph) recompute the last chunk and store nothing, so every lane a butterfly reads is there.
template <int KVD>
__global__ __launch_bounds__(256) void rope_append_qkn_kernel(_Float16* __restrict__ qkv, int M, int T, int start,
                                                              int heads, int kv_heads, int HD,
                                                              const float* __restrict__ cs, const float* __restrict__ sn,
                                                              void* __restrict__ kcache, void* __restrict__ vcache,
                                                              size_t seq_stride_elems, const float* __restrict__ q_norm,
                                                              const float* __restrict__ k_norm, float eps) {
  const int half = HD >> 1, cph = half >> 3;
  const int nslots = heads + 2 * kv_heads;
  const size_t per_row = (size_t)nslots * cph, total = (size_t)M * per_row;
  const size_t gid0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = gid0 < total;
  const size_t gid = live ? gid0 : total - 1;
  const int m = (int)(gid / per_row);
  const int rem = (int)(gid % per_row);
  const int slot = rem / cph, c8 = (rem % cph) * 8;
  const int seq = m / T, pos = start + m % T;
  _Float16* x = qkv + (size_t)m * nslots * HD + (size_t)slot * HD;
  const h8 xa = *(const h8*)(x + c8), xb = *(const h8*)(x + c8 + half);
  float a[8], b[8], ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = (float)xa[j], b[j] = (float)xb[j];
    ss = fmaf(a[j], a[j], ss);
    ss = fmaf(b[j], b[j], ss);
  }
  for (int o = 1; o < cph; o <<= 1) ss += __shfl_xor(ss, o, 64);  // every lane of the wave takes part
  float ra[8], rb[8];
  if (slot < heads + kv_heads) {
    const float r = 1.0f / sqrtf(ss / (float)HD + eps);
    const float* w = slot < heads ? q_norm : k_norm;
    const float4_t wa0 = *(const float4_t*)(w + c8), wa1 = *(const float4_t*)(w + c8 + 4);
    const float4_t wb0 = *(const float4_t*)(w + c8 + half), wb1 = *(const float4_t*)(w + c8 + half + 4);
    const float wa[8] = {wa0.x, wa0.y, wa0.z, wa0.w, wa1.x, wa1.y, wa1.z, wa1.w};
    const float wb[8] = {wb0.x, wb0.y, wb0.z, wb0.w, wb1.x, wb1.y, wb1.z, wb1.w};
    const float4_t c0 = *(const float4_t*)(cs + (size_t)pos * half + c8), c1 = *(const float4_t*)(cs + (size_t)pos * half + c8 + 4);
    const float4_t s0 = *(const float4_t*)(sn + (size_t)pos * half + c8), s1 = *(const float4_t*)(sn + (size_t)pos * half + c8 + 4);
    const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float na = a[j] * (r * wa[j]), nb = b[j] * (r * wb[j]);
      ra[j] = na * cc[j] - nb * sv[j];
      rb[j] = nb * cc[j] + na * sv[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) ra[j] = a[j], rb[j] = b[j];
  }
  if (!live) return;
  if (slot < heads) {
    kv_store8<WOQ_F16>(x, c8, ra);
    kv_store8<WOQ_F16>(x, c8 + half, rb);
  } else {
    const int kh = slot < heads + kv_heads ? slot - heads : slot - heads - kv_heads;
    void* cache = slot < heads + kv_heads ? kcache : vcache;
    const size_t e = (size_t)seq * seq_stride_elems + ((size_t)pos * kv_heads + kh) * HD;
    kv_store8<KVD>(cache, e + c8, ra);
    kv_store8<KVD>(cache, e + c8 + half, rb);
  }
}

// ---- causal attention over the cache -----------------------------------------------------------------------------
constexpr int AQB = 128;  // query rows per workgroup
constexpr int AKT = 64;   // cache positions per tile
constexpr int AVRB = 144; // bytes per V^T row: 64 positions x 2 B + 16 pad (conflict-free ds_read_b64, see header)

template <int HD>
__host__ __device__ constexpr int attn_lds_bytes() { return AKT * HD * 2 + HD * AVRB; }

template <int KVD, int HD>
__global__ __launch_bounds__(256, 2) void attn_prefill_kernel(const _Float16* __restrict__ qkv, int T, int start,
                                                              int heads, int kv_heads, const void* __restrict__ kcache,
                                                              const void* __restrict__ vcache, size_t seq_stride_elems,
                                                              _Float16* __restrict__ out, int n_qblocks, int window,
                                                              int prio) {
  constexpr int CPR = HD / 8;   // 16-B chunks per K row
  constexpr int DC = HD / 32;   // 32-wide d chunks of the QK^T contraction
  constexpr int DT = HD / 16;   // 16-wide d tiles of the output
  constexpr int KRB = HD * 2;   // K tile row bytes
  extern __shared__ __attribute__((aligned(16))) unsigned char asm_raw[];
  unsigned char* ks = asm_raw;                // [64][HD] fp16, chunk slot swizzled
  unsigned char* vs = asm_raw + AKT * KRB;    // [HD][AVRB]: V^T
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;
  // Which (sequence, head, query block). 3-D grid: x = query block (longest first), y = head, z = sequence. 1-D grid
  // (gridDim.y == 1, heads % 8 == 0): XCD-aware — workgroup ids go round-robin over the 8 XCDs, so id & 7 is the XCD;
  // XCD x takes heads [x heads / 8, (x + 1) heads / 8) of every sequence and walks their query blocks one head after the
  // other. The query blocks of a head (and the query heads of a kv group) then share ONE L2: with the 3-D order a
  // head's 16 blocks ran on all eight XCDs and every L2 had to hold every active head's K / V (4 x 2048 tokens x 32
  // heads = 134 MB per layer, re-read 8.5 times on average: the launch ran at the fabric's ~3.4 TB/s, not on its MFMAs).
  int qb, h, seq;
  if (gridDim.y == 1 && (heads & 7) == 0) {  // a 3-D grid with heads % 8 == 0 has gridDim.y >= 8; heads == 1 is 3-D too
    const int L = (int)blockIdx.x, xcd = L & 7, r = L >> 3;
    const int hp = heads >> 3, g = r / n_qblocks;
    qb = n_qblocks - 1 - r % n_qblocks;
    h = xcd * hp + g % hp;
    seq = g / hp;
  } else {
    qb = n_qblocks - 1 - (int)blockIdx.x;  // longest workgroups first
    h = blockIdx.y, seq = blockIdx.z;
  }
  const int kh = h / (heads / kv_heads);
  const int nslots = heads + 2 * kv_heads;
  const int q0 = qb * AQB + wid * 32;  // this wave's first query row (within the chunk)
  const size_t row_elems = (size_t)nslots * HD;
  const size_t cache0 = (size_t)seq * seq_stride_elems + (size_t)kh * HD;
  const size_t cache_row = (size_t)kv_heads * HD;
  const int kv_len = start + min(qb * AQB + AQB, T);  // positions this workgroup may look at
  const int n_tiles = (kv_len + AKT - 1) / AKT;
  // sliding window (0 = none): query position p sees [p + 1 - window, p]; tiles wholly below the workgroup's first
  // query's window are never loaded
  const int tile0 = window > 0 ? max(0, start + qb * AQB + 1 - window) / AKT : 0;
  const float sc = 1.44269504088896f / sqrtf((float)HD);  // softmax scale in the exp2 domain

  // Q^T fragments: lane (query i16 of row tile rt, quarter kq) holds d = 32c + 8kq .. +8
  h8 qf[2][DC];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int qr = min(q0 + rt * 16 + i16, T - 1);
    const _Float16* qp = qkv + ((size_t)seq * T + qr) * row_elems + (size_t)h * HD;
#pragma unroll
    for (int c = 0; c < DC; ++c) qf[rt][c] = *(const h8*)(qp + c * 32 + kq * 8);
  }
  float4_t o[DT][2];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) o[dt][rt] = (float4_t){0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {-INFINITY, -INFINITY}, l_part[2] = {0.f, 0.f};

  // ---- tile movers. K: thread -> rows tid/CPR + (256/CPR) i, chunk tid % CPR. V: thread -> 4 positions x 8 d ----
  constexpr int KPT = AKT * CPR / 256;  // K vectors per thread
  constexpr int KRS = 256 / CPR;        // K row step between a thread's vectors
  const int k_row = tid / CPR, k_chunk = tid % CPR;
  const int v_g = (tid / CPR), v_c = tid % CPR;  // position quad (0..15 live), d chunk
  const bool v_live = v_g < 16;
  h8 kreg[KPT], vreg[4];
  auto fetch = [&](int tile) {
    const int t0 = tile * AKT;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int t = min(t0 + k_row + i * KRS, kv_len - 1);
      kreg[i] = kv_load8<KVD>(kcache, cache0 + (size_t)t * cache_row + k_chunk * 8);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = min(t0 + min(v_g, 15) * 4 + r, kv_len - 1);
      vreg[r] = kv_load8<KVD>(vcache, cache0 + (size_t)t * cache_row + v_c * 8);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int row = k_row + i * KRS;
      const int f = HD == 128 ? (row & 15) : ((row >> 1) & 7);
      *(h8*)(ks + row * KRB + ((k_chunk ^ f) << 4)) = kreg[i];
    }
    if (v_live) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {  // d = 8 v_c + i: positions 4 v_g .. +3
        const h4 col = {vreg[0][i], vreg[1][i], vreg[2][i], vreg[3][i]};
        *(h4*)(vs + (v_c * 8 + i) * AVRB + ((v_g ^ (v_c & 15)) << 3)) = col;
      }
    }
  };

  fetch(tile0);
  for (int tile = tile0; tile < n_tiles; ++tile) {
    __syncthreads();  // everyone is done with the previous tile
    stage();
    __syncthreads();
    if (tile + 1 < n_tiles) fetch(tile + 1);  // flies under this tile's MFMAs
    const int t0 = tile * AKT;
    if (t0 > start + q0 + 31) continue;  // wholly above this wave's diagonal (wave-uniform)
    if (window > 0 && t0 + AKT - 1 < start + q0 + 1 - window) continue;  // wholly below this wave's windows

    // ---- S^T = K Q^T ----
    if (prio) __builtin_amdgcn_s_setprio(1);  // MFMA phases outrank the other workgroup's softmax on the same SIMD
    float4_t s[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) s[a][rt] = (float4_t){0.f, 0.f, 0.f, 0.f};
      const int row = a * 16 + i16;
      const int f = HD == 128 ? (row & 15) : ((row >> 1) & 7);
#pragma unroll
      for (int c = 0; c < DC; ++c) {
        const h8 kf = *(const h8*)(ks + row * KRB + (((c * 4 + kq) ^ f) << 4));
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) s[a][rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[rt][c], s[a][rt], 0, 0, 0);
      }
    }
    if (prio) __builtin_amdgcn_s_setprio(0);
    // ---- causal mask + online softmax (query = lane column i16, positions 16a + 4kq + j) ----
    // some position of the tile may exceed some query of the wave, or fall below some query's window
    const bool diag = t0 + AKT - 1 > start + q0 || (window > 0 && t0 < start + q0 + 32 - window);
    h8 pb[2][2];
    if (diag) {  // wave-uniform: the mask work (compare + select per score) only on tiles that touch the diagonal or a
                 // window edge — most tiles of a long prompt are wholly visible
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const int qpos = start + q0 + rt * 16 + i16;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int tp = t0 + a * 16 + kq * 4 + j;
            if (tp > qpos || (window > 0 && tp < qpos + 1 - window)) s[a][rt][j] = -INFINITY;
          }
      }
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      float mx = -INFINITY;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) mx = fmaxf(mx, s[a][rt][j]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run[rt], mx * sc);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;  // a row with nothing visible yet: keep exp2 finite
      const float alpha = __builtin_amdgcn_exp2f(m_run[rt] - m_use);  // raw v_exp_f32: arguments are <= 0
      const bool moved = m_new != m_run[rt];
      m_run[rt] = m_new;
      float ps = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[a][rt][j], sc, -m_use));
          ps += p;
          pb[a >> 1][rt][(a & 1) * 4 + j] = (_Float16)p;
        }
      l_part[rt] = fmaf(l_part[rt], alpha, ps);
      // once the running maxima have settled (most tiles after the first few) alpha is exactly 1 for every query of
      // the wave: skip the rescale of the output accumulators then (wave-uniform branch)
      if (__builtin_amdgcn_ballot_w64(moved) != 0) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt][rt] *= alpha;
      }
    }
    // ---- O^T += V^T P^T ----
    if (prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int d = dt * 16 + i16;
        const int sw = (d >> 3) & 15;
        const unsigned char* vrow = vs + d * AVRB;
        const u32x2 lo = *(const u32x2*)(vrow + (((8 * b + kq) ^ sw) << 3));
        const u32x2 hi = *(const u32x2*)(vrow + (((8 * b + 4 + kq) ^ sw) << 3));
        const h8 vf = __builtin_bit_cast(h8, (u32x4){lo.x, lo.y, hi.x, hi.y});
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) o[dt][rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[b][rt], o[dt][rt], 0, 0, 0);
      }
    if (prio) __builtin_amdgcn_s_setprio(0);
  }
  // ---- finish: divide by the row sums, store fp16 [M][heads * HD] ----
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    float l = l_part[rt];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = l > 0.f ? 1.f / l : 0.f;
    const int qr = q0 + rt * 16 + i16;
    if (qr < T) {
      _Float16* op = out + ((size_t)seq * T + qr) * ((size_t)heads * HD) + (size_t)h * HD + kq * 4;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const float4_t v = o[dt][rt] * inv;
        *(h4*)(op + dt * 16) = (h4){(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
      }
    }
  }
}

// last row of every sequence -> dst fp32 [n_seq][hidden]
__global__ __launch_bounds__(256) void gather_last_kernel(const float* __restrict__ h, int T, int hidden,
                                                          float* __restrict__ dst) {
  const int seq = blockIdx.x;
  const float* src = h + ((size_t)seq * T + (T - 1)) * hidden;
  for (int i = threadIdx.x; i < hidden; i += 256) dst[(size_t)seq * hidden + i] = src[i];
}

// ---- host launchers ---------------------------------------------------------------------------------------------
void launch_embed_rows(const void* embed, int dtype, const int32_t* tokens, int M, int hidden, float* out,
                       hipStream_t st) {
  hipLaunchKernelGGL(embed_rows_kernel, dim3(M), dim3(256), 0, st, embed, dtype, tokens, hidden, out);
}

int launch_rope_append(_Float16* qkv, int n_seq, int T, int start, int heads, int kv_heads, int HD, const float* cs,
                       const float* sn, void* kcache, void* vcache, int kv_dtype, size_t seq_stride_elems,
                       hipStream_t st, const float* q_norm, const float* k_norm, float qk_eps) {
  if ((HD & 15) != 0) return woq::fail("QBits: head_dim must be a multiple of 16");
  const int M = n_seq * T;
  const size_t threads = (size_t)M * (heads + 2 * kv_heads) * (HD / 16);
  const dim3 grid((unsigned)((threads + 255) / 256));
  if ((q_norm != nullptr) != (k_norm != nullptr)) return woq::fail("QBits: q_norm and k_norm come together");
  if (q_norm != nullptr) {
    const int cph = HD / 16;  // lanes per head slot: the butterfly wants a power of two inside one wave
    if ((cph & (cph - 1)) != 0 || cph > 64)
      return woq::fail("QBits: a q/k norm needs head_dim = 16 * a power of two (at most 1024)");
#define WOQ_ROPE_QKN_CASE(KVD)                                                                                      \
  if (kv_dtype == KVD) {                                                                                            \
    hipLaunchKernelGGL(rope_append_qkn_kernel<KVD>, grid, dim3(256), 0, st, qkv, M, T, start, heads, kv_heads, HD,  \
                       cs, sn, kcache, vcache, seq_stride_elems, q_norm, k_norm, qk_eps);                           \
    return 0;                                                                                                       \
  }
    WOQ_ROPE_QKN_CASE(WOQ_F16)
    WOQ_ROPE_QKN_CASE(WOQ_BF16)
    WOQ_ROPE_QKN_CASE(WOQ_FP8_E4M3)
#undef WOQ_ROPE_QKN_CASE
    return woq::fail("QBits: unsupported KV cache dtype");
  }
  if (kv_dtype == WOQ_F16)
    hipLaunchKernelGGL(rope_append_kernel<WOQ_F16>, grid, dim3(256), 0, st, qkv, M, T, start, heads, kv_heads, HD, cs,
                       sn, kcache, vcache, seq_stride_elems);
  else if (kv_dtype == WOQ_BF16)
    hipLaunchKernelGGL(rope_append_kernel<WOQ_BF16>, grid, dim3(256), 0, st, qkv, M, T, start, heads, kv_heads, HD, cs,
                       sn, kcache, vcache, seq_stride_elems);
  else if (kv_dtype == WOQ_FP8_E4M3)
    hipLaunchKernelGGL(rope_append_kernel<WOQ_FP8_E4M3>, grid, dim3(256), 0, st, qkv, M, T, start, heads, kv_heads, HD,
                       cs, sn, kcache, vcache, seq_stride_elems);
  else
    return woq::fail("QBits: unsupported KV cache dtype");
  return 0;
}

template <int KVD, int HD>
static int launch_attn_prefill_t(const _Float16* qkv, int n_seq, int T, int start, int heads, int kv_heads,
                                 const void* kcache, const void* vcache, size_t seq_stride_elems, _Float16* out,
                                 int window, hipStream_t st) {
  auto k = attn_prefill_kernel<KVD, HD>;
  const int nqb = (T + AQB - 1) / AQB;
  const long long total = (long long)nqb * heads * n_seq;
  const dim3 grid = ((heads & 7) == 0 && total < (1ll << 31)) ? dim3((unsigned)total)
                                                                        : dim3((unsigned)nqb, (unsigned)heads, (unsigned)n_seq);
  // s_setprio 1 around the two MFMA phases of a tile: the MFMAs of one workgroup outrank the softmax VALU of the other
  // workgroup on the same SIMD, so the two fall into alternating phases instead of queueing behind each other. Same
  // box, 8 layers at 4 x 2048: 24.42 -> 24.30 ms (attention -5 %, profiles/r03as). Always on: prio = 1.
  hipLaunchKernelGGL(k, grid, dim3(256), attn_lds_bytes<HD>(), st, qkv, T, start, heads, kv_heads, kcache, vcache,
                     seq_stride_elems, out, nqb, window, 1);
  return 0;
}

int launch_attn_prefill(const _Float16* qkv, int n_seq, int T, int start, int heads, int kv_heads, int HD,
                        const void* kcache, const void* vcache, int kv_dtype, size_t seq_stride_elems, _Float16* out,
                        int window, hipStream_t st) {
  if (HD != 64 && HD != 128) return woq::fail("QBits: attention head_dim must be 64 or 128");
#define WOQ_ATTN_CASE(KVD)                                                                                          \
  if (kv_dtype == KVD)                                                                                              \
    return HD == 128 ? launch_attn_prefill_t<KVD, 128>(qkv, n_seq, T, start, heads, kv_heads, kcache, vcache,       \
                                                       seq_stride_elems, out, window, st)                          \
                     : launch_attn_prefill_t<KVD, 64>(qkv, n_seq, T, start, heads, kv_heads, kcache, vcache,        \
                                                      seq_stride_elems, out, window, st);
  WOQ_ATTN_CASE(WOQ_F16)
  WOQ_ATTN_CASE(WOQ_BF16)
  WOQ_ATTN_CASE(WOQ_FP8_E4M3)
#undef WOQ_ATTN_CASE
  return woq::fail("QBits: unsupported KV cache dtype");
}

void launch_gather_last(const float* h, int n_seq, int T, int hidden, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(gather_last_kernel, dim3(n_seq), dim3(256), 0, st, h, T, hidden, dst);
}

}  // namespace woq

// ---- test entry points (include/woq_hip_experimental.h): the prompt pass's two launches on their own ----------------
extern "C" {

WOQ_API int woq_probe_rope_append(void* qkv, int n_seq, int T, int start, int heads, int kv_heads, int head_dim,
                                  const float* cos_dev, const float* sin_dev, void* kcache, void* vcache, int kv_dtype,
                                  size_t seq_stride_elems, void* stream) {
  WOQ_TRY
  WOQ_CHECK(n_seq > 0 && T > 0 && start >= 0 && heads > 0 && kv_heads > 0, "QBits: bad rope_append shape");
  const int rc = woq::launch_rope_append((_Float16*)qkv, n_seq, T, start, heads, kv_heads, head_dim, cos_dev, sin_dev,
                                         kcache, vcache, kv_dtype, seq_stride_elems, (hipStream_t)stream);
  if (rc) return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

WOQ_API int woq_probe_rope_append_qknorm(void* qkv, int n_seq, int T, int start, int heads, int kv_heads, int head_dim,
                                         const float* cos_dev, const float* sin_dev, void* kcache, void* vcache,
                                         int kv_dtype, size_t seq_stride_elems, const float* q_norm_dev,
                                         const float* k_norm_dev, float eps, void* stream) {
  WOQ_TRY
  WOQ_CHECK(n_seq > 0 && T > 0 && start >= 0 && heads > 0 && kv_heads > 0, "QBits: bad rope_append shape");
  WOQ_CHECK(q_norm_dev != nullptr && k_norm_dev != nullptr, "QBits: q_norm and k_norm come together");
  const int rc = woq::launch_rope_append((_Float16*)qkv, n_seq, T, start, heads, kv_heads, head_dim, cos_dev, sin_dev,
                                         kcache, vcache, kv_dtype, seq_stride_elems, (hipStream_t)stream, q_norm_dev,
                                         k_norm_dev, eps);
  if (rc) return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

WOQ_API int woq_probe_attn_prefill(const void* qkv, int n_seq, int T, int start, int heads, int kv_heads, int head_dim,
                                   const void* kcache, const void* vcache, int kv_dtype, size_t seq_stride_elems,
                                   void* out, int window, void* stream) {
  WOQ_TRY
  WOQ_CHECK(n_seq > 0 && T > 0 && start >= 0 && heads > 0 && kv_heads > 0 && heads % kv_heads == 0 && window >= 0,
            "QBits: bad attention shape");
  const int rc = woq::launch_attn_prefill((const _Float16*)qkv, n_seq, T, start, heads, kv_heads, head_dim, kcache,
                                          vcache, kv_dtype, seq_stride_elems, (_Float16*)out, window,
                                          (hipStream_t)stream);
  if (rc) return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

}  // extern "C"
