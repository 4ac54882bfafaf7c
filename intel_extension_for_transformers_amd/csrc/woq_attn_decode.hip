// woq_attn_decode.hip — the attention of a decode step (one new token against the KV cache): its kernels outside the
// fused qkv launch, the plan that decides how a step's attention runs, and the launchers that follow the plan.
//
// Reference path replaced: stock HF eager attention over the KV cache run by PyTorch CPU ops.
// Kernels: attn_decode_kernel (one workgroup per query head and context slice: the body of woq_attn_decode.h on plain
// fp32 inputs; attn_decode_qkn_kernel: the same with a per-head q / k RMSNorm), attn_combine_kernel (the slices' merge as a launch of its own) and attn_decode_mfma_kernel (grouped-query
// models at long contexts: one matrix-core workgroup per kv head and slice). The fused form — the same body behind the
// qkv GEMV's strips — is woq_gemv_attn.hip; the in-launch merges are woq_attn_merge.h.
// plan_attn_decode (host side, below) decides once per call which form runs, how its slices merge and their geometry;
// it is pure arithmetic, which the CPU suite runs through woq_probe_attn_decode_plan.
#include <algorithm>

#include "woq_attn_decode.h"
#include "woq_attn_merge.h"
#include "woq_device.h"
#include "woq_gemv_launch.h"
#include "woq_host.h"
#include "woq_kv_codec.h"
#include "woq_xq.h"
#include "../../include/woq_hip_experimental.h"

namespace woq {

// ---- one workgroup per (query head, context slice): the body of woq_attn_decode.h on an earlier launch's fp32 q / k / v
template <typename KV, int HD, bool SPLIT>
__global__ __launch_bounds__(256) void attn_decode_kernel(const float* __restrict__ qkv, KV* __restrict__ kcache,
                                                          KV* __restrict__ vcache, const int32_t* __restrict__ pos_p,
                                                          const float* __restrict__ cs, const float* __restrict__ sn,
                                                          int hk, int window, int spw,
                                                          float* __restrict__ out, XqPtrs xo, AttnMerge mg) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  // hk = heads | kv_heads << 16: with `window` the 13th and 14th argument dwords — everything in front of the first
  // K / V request is preloaded (the argument segment's first read costs ~1 us, profiles/r06c_xqs_stage_stamps.txt)
  const int heads = hk & 0xffff, kv_heads = hk >> 16;
  // workgroup ids go round-robin over the 8 XCDs: give every XCD a run of consecutive heads, so that the query heads
  // sharing a kv head (GQA) share an L2 instead of pulling the same cache rows into several
  const int bx = (int)blockIdx.x;
  const int h = (heads & 7) == 0 ? (bx & 7) * (heads >> 3) + (bx >> 3) : bx;
  attn_decode_body<KV, HD, SPLIT>(sm, h, (int)blockIdx.y, (int)gridDim.y, AttnPlain{qkv}, kcache, vcache, pos_p, cs,
                                  sn, heads, kv_heads, window, spw, out, xo);
  if constexpr (SPLIT) {  // `out` = the partial buffer; the head's last slice workgroup merges (woq_attn_merge.h)
    if (mg.counter != nullptr) attn_slices_merge<HD, 1>(out, heads, h, 1, (int)gridDim.y, mg.counter + h, mg, sm);
  }
}

// the same launch with the per-head q / k RMSNorm in front of the rotation (woq_attn_decode.h QKN): a kernel of its own,
// so that the one above keeps its arguments and its code
template <typename KV, int HD, bool SPLIT>
__global__ __launch_bounds__(256) void attn_decode_qkn_kernel(const float* __restrict__ qkv, KV* __restrict__ kcache,
                                                              KV* __restrict__ vcache, const int32_t* __restrict__ pos_p,
                                                              const float* __restrict__ cs, const float* __restrict__ sn,
                                                              int hk, int window, int spw, float* __restrict__ out,
                                                              XqPtrs xo, AttnMerge mg, AttnQkNorm qn) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int heads = hk & 0xffff, kv_heads = hk >> 16;
  const int bx = (int)blockIdx.x;
  const int h = (heads & 7) == 0 ? (bx & 7) * (heads >> 3) + (bx >> 3) : bx;
  attn_decode_body<KV, HD, SPLIT, AttnPlain, true>(sm, h, (int)blockIdx.y, (int)gridDim.y, AttnPlain{qkv}, kcache, vcache,
                                                   pos_p, cs, sn, heads, kv_heads, window, spw, out, xo,
                                                   XqPub{nullptr, 0u}, qn);
  if constexpr (SPLIT) {
    if (mg.counter != nullptr) attn_slices_merge<HD, 1>(out, heads, h, 1, (int)gridDim.y, mg.counter + h, mg, sm);
  }
}

// merge the slices of attn_decode_kernel<SPLIT>: out[h][d] = sum_s o_s[d] e^(m_s - m) / sum_s l_s e^(m_s - m).
// 256 threads per head; two thread groups of HD walk alternate slices. Round 4: ONE round trip — a thread's partial
// rows (clamped, branch-free; rows past ns weigh 0) are requested together with the slice maxima / sums, before anything
// is waited for; the weights are then worked out in LDS while the rows are in flight (round 3 read the maxima, then
// the rows: two dependent trips in a launch that is nothing but latency, 5.1 us per layer at 32 slices).
template <int HD>
__global__ __launch_bounds__(256) void attn_combine_kernel(const float* __restrict__ part, int ns,
                                                          float* __restrict__ out, XqPtrs xo) {
  __shared__ float ms[64], wl[64], wsc[64], red[256];
  constexpr int GROUPS = 256 / HD;                // 2 for head_dim 128, 4 for 64
  constexpr int PER = ATTN_MAX_SLICES / GROUPS;   // partial rows a thread may have to fetch
  const int h = blockIdx.x, tid = threadIdx.x;
  const int d = tid % HD, grp = tid / HD;
  const float* p = part + (size_t)h * ATTN_MAX_SLICES * HD;  // woq_attn_merge.h: o [head][64][HD], then ml [head][64][2]
  const float* pml = part + (size_t)gridDim.x * ATTN_MAX_SLICES * HD + (size_t)h * ATTN_MAX_SLICES * 2;
  const int si = min(tid, ns - 1);
  const float m_r = pml[si * 2], l_r = pml[si * 2 + 1];
  float v[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) v[u] = p[(size_t)min(grp + u * GROUPS, ns - 1) * HD + d];
  if (tid < ns) ms[tid] = m_r, wl[tid] = l_r;
  __syncthreads();
  float m = -INFINITY;
  for (int s = 0; s < ns; ++s) m = fmaxf(m, ms[s]);
  if (tid < ns) {
    const float w = ms[tid] == -INFINITY ? 0.f : __expf(ms[tid] - m);
    wsc[tid] = w;
    wl[tid] *= w;
  }
  __syncthreads();
  float l = 0.f;
  for (int s = 0; s < ns; ++s) l += wl[s];
  float o = 0.f;
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int s = grp + u * GROUPS;
    if (s < ns) o = fmaf(v[u], wsc[s], o);  // ascending s
  }
  red[tid] = o;
  __syncthreads();
  if (grp == 0) {
    float t = 0.f;
#pragma unroll
    for (int g2 = 0; g2 < GROUPS; ++g2) t += red[g2 * HD + d];
    out[(size_t)h * HD + d] = t / l;
    if (xo.limbs != nullptr) xq_emit16(t / l, xo, (h * HD + d) >> 4, d & 15);
  }
}

// ---- long-context decode attention for grouped-query models, on the matrix cores -----------------------------------
// One workgroup per (kv head, context slice): the REP query heads that share the kv head are the 16 columns of
// S^T = K Q^T (REP <= 16 live), so every K / V row of the slice leaves HBM / L2 ONCE for all of them — the
// per-query-head sliced kernel above pulls the same rows through the CUs' load paths REP times.
// The four waves are independent streams: wave w owns the 32-position sub-tiles w, w + 4, ... of the slice with its
// own online-softmax state, no workgroup barrier inside the loop, one merge through LDS at the end:
//  * K fragments come STRAIGHT from the cache into MFMA operand registers: the contraction runs over d, and any
//    assignment of d to (MFMA, lane quarter, element) is legal as long as Q uses the same one — lane quarter kq takes
//    d = 32 kq + 8 c + e for MFMA c, i.e. 32 contiguous elements of its row;
//  * q is split into fp16 hi + lo (two MFMAs per fragment): the scores carry fp32-class accuracy, the bar the
//    decode parity tests hold (K / V of an fp8 or fp16 cache are exact in fp16);
//  * V goes through a wave-private transposed LDS tile ([d][32 positions], the 4 x 8 register transpose of
//    attn_prefill_kernel) because positions are the contraction index of O^T = V^T P^T; the probabilities are the
//    S^T accumulators repacked in place (positions {4 kq + j, 16 + 4 kq + j} per lane on both operands);
//  * the next sub-tile's loads are in flight while the current one is in the MFMAs.
// The new token's k / v are applied from LDS by wave 0 of the last slice (rounded to the cache dtype like the rows a
// later step reads back) and appended there. Output: un-normalised partials (o[HD], max, sum) per (head, slice) in the
// natural-exp convention attn_combine_kernel merges.
// One register set of the kernel below: a 32-position sub-tile's K fragments (lane: rows a * 16 + i16, 32 contiguous d)
// and V rows (lane: rows 4 v_g + r, 16 contiguous d). fp16 caches hold them as loaded; an fp8 cache keeps the RAW bytes —
// half the registers, 16-byte requests instead of 8-byte ones — and converts a fragment right where it enters an
// MFMA / the LDS transpose (round 4: 272 -> under 256 registers puts two workgroups on a CU instead of one).
template <int KVD>
struct DecRegs {
  h8 kf[2][4], vr[4][2];
  __device__ __forceinline__ void load_k(int a, const void* kc, size_t row) {
#pragma unroll
    for (int c = 0; c < 4; ++c) kf[a][c] = kv_load8<KVD>(kc, row + c * 8);
  }
  __device__ __forceinline__ void load_v(int r, const void* vc, size_t row) {
    vr[r][0] = kv_load8<KVD>(vc, row);
    vr[r][1] = kv_load8<KVD>(vc, row + 8);
  }
  __device__ __forceinline__ h8 k(int a, int c) const { return kf[a][c]; }
  __device__ __forceinline__ h8 v(int r, int hh) const { return vr[r][hh]; }
};
template <>
struct DecRegs<WOQ_FP8_E4M3> {
  u32x4 kf[2][2], vr[4];
  __device__ __forceinline__ void load_k(int a, const void* kc, size_t row) {
    kf[a][0] = *(const u32x4*)((const uint8_t*)kc + row);
    kf[a][1] = *(const u32x4*)((const uint8_t*)kc + row + 16);
  }
  __device__ __forceinline__ void load_v(int r, const void* vc, size_t row) {
    vr[r] = *(const u32x4*)((const uint8_t*)vc + row);
  }
  __device__ __forceinline__ h8 k(int a, int c) const {
    const u32x4& w = kf[a][c >> 1];
    return fp8x8_to_h8((c & 1) ? (u32x2){w.z, w.w} : (u32x2){w.x, w.y});
  }
  __device__ __forceinline__ h8 v(int r, int hh) const {
    const u32x4& w = vr[r];
    return fp8x8_to_h8(hh ? (u32x2){w.z, w.w} : (u32x2){w.x, w.y});
  }
};

constexpr int DST = 32;   // positions per sub-tile
constexpr int DVRB = 80;  // bytes per V^T row: 32 positions x 2 B + 16 pad
constexpr int attn_dec_lds_bytes(int HD, int REP) { return 4 * HD * DVRB + 2 * HD * 4 + REP * HD * 4; }

template <int KVD, int HD, int REP>
__global__ __launch_bounds__(256) void attn_decode_mfma_kernel(const float* __restrict__ qkv, void* __restrict__ kcache,
                                                               void* __restrict__ vcache,
                                                               const int32_t* __restrict__ pos_p,
                                                               const float* __restrict__ cs,
                                                               const float* __restrict__ sn, int hkc, int window,
                                                               float* __restrict__ part, int max_rows, AttnMerge mg) {
  // hkc = heads | kv_heads << 8 | (chunk_fixed / 32) << 16: with `window` the 13th and 14th argument dwords, so that
  // everything in front of the first K / V request is PRELOADED — a kernel's first read of its argument segment costs
  // ~1 us inside a replayed graph (profiles/r06c_xqs_stage_stamps.txt), and heads / kv_heads / window / chunk_fixed
  // used to sit behind the 14 preloaded dwords
  const int heads = hkc & 0xff, kv_heads = (hkc >> 8) & 0xff, chunk_fixed = ((hkc >> 16) & 0xffff) * 32;
  static_assert(HD == 128 && REP <= 16, "one 16-column MFMA tile of query heads, head_dim 128");
  static_assert(16 * (HD + 2) * 4 <= HD * DVRB, "the merge record of a wave reuses its V^T tile");
  constexpr int DC = HD / 32, DT = HD / 16, half = HD / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char* vw = dsm_raw + wid * (HD * DVRB);    // this wave's V^T tile, later its merge record
  float* kn = (float*)(dsm_raw + 4 * HD * DVRB);      // [HD] new k (rotated, as the cache holds it), [HD] new v
  float* vn = kn + HD;
  float* qs = vn + HD;                                // [REP][HD] rotated query heads
  const int i16 = lane & 15, kq = lane >> 4;
  const int kh = blockIdx.x, ns = (int)gridDim.y, sp = (int)blockIdx.y;
  // Two slice geometries. ADAPTIVE (chunk_fixed == 0, or a sliding window): the cached span is cut into ns even
  // chunks — every address then depends on the position, which is a device-side word: one dependent round trip before
  // the first K / V byte can be asked for. FIXED (round 4): slice sp owns absolute positions [sp * chunk_fixed,
  // (sp + 1) * chunk_fixed) whatever the position is (the last slice also takes whatever lies beyond), so the two
  // sub-tiles every wave starts with are requested BEFORE the position is read; rows at or beyond it hold zeros or
  // older finite values (the cache is zero-filled at creation) and are masked like ragged tails. Slices that lie
  // wholly beyond the position publish an empty partial.
  const bool fixed = chunk_fixed > 0 && window == 0;
  const size_t cache_row = (size_t)kv_heads * HD;
  const int v_g = lane >> 3, v_c = lane & 7;  // V staging: positions 4 v_g .. + 4, d = 16 v_c .. + 16
  size_t cache0 = (size_t)(fixed ? sp * chunk_fixed : 0) * cache_row + (size_t)kh * HD;
  int last = fixed ? max(0, min(chunk_fixed, max_rows - sp * chunk_fixed) - 1) : 0;
  // two register sets: a wave's first two sub-tiles are requested back to back, then set X is refilled for
  // sub-tile n + 8 as soon as sub-tile n has left it (one exposed load latency per wave, not one per sub-tile)
  DecRegs<KVD> setA, setB;
  auto fetch = [&](DecRegs<KVD>& rs, int sub) {
    const int t0 = sub * DST;
#pragma unroll
    for (int a = 0; a < 2; ++a)
      rs.load_k(a, kcache, cache0 + (size_t)min(t0 + a * 16 + i16, last) * cache_row + kq * 32);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      rs.load_v(r, vcache, cache0 + (size_t)min(t0 + v_g * 4 + r, last) * cache_row + v_c * 16);
  };
  const bool early = fixed && sp * chunk_fixed < max_rows;
  if (early) {
    if (wid * DST <= last) fetch(setA, wid);
    if ((wid + 4) * DST <= last) fetch(setB, wid + 4);
  }
  const int apos = pos_p[0];
  const int w_lo = window > 0 ? max(0, apos + 1 - window) : 0;
  const int span = apos - w_lo;
  int t_lo, npos;
  bool incl_new;
  if (fixed) {
    t_lo = sp * chunk_fixed;
    npos = sp == ns - 1 ? max(apos - t_lo, 0) : max(0, min(apos - t_lo, chunk_fixed));
    incl_new = sp == min(apos / chunk_fixed, ns - 1);
  } else {
    const int chunk = (((span + ns - 1) / ns) + 4 * DST - 1) & ~(4 * DST - 1);
    t_lo = w_lo + min(sp * chunk, span);
    npos = min(apos - t_lo, chunk);  // cached positions of this slice
    incl_new = sp == ns - 1;
    cache0 = (size_t)t_lo * cache_row + (size_t)kh * HD;
  }
  const int n_sub = (npos + DST - 1) / DST;
  const int last_early = last;
  last = max(npos - 1, 0);
  const float sc = 1.44269504088896f / sqrtf((float)HD);

  // prologue, request phase (round 4): the new token's q / k / v and its cos / sin rows are asked for BEFORE the K / V
  // sub-tiles of the adaptive geometry — returns come back in order, so behind 16 KB of cache rows per wave the rotation
  // cannot start until the whole first burst has landed. (Measured neutral: 9.49 vs 9.41 us per layer at 8k,
  // profiles/r04j_*; kept because it is never worse.)
  constexpr int QIT = (REP * HD + 255) / 256;
  static_assert(256 % HD == 0, "a thread keeps its d across the query heads it rotates");
  float q_a[QIT], q_b[QIT];
  const float q_co = cs[(size_t)apos * half + (tid & (half - 1))], q_si = sn[(size_t)apos * half + (tid & (half - 1))];
#pragma unroll
  for (int it = 0; it < QIT; ++it) {
    const int idx = min(tid + it * 256, REP * HD - 1);
    const int d = idx & (HD - 1);
    const float* q = qkv + (size_t)kh * REP * HD + (idx - d);
    q_a[it] = q[d], q_b[it] = q[d ^ half];
  }
  float k_a[8], k_b[8], k_co[8], k_si[8], v_in[8];
  if (tid < HD / 8) {
    const float* k = qkv + (size_t)(heads + kh) * HD;
    const float* v = qkv + (size_t)(heads + kv_heads + kh) * HD;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = tid * 8 + j, i = d & (half - 1);
      k_co[j] = cs[(size_t)apos * half + i], k_si[j] = sn[(size_t)apos * half + i];
      k_a[j] = k[d], k_b[j] = k[d ^ half];
      v_in[j] = v[d];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // what the early requests did not cover: everything in the adaptive geometry; in the fixed one the sub-tiles past
  // the slice's own chunk (short chunks, or the last slice's overflow)
  if (wid < n_sub && !(early && wid * DST <= last_early)) fetch(setA, wid);
  if (wid + 4 < n_sub && !(early && (wid + 4) * DST <= last_early)) fetch(setB, wid + 4);

  // prologue through LDS: threads 0..15 build the new k / v of this kv head (rotated, rounded through the cache dtype
  // like the rows a later step reads back; the slice that holds the new position appends them), everyone rotates the REP
  // query heads
  if (tid < HD / 8) {
    float kk[8], vv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = tid * 8 + j;
      kk[j] = d < half ? k_a[j] * k_co[j] - k_b[j] * k_si[j] : k_a[j] * k_co[j] + k_b[j] * k_si[j];
      vv[j] = v_in[j];
    }
    alignas(16) unsigned char tmp[32];
    kv_store8<KVD>(tmp, 0, kk);
    const h8 kr = kv_load8<KVD>(tmp, 0);
    kv_store8<KVD>(tmp, 0, vv);
    const h8 vr8 = kv_load8<KVD>(tmp, 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) kn[tid * 8 + j] = (float)kr[j], vn[tid * 8 + j] = (float)vr8[j];
    if (incl_new) {
      const size_t e = (size_t)apos * cache_row + (size_t)kh * HD + tid * 8;
      kv_store8<KVD>(kcache, e, kk);
      kv_store8<KVD>(vcache, e, vv);
    }
  }
#pragma unroll
  for (int it = 0; it < QIT; ++it) {
    const int idx = tid + it * 256;
    if (idx < REP * HD) {
      const int d = idx & (HD - 1);
      qs[idx] = d < half ? q_a[it] * q_co - q_b[it] * q_si : q_a[it] * q_co + q_b[it] * q_si;
    }
  }
  __syncthreads();
  // Q^T fragments, fp16 hi + lo: lane (head i16, quarter kq) holds d = 32 kq + 8 c + e
  h8 qh[DC], ql[DC];
#pragma unroll
  for (int c = 0; c < DC; ++c) {
    float qv[8];
    if (i16 < REP) {
      const float* src = qs + i16 * HD + kq * 32 + c * 8;
      *(float4_t*)&qv[0] = *(const float4_t*)src;
      *(float4_t*)&qv[4] = *(const float4_t*)(src + 4);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) qv[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const _Float16 hi = (_Float16)qv[e];
      qh[c][e] = hi;
      ql[c][e] = (_Float16)(qv[e] - (float)hi);
    }
  }
  float4_t o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = (float4_t){0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_part = 0.f;

  auto process = [&](DecRegs<KVD>& rs, int sub) {
    // this sub-tile: V^T into LDS, K fragments into the score MFMAs; then the refill of the register set
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const h8 v0 = rs.v(0, hh), v1 = rs.v(1, hh), v2 = rs.v(2, hh), v3 = rs.v(3, hh);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int d = v_c * 16 + hh * 8 + i;
        const h4 col = {v0[i], v1[i], v2[i], v3[i]};
        *(h4*)(vw + d * DVRB + ((v_g ^ v_c) << 3)) = col;
      }
    }
    float4_t s[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      s[a] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < DC; ++c) {
        const h8 kf = rs.k(a, c);
        s[a] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, ql[c], s[a], 0, 0, 0);
        s[a] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qh[c], s[a], 0, 0, 0);
      }
    }
    const int t0 = sub * DST;
    __builtin_amdgcn_sched_barrier(0);  // the loads below reuse the registers the stores / MFMAs above just released
    if (sub + 8 < n_sub) fetch(rs, sub + 8);
    float mx = -INFINITY;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (t0 + a * 16 + kq * 4 + j >= npos) s[a][j] = -INFINITY;
        mx = fmaxf(mx, s[a][j]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx * sc);  // finite: position t0 of a processed sub-tile is always live
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    float ps = 0.f;
    h8 pb;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = __builtin_amdgcn_exp2f(fmaf(s[a][j], sc, -m_new));
        ps += p;
        pb[a * 4 + j] = (_Float16)p;
      }
    l_part = fmaf(l_part, alpha, ps);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const unsigned char* vrow = vw + (dt * 16 + i16) * DVRB;
      const u32x2 lo = *(const u32x2*)(vrow + ((kq ^ dt) << 3));
      const u32x2 hi = *(const u32x2*)(vrow + (((4 + kq) ^ dt) << 3));
      const h8 vf = __builtin_bit_cast(h8, (u32x4){lo.x, lo.y, hi.x, hi.y});
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb, o[dt] * alpha, 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
  };
  for (int sub = wid; sub < n_sub; sub += 8) {
    process(setA, sub);
    if (sub + 4 < n_sub) process(setB, sub + 4);
  }
  if (wid == 0 && incl_new) {  // the new position: score from the fragments, value row from LDS
    float d = 0.f;
    const float* qrow = qs + min(i16, REP - 1) * HD + kq * 32;
#pragma unroll 8
    for (int e = 0; e < 32; ++e) d = fmaf(qrow[e], kn[kq * 32 + e], d);
    d += __shfl_xor(d, 16, 64);
    d += __shfl_xor(d, 32, 64);
    const float m_new = fmaxf(m_run, d * sc);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    const float p = __builtin_amdgcn_exp2f(fmaf(d, sc, -m_new));
    m_run = m_new;
    l_part = fmaf(l_part, alpha, kq == 0 ? p : 0.f);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int j = 0; j < 4; ++j) o[dt][j] = fmaf(o[dt][j], alpha, p * vn[dt * 16 + kq * 4 + j]);
  }
  // merge the four waves: record = o[16 heads][HD], max[16], sum[16] (fp32) in the wave's own V^T tile
  float l = l_part;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  {
    float* rec = (float*)vw;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *(float4_t*)(rec + i16 * HD + dt * 16 + kq * 4) = o[dt];
    if (kq == 0) {
      rec[16 * HD + i16] = m_run;
      rec[16 * HD + 16 + i16] = l;
    }
  }
  __syncthreads();
  {
    const int d = tid & (HD - 1);
    for (int h = tid / HD; h < REP; h += 256 / HD) {
      float mw[4], m = -INFINITY;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        mw[w] = ((const float*)(dsm_raw + w * (HD * DVRB)))[16 * HD + h];
        m = fmaxf(m, mw[w]);
      }
      float acc = 0.f, den = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float* rec = (const float*)(dsm_raw + w * (HD * DVRB));
        const float wt = mw[w] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw[w] - m);
        acc = fmaf(rec[h * HD + d], wt, acc);
        den = fmaf(rec[16 * HD + 16 + h], wt, den);
      }
      const float m_nat = m == -INFINITY ? -INFINITY : m * 0.6931471805599453f;  // exp2 domain -> natural
      if (mg.part_g != nullptr) {  // all-to-all merge (round 6): tagged granules, finalised below by the slices themselves
        const AttnA2A a2a{mg.part_g, (mg.seq[0] << 6) | (unsigned int)mg.layer, mg.status};
        attn_a2a_publish(a2a, kh * REP + h, sp, HD, d, acc);
        if (d == 0) {
          attn_a2a_publish(a2a, kh * REP + h, sp, HD, HD, m_nat);
          attn_a2a_publish(a2a, kh * REP + h, sp, HD, HD + 1, den);
        }
        continue;
      }
      // publish (woq_attn_merge.h: agent-scope write-through stores; the merging workgroup may sit on another XCD)
      st_agent(attn_part_o(part, kh * REP + h, sp, HD) + d, acc);
      if (d == 0) {
        float* ml = attn_part_ml(part, heads, kh * REP + h, sp, HD);
        st_agent(ml, m_nat);
        st_agent(ml + 1, den);
      }
    }
  }
  if (mg.part_g != nullptr) {
    // the group's REP * 8 output blocks go round the slices: block B = sp + R * ns is DPP row R's — 16 rows per workgroup
    // and pass, as many passes as REP * 8 / ns needs (REP = 8 in two slices: two)
    constexpr int NB = REP * (HD / 16);
    const AttnA2A a2a{mg.part_g, (mg.seq[0] << 6) | (unsigned int)mg.layer, mg.status};
    for (int R0 = 0; sp + R0 * ns < NB; R0 += 16) {
      if (sp + (R0 + wid * 4) * ns >= NB) continue;  // (wave-uniform: no row of this wave has a block in this pass)
      const int B = sp + (R0 + wid * 4 + (lane >> 4)) * ns;
      const int Bc = min(B, NB - 1);
      attn_a2a_finalize<HD, 32>(a2a, kh * REP + Bc / (HD / 16), Bc % (HD / 16), ns, B < NB, [&](float v, int idx) {
        mg.out[idx] = v;
        if (mg.xo.limbs != nullptr) xq_emit16(v, mg.xo, idx >> 4, idx & 15);
      });
    }
    return;
  }
  // the last slice workgroup of this kv head to get here merges the group's REP heads and emits the attention output
  if (mg.counter != nullptr) attn_slices_merge<HD, (REP < 2 ? REP : 2)>(part, heads, kh * REP, REP, ns, mg.counter + kh, mg, (float*)dsm_raw);
}

// ---- the plan ------------------------------------------------------------------------------------------------------
// the six instances of the grouped kernel, written once: the launch, the occupancy query and the plan's "does the
// grouped form cover this shape" all read this table (null = not covered)
using AttnMfmaKernel = void (*)(const float*, void*, void*, const int32_t*, const float*, const float*, int, int, float*,
                                int, AttnMerge);
static AttnMfmaKernel attn_mfma_kernel_for(int kv_dtype, int rep) {
#define WOQ_DEC_CASE(KVD, R) \
  if (kv_dtype == KVD && rep == R) return attn_decode_mfma_kernel<KVD, 128, R>;
  WOQ_DEC_CASE(WOQ_F16, 2) WOQ_DEC_CASE(WOQ_F16, 4) WOQ_DEC_CASE(WOQ_F16, 8)
  WOQ_DEC_CASE(WOQ_FP8_E4M3, 2) WOQ_DEC_CASE(WOQ_FP8_E4M3, 4) WOQ_DEC_CASE(WOQ_FP8_E4M3, 8)
#undef WOQ_DEC_CASE
  return nullptr;
}

// positions one per-head attention workgroup may hold scores for: all a query can see, or its slice (in 64s) + 64
static int attn_dec_span(int max_ctx, int window, int slices) {
  const int reach = window > 0 ? std::min(window, max_ctx) : max_ctx;
  return slices > 1 ? ((((reach + slices - 1) / slices) + 63) & ~63) + 64 : reach;
}

// Does the fused qkv + attention launch take this (blob, attention) combination at `slices` slices?
static bool fused_attn_covers(const woq_blob_header& h, const AttnShape& s, int slices) {
  if (h.weight_type != WOQ_W_INT4_CLIP || h.off_shuffle != 0 || h.K != h.Kpad || h.N != h.Npad) return false;
  if (h.Kpad / WOQ_TILE_K != 4 * FUSED_TPW) return false;  // four waves of eight tiles
  BlobView v;
  if (!blob_view(nullptr, h, v)) return false;
  // (grouped-query shapes and a sliding window are taken as well: kh = h / rep, re-based cache pointers)
  if (s.kv_heads < 1 || s.heads % s.kv_heads != 0 || s.head_dim != 128 || slices > ATTN_A2A_MAX_SLICES) return false;
  if (slices > 1 && s.heads * slices > 512) return false;  // the slices of a head wait for each other: resident together
  if (slices > 1 && (s.heads + 2 * s.kv_heads) * 8 + s.heads * slices > 65535) return false;  // the packed strip count
  if (h.N != (s.heads + 2 * s.kv_heads) * s.head_dim) return false;
  if (s.kv_dtype != WOQ_F16 && s.kv_dtype != WOQ_BF16 && s.kv_dtype != WOQ_FP8_E4M3) return false;
  // every workgroup of the launch gets max(attention LDS, GEMV LDS): the strips inherit the attention's score buffer,
  // which grows with max_ctx. Up to 38 KiB (max_ctx 8192) four workgroups still share a CU's 160 KiB; beyond that the
  // strips would lose occupancy to a buffer they never touch, so such engines keep the two launches.
  return attn_dec_lds_floats(128, attn_dec_span(s.max_ctx, s.window, slices)) * 4 <= 38 * 1024;
}

AttnDecodePlan plan_attn_decode(const AttnShape& s, const AttnOptions& o, const AttnFacts& f) {
  AttnDecodePlan p = {};
  p.shape = s;
  p.slices = o.splits > 1 ? o.splits : 1;
  p.merge = ATTN_MERGE_NONE;
  const bool tags_ok = f.layers <= 64;  // beyond 64 layers the layer bits of a hand-off tag would run into the counter
  // FUSED: the XQ step only; a request for the grouped form keeps the separate launches even where that form does not
  // apply; sliced, it needs the partial granules and no arrival counters (its slices merge among themselves)
  if (f.xq && o.fuse_attn && f.granules && f.qkv_hdr != nullptr && !o.grouped && tags_ok &&
      !(p.slices > 1 && (!o.fuse_sliced || o.fold)) && fused_attn_covers(*f.qkv_hdr, s, p.slices)) {
    p.form = ATTN_FUSED;
    if (p.slices > 1) p.merge = ATTN_MERGE_A2A;
    p.span = attn_dec_span(s.max_ctx, s.window, p.slices);
    p.spw = attn_dec_spw(p.span);
    p.lds = attn_dec_lds_floats(128, p.span) * 4;
    p.grid_x = (unsigned)(f.qkv_hdr->N / 16 + s.heads * p.slices), p.grid_y = 1;  // strips, then attention workgroups
    p.launches = 1;
    return p;
  }
  p.form = ATTN_PER_HEAD;
  p.launches = 2;
  if (s.head_dim != 64 && s.head_dim != 128) return p.error = "QBits: attention head_dim must be 64 or 128", p;
  if (o.splits > ATTN_MAX_SLICES) return p.error = "QBits: at most 64 context slices", p;
  if (p.slices > 1) p.merge = o.fold ? ATTN_MERGE_COUNTER : ATTN_MERGE_COMBINE;
  // GROUPED: only where it applies — sliced, head_dim 128, 2 / 4 / 8 query heads per kv head, an fp16 or fp8 cache,
  // counts that fit the packed argument dword — anything else keeps the per-query-head kernels
  const int rep = s.kv_heads > 0 ? s.heads / s.kv_heads : 0;
  // (a layer with a q / k norm: the grouped kernel does not carry it — such layers keep the per-query-head kernels)
  if (o.grouped && !f.qk_norm && s.head_dim == 128 && p.slices > 1 && s.heads <= 255 && s.kv_heads <= 255 &&
      o.chunk_fixed / 32 <= 65535 && attn_mfma_kernel_for(s.kv_dtype, rep) != nullptr) {
    p.form = ATTN_GROUPED;
    p.chunk_fixed = o.chunk_fixed % DST != 0 ? 0 : o.chunk_fixed;
    // the slices merge among themselves where every workgroup of the grid is resident at once (they wait for each
    // other); the arrival counters win over it
    if (f.xq && o.grouped_a2a && !o.fold && f.granules && tags_ok && p.slices <= 32 && s.kv_heads * p.slices <= f.slots)
      p.merge = ATTN_MERGE_A2A;
    p.lds = (size_t)attn_dec_lds_bytes(128, rep);
    p.grid_x = (unsigned)s.kv_heads, p.grid_y = (unsigned)p.slices;
  } else {
    p.span = attn_dec_span(s.max_ctx, s.window, p.slices);
    p.spw = attn_dec_spw(p.span);
    p.lds = attn_dec_lds_floats(s.head_dim, p.span) * 4;
    if (p.lds > 160 * 1024) return p.error = "QBits: max_ctx too large for the decode attention (raise attn_splits)", p;
    p.grid_x = (unsigned)s.heads, p.grid_y = (unsigned)p.slices;
  }
  if (p.merge == ATTN_MERGE_COMBINE) p.launches = 3;
  return p;
}

// ---- the launchers -------------------------------------------------------------------------------------------------
template <typename KV, int HD, bool SPLIT>
static int launch_attn_per_head(const AttnDecodePlan& p, const AttnDecodeIO& io, hipStream_t st) {
  constexpr auto k = attn_decode_kernel<KV, HD, SPLIT>;
  if (const int rc = allow_dynamic_lds<k>(160 * 1024)) return rc;
  const XqPtrs no_xq{nullptr, nullptr, nullptr};
  // sliced: the kernel writes partials, and the merge (its last workgroups, or the combine launch) the output and its XQ form
  const AttnMerge mg = SPLIT ? AttnMerge{p.merge == ATTN_MERGE_COUNTER ? io.counters : nullptr, io.out, io.xo}
                             : AttnMerge{nullptr, nullptr, no_xq};
  if (io.q_norm != nullptr) {
    constexpr auto kn = attn_decode_qkn_kernel<KV, HD, SPLIT>;
    if (const int rc = allow_dynamic_lds<kn>(160 * 1024)) return rc;
    hipLaunchKernelGGL(kn, dim3(p.grid_x, p.grid_y), dim3(256), p.lds, st, io.qkv, (KV*)io.kcache, (KV*)io.vcache, io.pos,
                       io.cs, io.sn, p.shape.heads | (p.shape.kv_heads << 16), p.shape.window, p.spw,
                       SPLIT ? io.part : io.out, SPLIT ? no_xq : io.xo, mg, AttnQkNorm{io.q_norm, io.k_norm, io.qk_eps});
    return 0;
  }
  hipLaunchKernelGGL(k, dim3(p.grid_x, p.grid_y), dim3(256), p.lds, st, io.qkv, (KV*)io.kcache, (KV*)io.vcache, io.pos,
                     io.cs, io.sn, p.shape.heads | (p.shape.kv_heads << 16), p.shape.window, p.spw,
                     SPLIT ? io.part : io.out, SPLIT ? no_xq : io.xo, mg);
  return 0;
}
template <typename KV>
static int launch_attn_per_head_kv(const AttnDecodePlan& p, const AttnDecodeIO& io, hipStream_t st) {
  if (p.shape.head_dim == 128)
    return p.slices > 1 ? launch_attn_per_head<KV, 128, true>(p, io, st) : launch_attn_per_head<KV, 128, false>(p, io, st);
  return p.slices > 1 ? launch_attn_per_head<KV, 64, true>(p, io, st) : launch_attn_per_head<KV, 64, false>(p, io, st);
}

int launch_attn_decode(const AttnDecodePlan& p, const AttnDecodeIO& io, hipStream_t st) {
  if (p.error != nullptr) return woq::fail(p.error);
  if (p.form == ATTN_FUSED) return woq::fail("QBits: a fused attention plan runs inside the qkv launch");
  const AttnShape& s = p.shape;
  if ((io.q_norm != nullptr) != (io.k_norm != nullptr)) return woq::fail("QBits: q_norm and k_norm come together");
  if (io.q_norm != nullptr && p.form == ATTN_GROUPED)
    return woq::fail("QBits: the grouped decode attention does not carry a q / k norm");
  if (p.form == ATTN_GROUPED) {
    AttnMerge mg{p.merge == ATTN_MERGE_COUNTER ? io.counters : nullptr, io.out, io.xo};
    if (p.merge == ATTN_MERGE_A2A) mg.part_g = io.part_g, mg.seq = io.seq, mg.layer = io.layer, mg.status = io.status;
    const AttnMfmaKernel k = attn_mfma_kernel_for(s.kv_dtype, s.heads / s.kv_heads);
    hipLaunchKernelGGL(k, dim3(p.grid_x, p.grid_y), dim3(256), p.lds, st, io.qkv, io.kcache, io.vcache, io.pos, io.cs, io.sn,
                       s.heads | (s.kv_heads << 8) | ((p.chunk_fixed / 32) << 16), s.window, io.part, s.max_ctx, mg);
  } else {
    const int rc = s.kv_dtype == WOQ_F16        ? launch_attn_per_head_kv<_Float16>(p, io, st)
                   : s.kv_dtype == WOQ_FP8_E4M3 ? launch_attn_per_head_kv<Fp8>(p, io, st)
                                                : launch_attn_per_head_kv<__bf16>(p, io, st);  // (any other cache type)
    if (rc) return rc;
  }
  if (p.merge == ATTN_MERGE_COMBINE) {
    const auto k = s.head_dim == 128 ? attn_combine_kernel<128> : attn_combine_kernel<64>;
    hipLaunchKernelGGL(k, dim3(s.heads), dim3(256), 0, st, io.part, p.slices, io.out, io.xo);
  }
  return 0;
}

int attn_decode_mfma_slots(int kv_dtype, int rep) {
  static int cache[2][9] = {};  // [fp16 | fp8][rep], 0 = not asked yet, -1 = not covered
  const int ci = kv_dtype == WOQ_FP8_E4M3 ? 1 : 0;
  if ((kv_dtype != WOQ_F16 && kv_dtype != WOQ_FP8_E4M3) || rep < 0 || rep > 8) return 0;
  if (cache[ci][rep] != 0) return std::max(cache[ci][rep], 0);
  cache[ci][rep] = -1;
  int per_cu = 0;
  if (const AttnMfmaKernel k = attn_mfma_kernel_for(kv_dtype, rep))
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 256, attn_dec_lds_bytes(128, rep)) != hipSuccess)
      per_cu = 0;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  if (per_cu * cus > 0) cache[ci][rep] = per_cu * cus;
  return per_cu * cus;
}

void attn_plan_report(const AttnDecodePlan& p, long long* out11) {
  const long long v[11] = {p.form, p.merge, p.slices, p.chunk_fixed, p.span, p.spw, (long long)p.lds,
                           p.grid_x, p.grid_y, p.launches, p.error != nullptr};
  std::copy(v, v + 11, out11);
  if (p.error != nullptr) woq::fail(p.error);
}

}  // namespace woq

using namespace woq;

extern "C" {

// test entry point (include/woq_hip_experimental.h): the plan for given inputs, host only
WOQ_API int woq_probe_attn_decode_plan(const int* in23, long long* out11) {
  WOQ_TRY
  WOQ_CHECK(in23 != nullptr && out11 != nullptr, "QBits: bad argument");
  const int* a = in23;
  const AttnShape s{a[0], a[1], a[2], a[3], a[4], a[5]};
  WOQ_CHECK(s.heads > 0 && s.kv_heads > 0 && s.heads % s.kv_heads == 0 && s.max_ctx > 0 && s.window >= 0 && a[6] >= 1 &&
                a[9] >= 0,
            "QBits: bad attention shape");
  AttnOptions o;
  o.splits = a[6], o.grouped = a[7] != 0, o.fold = a[8] != 0, o.chunk_fixed = a[9];
  o.fuse_attn = a[10] != 0, o.fuse_sliced = a[11] != 0, o.grouped_a2a = a[12] != 0;
  woq_blob_header h;
  const bool has_hdr = a[17] > 0;
  if (has_hdr)
    WOQ_CHECK(woq_header_init(&h, a[17], (s.heads + 2 * s.kv_heads) * s.head_dim, a[18], (uint32_t)a[19], (uint32_t)a[20],
                              WOQ_C_FP32, a[21], a[22]) == 0,
              "QBits: bad argument");
  const AttnFacts f{a[13] != 0, a[14] != 0, a[15], has_hdr ? &h : nullptr, a[16]};
  const AttnDecodePlan p = plan_attn_decode(s, o, f);
  attn_plan_report(p, out11);
  if (p.error != nullptr) return 1;
  WOQ_END
}

// the engine's separate decode-attention launches on their own (both probes below)
static int probe_attn_decode(const float* qkv, void* kcache, void* vcache, int kv_dtype, const int32_t* pos_dev,
                             const float* cos_dev, const float* sin_dev, int heads, int kv_heads, int head_dim,
                             int max_ctx, int window, int splits, int grouped, int merge, int chunk_fixed, float* out,
                             void* stream, const float* q_norm, const float* k_norm, float qk_eps) {
  WOQ_TRY
  WOQ_CHECK(heads > 0 && kv_heads > 0 && heads % kv_heads == 0 && max_ctx > 0 && window >= 0 && splits >= 1,
            "QBits: bad attention shape");
  WOQ_CHECK(merge == 0 || merge == 1, "QBits: merge must be 0 (combine launch) or 1 (last-arriver counters)");
  const hipStream_t st = (hipStream_t)stream;
  AttnOptions o;
  o.splits = splits, o.grouped = grouped != 0, o.fold = merge != 0, o.chunk_fixed = chunk_fixed;
  const AttnDecodePlan plan = plan_attn_decode(AttnShape{heads, kv_heads, head_dim, kv_dtype, max_ctx, window}, o,
                                               AttnFacts{false, false, 0, nullptr, 0, q_norm != nullptr});
  if (plan.error != nullptr) return woq::fail(plan.error);
  // the partial buffer of woq_attn_merge.h (o [heads][64][D], then ml [heads][64][2]) and one counter per head
  const size_t part_bytes = (size_t)heads * ATTN_MAX_SLICES * (head_dim + 2) * sizeof(float);
  float* part = nullptr;
  unsigned int* counters = nullptr;
  WOQ_HIP(hipMallocAsync((void**)&part, part_bytes, st));
  if (merge) {
    if (hipMallocAsync((void**)&counters, (size_t)heads * sizeof(unsigned int), st) != hipSuccess ||
        hipMemsetAsync(counters, 0, (size_t)heads * sizeof(unsigned int), st) != hipSuccess) {
      if (counters) hipFreeAsync(counters, st);
      hipFreeAsync(part, st);
      return woq::fail("QBits: could not allocate the attention merge counters");
    }
  }
  const AttnDecodeIO io{qkv, kcache, vcache, pos_dev, cos_dev, sin_dev, out, XqPtrs{nullptr, nullptr, nullptr},
                        part, counters, nullptr, nullptr, 0, nullptr, q_norm, k_norm, qk_eps};
  const int rc = launch_attn_decode(plan, io, st);
  const hipError_t le = hipGetLastError();
  if (counters) hipFreeAsync(counters, st);
  hipFreeAsync(part, st);
  if (rc) return rc;
  WOQ_HIP(le);
  WOQ_END
}

// test entry points (include/woq_hip_experimental.h)
WOQ_API int woq_probe_attn_decode(const float* qkv, void* kcache, void* vcache, int kv_dtype, const int32_t* pos_dev,
                                  const float* cos_dev, const float* sin_dev, int heads, int kv_heads, int head_dim,
                                  int max_ctx, int window, int splits, int grouped, int merge, int chunk_fixed,
                                  float* out, void* stream) {
  return probe_attn_decode(qkv, kcache, vcache, kv_dtype, pos_dev, cos_dev, sin_dev, heads, kv_heads, head_dim, max_ctx,
                           window, splits, grouped, merge, chunk_fixed, out, stream, nullptr, nullptr, 0.f);
}
WOQ_API int woq_probe_attn_decode_qknorm(const float* qkv, void* kcache, void* vcache, int kv_dtype,
                                         const int32_t* pos_dev, const float* cos_dev, const float* sin_dev, int heads,
                                         int kv_heads, int head_dim, int max_ctx, int window, int splits, int merge,
                                         const float* q_norm_dev, const float* k_norm_dev, float eps, float* out,
                                         void* stream) {
  if (q_norm_dev == nullptr || k_norm_dev == nullptr) return woq::fail("QBits: q_norm and k_norm come together");
  return probe_attn_decode(qkv, kcache, vcache, kv_dtype, pos_dev, cos_dev, sin_dev, heads, kv_heads, head_dim, max_ctx,
                           window, splits, 0, merge, 0, out, stream, q_norm_dev, k_norm_dev, eps);
}

}  // extern "C"
