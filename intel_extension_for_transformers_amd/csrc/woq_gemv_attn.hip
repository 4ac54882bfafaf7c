// woq_gemv_attn.hip — [RMSNorm + qkv GEMV] and [RoPE + KV append + single-query attention] of a decode step in ONE
// launch (round 3). Reference path replaced: qbits.cpp:113-140 at M = 1 followed by stock HF eager attention on the CPU.
//
// Why. Inside the captured decode step every launch costs ~2 us before it does anything (measured with an empty
// kernel on the same grid, hipGraph replay: 1.7-2.4 us), and the batch-1 attention launch is a latency chain of 32
// workgroups that costs 5.0 us per layer in place (profiles/r03g_skip_masks.txt) — most of it waiting for its own
// first requests (position, cos / sin row, K / V rows) after the boundary. The qkv -> attention edge is the one edge of
// the layer that is NOT all-to-all: head h needs only the 24 column strips that hold its q, k and v rows.
// How. The grid is the GEMV's strips plus one attention workgroup per head at its END. An attention workgroup issues
// everything that does not depend on this token's q / k / v at once (position, K / V rows of its first passes, cos /
// sin), then its wave 0 re-reads the head's 384 {tag, value} granules until every tag is this (step, layer)'s; a strip
// workgroup's epilogue writes its 16 outputs as such granules — one 8-byte write-through agent-scope store each, the
// data is its own flag (cdna_hip_programming.md Guideline 16, form R2: no fence, no flag that can overtake its data).
// Tags come from a device-side step counter (the step's first kernel advances it), so a replayed graph sees fresh
// tags; the wait is bounded (~20 ms, then a sticky status word) and needs no dispatch order: strips never wait, and
// 32 waiting workgroups cannot keep 768 strips off a chip that holds all of them at once.
// A first form without resident attention workgroups — the strip that completes a head runs its attention — was
// correct but slower than two launches (profiles/r03j_fused_attn_last_arriver_negative.txt).
// Scope: head_dim 128, K = 32 tiles at 8 per wave (4 waves), up to 16 context slices that merge among themselves; the
// rule is the plan's (woq_attn_decode.hip plan_attn_decode, fused_attn_covers), and this launcher takes the plan's
// slices, span and LDS. Everything else keeps the separate launches.
// Layer extras (woq_engine_set_layer_extras): a qkv bias rides in the strips' epilogue (XqsLate.bias); a q / k norm runs
// inside the attention workgroups, in a kernel of its own (gemv_xqs_attn_qkn_kernel) over the same body.
#include <algorithm>
#include <cstdlib>

#include "woq_attn_decode.h"
#include "woq_gemv_common.h"
#include "woq_gemv_launch.h"
#include "woq_gemv_xqs.h"
#include "woq_host.h"
#include "woq_xq.h"

namespace woq {

struct FusedAttnArgs {
  const unsigned int* seq;  // device-side step counter (advanced by the step's first kernel): tag = seq << 6 | layer
  int layer;
  int* status;              // sticky: set when an attention workgroup gave up waiting
  void* kcache;
  void* vcache;
  const int32_t* pos;
  const float* cs;
  const float* sn;
  int heads, kv_heads, window, spw;
  float* attn_out;  // fp32 [heads * 128] attention output
  XqPtrs xq_attn;
  int ns;           // context slices per head (round 6): heads * ns attention workgroups behind the strips
  unsigned long long* part_g;  // ns > 1: the slices' partials as tagged granules (woq_attn_decode.h attn_part_granule)
};

// Round 6: the q strips of the fused launch are given the WHOLE slice as their window (8 tiles per wave up front) and the
// k / v strips a shallower one, so that q lands while k / v are still streaming: the attention workgroups then run
// everything over the cache on q alone (woq_attn_decode.h) and only the new position's score and value stand behind
// the launch's last strips. (Depth 4 for both is the round-5 order of arrival.)
constexpr int FUSED_DQ = 8, FUSED_DKV = 1;
// the fused launch's 14th argument dword: tpg_shift | flags << 8 | strips << 16 — the strip workgroups come first in the
// grid, one attention workgroup per head behind them — so that the role test needs nothing but preloaded arguments
// (gridDim is a hidden argument: it lives in the argument segment too)
__device__ __forceinline__ int fa_strips_of_grid(int tpg_flags) { return (tpg_flags >> 16) & 0xffff; }

// the body of both kernels below; QKN: the attention workgroups run the per-head q / k RMSNorm `qn` (woq_attn_decode.h)
template <int SMODE, bool ASYM, bool S32, typename KV, bool QKN>
__device__ __forceinline__ void gemv_xqs_attn_body(const u32x4* __restrict__ q, const void* __restrict__ scales,
                                                   const uint8_t* __restrict__ xlimbs, const float* __restrict__ xu,
                                                   int tiles_k, int n_q_strips, int base_tiles, int rem_tiles,
                                                   int n_groups, int tpg_flags, unsigned long long* __restrict__ qkv_g,
                                                   const FusedAttnArgs& fa, const AttnQkNorm& qn) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int n_strips = fa_strips_of_grid(tpg_flags);
  if ((int)blockIdx.x >= n_strips) {  // the attention workgroup of head blockIdx.x - n_strips
    const unsigned int tag = (fa.seq[0] << 6) | (unsigned int)fa.layer;
    const int a = (int)blockIdx.x - n_strips;
    if (fa.ns > 1) {
      // Context slices inside the fused launch (round 6, long contexts): heads * ns attention workgroups, each the
      // per-head flash-decoding slice of woq_attn_decode.h on a granule source — its K / V rows (they depend on the
      // position only) stream beside the launch's weight tiles while q is still in the making; the slices of a head then
      // merge among themselves (tagged partial granules, every slice finalises a share of the head's XQ blocks): no
      // combine launch. Workgroup ids go round-robin over the 8 XCDs: the query heads that share a kv head AND a slice
      // read the same cache rows, so they get ids that differ by multiples of 8 (one L2 pulls the rows from HBM once).
      const int rep = fa.heads / fa.kv_heads, groups = fa.kv_heads * fa.ns;
      int h, slice;
      if ((groups & 7) == 0 && (n_strips & 7) == 0) {
        const int y = a >> 3, gi = (a & 7) + 8 * (y / rep);
        h = (gi / fa.ns) * rep + y % rep, slice = gi % fa.ns;
      } else {
        h = a / fa.ns, slice = a % fa.ns;
      }
      attn_decode_body<KV, 128, true, AttnGranule, QKN>(
          (float*)smem_raw, h, slice, fa.ns, AttnGranule{qkv_g, tag, fa.status, fa.part_g}, (KV*)fa.kcache,
          (KV*)fa.vcache, fa.pos, fa.cs, fa.sn, fa.heads, fa.kv_heads, fa.window, fa.spw, fa.attn_out, fa.xq_attn,
          XqPub{nullptr, 0u}, qn);
      return;
    }
    attn_decode_body<KV, 128, false, AttnGranule, QKN>((float*)smem_raw, a, 0, 1, AttnGranule{qkv_g, tag, fa.status},
                                                       (KV*)fa.kcache, (KV*)fa.vcache, fa.pos, fa.cs, fa.sn, fa.heads,
                                                       fa.kv_heads, fa.window, fa.spw, fa.attn_out, fa.xq_attn,
                                                       XqPub{nullptr, 0u}, qn);
    return;
  }
  // (the K range always starts at tile 0 here: the kt_off slot of the preloaded dwords carries the number of q strips)
  if ((int)blockIdx.x < n_q_strips)
    gemv_xqs_body<FUSED_TPW, 1, FUSED_DQ, SMODE, ASYM, S32, true>(smem_raw, q, scales, xlimbs, xu, tiles_k, 0, base_tiles,
                                                                     rem_tiles, n_groups, tpg_flags & 0xff,
                                                                     (tpg_flags >> 8) & 0xff, 4, xqs_late_ptr());
  else
    gemv_xqs_body<FUSED_TPW, 1, FUSED_DKV, SMODE, ASYM, S32, true>(smem_raw, q, scales, xlimbs, xu, tiles_k, 0, base_tiles,
                                                                      rem_tiles, n_groups, tpg_flags & 0xff,
                                                                      (tpg_flags >> 8) & 0xff, 4, xqs_late_ptr());
}

template <int SMODE, bool ASYM, bool S32, typename KV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void gemv_xqs_attn_kernel(
    const u32x4* __restrict__ q, const void* __restrict__ scales, const uint8_t* __restrict__ xlimbs,
    const float* __restrict__ xu, int tiles_k, int n_q_strips, int base_tiles, int rem_tiles, int n_groups, int tpg_flags,
    XqsLate late_in_the_argument_segment, unsigned long long* __restrict__ qkv_g, int N, FusedAttnArgs fa) {
  gemv_xqs_attn_body<SMODE, ASYM, S32, KV, false>(q, scales, xlimbs, xu, tiles_k, n_q_strips, base_tiles, rem_tiles, n_groups,
                                                  tpg_flags, qkv_g, fa, AttnQkNorm{nullptr, nullptr, 0.f});
}
// the same launch for layers with a q / k norm (Qwen3): a kernel of its own, the norm's arguments behind the others, so
// that the one above keeps its argument segment and its code
template <int SMODE, bool ASYM, bool S32, typename KV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void gemv_xqs_attn_qkn_kernel(
    const u32x4* __restrict__ q, const void* __restrict__ scales, const uint8_t* __restrict__ xlimbs,
    const float* __restrict__ xu, int tiles_k, int n_q_strips, int base_tiles, int rem_tiles, int n_groups, int tpg_flags,
    XqsLate late_in_the_argument_segment, unsigned long long* __restrict__ qkv_g, int N, FusedAttnArgs fa, AttnQkNorm qn) {
  gemv_xqs_attn_body<SMODE, ASYM, S32, KV, true>(q, scales, xlimbs, xu, tiles_k, n_q_strips, base_tiles, rem_tiles, n_groups,
                                                 tpg_flags, qkv_g, fa, qn);
}

// what the fused launch carries beside the blob (BlobView)
struct FusedLaunch {
  XqPtrs xin;
  int flags, n_ssq;
  unsigned long long* out;
  float eps;
  const float* ssq_in;
  const float* bias;  // fp32 [N] or null: added by the strips' epilogue (Qwen2's q / k / v biases)
  FusedAttnArgs fa;
  AttnQkNorm qn;  // q == null: no q / k norm
  size_t lds_attn;
};

template <int SMODE, bool ASYM, bool S32, typename KV, bool QKN>
static int launch_fused_t(const BlobView& v, const FusedLaunch& a, hipStream_t st) {
  // every workgroup gets max(attention LDS, GEMV LDS)
  const size_t lds = std::max(a.lds_attn, XqsLds<FUSED_TPW, 1, SMODE, ASYM, S32>::total(4));
  if (lds > 160 * 1024) return woq::fail("QBits: fused qkv + attention launch does not fit LDS");
  constexpr auto kern = gemv_xqs_attn_kernel<SMODE, ASYM, S32, KV>;
  constexpr auto kern_qkn = gemv_xqs_attn_qkn_kernel<SMODE, ASYM, S32, KV>;
  if (const int rc = QKN ? allow_dynamic_lds<kern_qkn>(160 * 1024) : allow_dynamic_lds<kern>(160 * 1024)) return rc;
  XqsLate late;
  late.zp = v.zp, late.xsx = a.xin.sx, late.out = (float*)a.out, late.bias = a.bias, late.residual = nullptr;
  late.ssq_in = a.ssq_in, late.next_norm_w = nullptr, late.ssq_out = nullptr, late.tp = nullptr;
  late.tag_seq = a.fa.seq, late.tag_layer = a.fa.layer, late.xo = XqPtrs{nullptr, nullptr, nullptr}, late.eps = a.eps;
  late.N = v.N, late.K = v.K, late.n_ssq = a.n_ssq, late.lut = LutArgs{};
  if constexpr (QKN)
    hipLaunchKernelGGL(kern_qkn, dim3(v.N / 16 + a.fa.heads * a.fa.ns), dim3(256), lds, st, v.q, v.scales, a.xin.limbs,
                       a.xin.u, v.tiles_k, a.fa.heads * 8, FUSED_TPW, 0, v.n_groups,
                       v.tpg_shift | (a.flags << 8) | ((v.N / 16) << 16), late, a.out, v.N, a.fa, a.qn);
  else
    hipLaunchKernelGGL(kern, dim3(v.N / 16 + a.fa.heads * a.fa.ns), dim3(256), lds, st, v.q, v.scales, a.xin.limbs,
                       a.xin.u, v.tiles_k, a.fa.heads * 8, FUSED_TPW, 0, v.n_groups,
                       v.tpg_shift | (a.flags << 8) | ((v.N / 16) << 16), late, a.out, v.N, a.fa);
  return 0;
}

template <typename KV>
static int launch_fused_kv(const BlobView& v, const FusedLaunch& a, hipStream_t st) {
  return select_qform<true>(v.smode, v.asym, v.s32, v.ndig, "QBits: bad fused qkv + attention configuration",
                            [&](auto SM, auto AS, auto S3, auto) {
                              return a.qn.q != nullptr ? launch_fused_t<SM(), AS(), S3(), KV, true>(v, a, st)
                                                          : launch_fused_t<SM(), AS(), S3(), KV, false>(v, a, st);
                            });
}

int launch_gemv_xq_attn(const AttnDecodePlan& plan, const AttnDecodeIO& io, const XqPtrs& xin, const void* blob,
                        const woq_blob_header& h, unsigned long long* qkv_g, const float* ssq_in, float eps,
                        hipStream_t st, const float* bias) {
  BlobView v;
  if (plan.form != ATTN_FUSED || !blob_view(blob, h, v)) return woq::fail("QBits: bad fused qkv + attention configuration");
  if (plan.slices > 1 && io.part_g == nullptr)
    return woq::fail("QBits: context slices in the fused launch need the partial granules");
  if ((io.q_norm != nullptr) != (io.k_norm != nullptr)) return woq::fail("QBits: q_norm and k_norm come together");
  FusedLaunch a;
  a.xin = xin;
  a.flags = v.sbf16 ? 1 : 0;
  a.eps = eps;
  a.n_ssq = h.K / 16;
  a.ssq_in = ssq_in;
  a.bias = bias;
  a.out = qkv_g;
  const AttnShape& s = plan.shape;
  a.fa = FusedAttnArgs{io.seq, io.layer, io.status, io.kcache, io.vcache, io.pos, io.cs, io.sn, s.heads, s.kv_heads,
                       s.window, plan.spw, io.out, io.xo, plan.slices, io.part_g};
  a.qn = AttnQkNorm{io.q_norm, io.k_norm, io.qk_eps};
  a.lds_attn = plan.lds;
  if (s.kv_dtype == WOQ_F16) return launch_fused_kv<_Float16>(v, a, st);
  if (s.kv_dtype == WOQ_FP8_E4M3) return launch_fused_kv<Fp8>(v, a, st);
  return launch_fused_kv<__bf16>(v, a, st);
}

}  // namespace woq
