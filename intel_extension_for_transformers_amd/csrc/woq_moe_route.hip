// woq_moe_route.hip — the router of a sparse mixture-of-experts layer (HF MixtralTopKRouter / Qwen3MoeTopKRouter), fp32:
//   xn = x * rsqrt(mean(x^2) + eps) * norm_w   (no norm_w: xn = x)        logit[e] = xn . router_w[e]
//   p = softmax(logit) over the E experts; the top_k largest p, descending, equal p: the lower expert id first;
//   w = p[idx], divided by its own sum (j ascending) when renorm is set.
// Everything is fp32 in a fixed order, no floating-point atomics: the same inputs give the same bytes.
//
// Two forms, one launch each.
//  Decode (T = 1). A wave owns one expert row, a workgroup four of them, so the E rows of a large router are streamed by
//   E / 4 workgroups across the chip instead of through one CU. Every wave recomputes the row's RMS factor (H floats out
//   of L2: cheaper than a launch that would hand it over), keeps a lane-strided fmaf chain over its router row and adds
//   the lanes by butterflies. Logits go to a device scratch; an integer ticket behind a fence tells the last workgroup
//   to arrive, which does the soft-max and the selection, writes xn, and leaves the ticket zero for the next launch.
//   A single workgroup of 16 waves measured level at E = 8 and 2.4 times slower at E = 128: not kept.
//  Prompt (T > 1). A workgroup owns 16 rows. Its four waves first take four rows each for the RMS factors, then
//   interleave over K in 16-k runs: a lane loads four consecutive k of its row, applies factor and norm_w, stores them as
//   xn (every element passes exactly one lane) and feeds them to four v_mfma_f32_16x16x4_f32 per 16-expert column tile —
//   fp32 operands, so routing stays fp32-class. The waves' partial tiles are added in wave order into one LDS tile
//   [16][E], on which 16-lane groups do the soft-max and the selection of their row.
// The selection is a rank count, not a sort: lane g of a row's group holds experts g, g + G, ... and counts, for each, the
// experts that beat it (larger p, or equal p and a lower id); a rank below top_k is its output slot. E <= 256 keeps this
// at E LDS broadcast reads per expert, with no data-dependent control flow.
// Also here: the engine's combine of the experts' rows onto the fp32 residual stream (moe_combine_residual_kernel below).
#include <math.h>

#include <string>

#include "woq_device.h"
#include "woq_host.h"
#include "../../include/woq_hip_experimental.h"

namespace woq {
namespace {

constexpr int ROUTE_MAX_E = 256, ROUTE_MAX_K = 16;
constexpr int ROUTE_ROWS = 16;                    // rows of a prompt-form workgroup: one MFMA tile
constexpr size_t ROUTE_TICKET_OFF = ROUTE_MAX_E * 4;  // scratch: fp32 logits [256] | the ticket word
constexpr size_t ROUTE_SCRATCH_BYTES = ROUTE_TICKET_OFF + 256;

struct RouteArgs {
  const float* x; int ldx;
  const float* norm_w; float eps;
  const void* rw; int rw_dtype;
  int T, H, E, top_k, renorm;
  float* xn; int32_t* idx; float* w;
  float* logits; unsigned int* ticket;  // decode form only
  // decode form, all four or none: the one row's plan in woq_moe.hip's format (the top_k slots hold distinct experts)
  int32_t* sorted; int32_t* pos_of; MoeBlock* blocks; int32_t* nblocks;
};

__device__ __forceinline__ float4_t route_w4(const void* rw, int dt, size_t off) {
  if (dt == WOQ_F32) return *(const float4_t*)((const float*)rw + off);
  const uint2 r = *(const uint2*)((const uint16_t*)rw + off);
  const uint16_t b[4] = {(uint16_t)r.x, (uint16_t)(r.x >> 16), (uint16_t)r.y, (uint16_t)(r.y >> 16)};
  if (dt == WOQ_BF16) return float4_t{bf16_bits_to_f32(b[0]), bf16_bits_to_f32(b[1]), bf16_bits_to_f32(b[2]), bf16_bits_to_f32(b[3])};
  return float4_t{f16_bits_to_f32(b[0]), f16_bits_to_f32(b[1]), f16_bits_to_f32(b[2]), f16_bits_to_f32(b[3])};
}

// one wave: 1 / sqrt(mean(x^2) + eps) of a row, lane-strided fmaf chains met by xor butterflies (every lane ends on the
// same bits, and so does every wave that runs this over the same row)
__device__ __forceinline__ float route_row_inv(const float* __restrict__ xrow, int H, float eps, int lane) {
  float ss = 0.f;
#pragma unroll 4
  for (int k = lane * 4; k < H; k += 256) {
    const float4_t v = *(const float4_t*)(xrow + k);
    ss = fmaf(v.x, v.x, ss);
    ss = fmaf(v.y, v.y, ss);
    ss = fmaf(v.z, v.z, ss);
    ss = fmaf(v.w, v.w, ss);
  }
  ss = wave_sum(ss);
  return 1.0f / sqrtf(ss / (float)H + eps);
}

__device__ __forceinline__ float4_t route_xn4(float4_t v, float inv, const float* __restrict__ norm_w, int k) {
  if (norm_w == nullptr) return v;
  const float4_t g = *(const float4_t*)(norm_w + k);
  return float4_t{(v.x * inv) * g.x, (v.y * inv) * g.y, (v.z * inv) * g.z, (v.w * inv) * g.w};
}

// Soft-max and selection of one row by a group of G threads (g = the thread's place in it). L: the row's E logits in
// LDS, P: E floats of LDS scratch, sel_i / sel_w: ROUTE_MAX_K slots of LDS. Holds barriers: the whole workgroup calls it,
// `live` false for a row past T (nothing is written to global memory).
template <int G>
__device__ __forceinline__ void route_select(float* L, float* P, int32_t* sel_i, float* sel_w, int g, bool live,
                                             const RouteArgs& a, int row) {
  const int E = a.E, K = a.top_k;
  float m = -INFINITY;
  for (int e = 0; e < E; ++e) m = fmaxf(m, L[e]);
  for (int e = g; e < E; e += G) P[e] = expf(L[e] - m);
  if (g < ROUTE_MAX_K) sel_i[g] = -1, sel_w[g] = 0.f;
  __syncthreads();
  float s = 0.f;
  for (int e = 0; e < E; ++e) s += P[e];  // ascending, every thread of the group alike
  for (int e = g; e < E; e += G) L[e] = P[e] / s;
  __syncthreads();
  // a NaN p (a NaN or infinite input) ranks below every number, so ranks stay a permutation and ids stay in [0, E)
  for (int e = g; e < E; e += G) {
    const float pe = L[e], ke = pe != pe ? -1.f : pe;
    int rank = 0;
    for (int j = 0; j < E; ++j) {
      const float pj = L[j], kj = pj != pj ? -1.f : pj;
      rank += (kj > ke || (kj == ke && j < e)) ? 1 : 0;
    }
    if (rank < K) sel_i[rank] = e, sel_w[rank] = pe;
  }
  __syncthreads();
  if (g < K && live) {
    float d = 1.f;
    if (a.renorm) {
      d = 0.f;
      for (int j = 0; j < K; ++j) d += sel_w[j];
    }
    a.idx[(size_t)row * K + g] = sel_i[g];
    a.w[(size_t)row * K + g] = a.renorm ? sel_w[g] / d : sel_w[g];
  }
}

// ---- decode form -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_route_decode_kernel(const RouteArgs a) {
  __shared__ float L[ROUTE_MAX_E], P[ROUTE_MAX_E], sel_w[ROUTE_MAX_K];
  __shared__ int32_t sel_i[ROUTE_MAX_K];
  __shared__ int is_last;
  const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int waves = (int)blockDim.x >> 6;
  const float inv = a.norm_w != nullptr ? route_row_inv(a.x, a.H, a.eps, lane) : 1.f;
  for (int e = (int)blockIdx.x * waves + wid; e < a.E; e += (int)gridDim.x * waves) {
    float acc = 0.f;
#pragma unroll 4
    for (int k = lane * 4; k < a.H; k += 256) {
      const float4_t xv = route_xn4(*(const float4_t*)(a.x + k), inv, a.norm_w, k);
      const float4_t wv = route_w4(a.rw, a.rw_dtype, (size_t)e * a.H + k);
      acc = fmaf(xv.x, wv.x, acc);
      acc = fmaf(xv.y, wv.y, acc);
      acc = fmaf(xv.z, wv.z, acc);
      acc = fmaf(xv.w, wv.w, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) a.logits[e] = acc;
  }
  // count in; the last workgroup to arrive finishes for all of them (a grid of one workgroup has nobody to wait for)
  __threadfence();
  __syncthreads();
  if (gridDim.x > 1) {
    if (tid == 0) {
      const unsigned int prev = atomicAdd(a.ticket, 1u);
      is_last = prev == gridDim.x - 1 ? 1 : 0;
      if (is_last) *a.ticket = 0u;  // zero again for the next launch
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
  }
  if (tid < a.E)
    L[tid] = __uint_as_float(__hip_atomic_load((const unsigned int*)a.logits + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __syncthreads();
  route_select<256>(L, P, sel_i, sel_w, tid, true, a, 0);
  // the plan: slot j's place among the slots in expert order = the selected experts below its own; one block a slot
  if (a.sorted != nullptr && tid < a.top_k) {
    int p = 0;
    for (int j = 0; j < a.top_k; ++j) p += sel_i[j] < sel_i[tid] ? 1 : 0;
    a.sorted[p] = tid;
    a.pos_of[tid] = p;
    a.blocks[p] = MoeBlock{sel_i[tid], p, 1, 0};
    if (tid == 0) *a.nblocks = a.top_k;
  }
  if (a.xn != nullptr)
    for (int k = tid * 4; k < a.H; k += (int)blockDim.x * 4)
      *(float4_t*)(a.xn + k) = route_xn4(*(const float4_t*)(a.x + k), inv, a.norm_w, k);
}

// ---- prompt form -----------------------------------------------------------------------------------------------------
// NT = column tiles of 16 experts the accumulators hold (E <= 16 NT)
template <int NT>
__global__ __launch_bounds__(256) void moe_route_prompt_kernel(const RouteArgs a) {
  constexpr int LD = NT * 16 + 1;  // odd: the 16 rows' reads of one expert fall on distinct banks
  __shared__ float L[ROUTE_ROWS][LD], P[ROUTE_ROWS][LD];
  __shared__ float sel_w[ROUTE_ROWS][ROUTE_MAX_K], inv_s[ROUTE_ROWS];
  __shared__ int32_t sel_i[ROUTE_ROWS][ROUTE_MAX_K];
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6, i16 = lane & 15, kq = lane >> 4;
  const int m0 = (int)blockIdx.x * ROUTE_ROWS;
  const bool norm = a.norm_w != nullptr;
  for (int r = wid; r < ROUTE_ROWS; r += 4) {
    const int row = m0 + r;
    const float inv = (norm && row < a.T) ? route_row_inv(a.x + (size_t)row * a.ldx, a.H, a.eps, lane) : 1.f;
    if (lane == 0) inv_s[r] = inv;
  }
  __syncthreads();

  const int m = m0 + i16;
  const bool row_live = m < a.T;
  const float* xrow = a.x + (size_t)(row_live ? m : 0) * a.ldx;
  const float inv = inv_s[i16];
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float4_t zero = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = wid * 16; k0 < a.H; k0 += 64) {  // (a wave's trip count is uniform: the MFMA is wave-wide)
    const int k = k0 + kq * 4;
    const bool k_live = k < a.H;  // H % 4 == 0: a lane's four k are inside or outside together
    float4_t xv = zero;
    if (k_live && row_live) {
      xv = route_xn4(*(const float4_t*)(xrow + k), inv, a.norm_w, k);
      if (a.xn != nullptr) *(float4_t*)(a.xn + (size_t)m * a.H + k) = xv;
    }
    // all tiles' router words are requested first; then the tiles alternate inside each k, so that back-to-back MFMAs
    // write different accumulators (per accumulator the k order stays x, y, z, w)
    float4_t wv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int e = t * 16 + i16;
      wv[t] = (k_live && e < a.E) ? route_w4(a.rw, a.rw_dtype, (size_t)e * a.H + k) : zero;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.x, wv[t].x, acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.y, wv[t].y, acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.z, wv[t].z, acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.w, wv[t].w, acc[t], 0, 0, 0);
  }
  // D: register v of lane l = row 4 (l >> 4) + v, expert column l & 15 of the tile. The waves add in wave order.
#pragma unroll 1
  for (int w = 0; w < 4; ++w) {
    if (wid == w) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float* p = &L[4 * kq + v][t * 16 + i16];
          *p = w == 0 ? acc[t][v] : *p + acc[t][v];
        }
    }
    __syncthreads();
  }
  const int r = tid >> 4, g = tid & 15;
  route_select<16>(L[r], P[r], sel_i[r], sel_w[r], g, m0 + r < a.T, a, m0 + r);
}

const char* route_problem(const RouteArgs& a, const void* scratch) {
  if (a.H <= 0 || a.H % 4 != 0) return "QBits: woq_moe_route: the hidden size must be a positive multiple of 4";
  if (a.E < 1 || a.E > ROUTE_MAX_E) return "QBits: woq_moe_route takes 1 to 256 experts";
  if (a.top_k < 1 || a.top_k > ROUTE_MAX_K || a.top_k > a.E) return "QBits: woq_moe_route takes 1 <= top_k <= min(E, 16)";
  if (a.rw_dtype != WOQ_F32 && a.rw_dtype != WOQ_BF16 && a.rw_dtype != WOQ_F16)
    return "QBits: woq_moe_route takes a router weight in fp32, bf16 or fp16";
  if (a.T < 0 || (long long)a.T > 0x7fffffffll / ROUTE_MAX_K) return "QBits: woq_moe_route: bad row count";
  if (a.T == 0) return nullptr;
  if (!a.x || !a.rw || !a.idx || !a.w) return "QBits: woq_moe_route: null tensor";
  if (a.ldx < a.H || a.ldx % 4 != 0 || (uintptr_t)a.x % 16 != 0 || (uintptr_t)a.rw % 16 != 0 ||
      (a.norm_w && (uintptr_t)a.norm_w % 16 != 0) || (a.xn && (uintptr_t)a.xn % 16 != 0))
    return "QBits: woq_moe_route: rows must be 16-byte aligned and ldx a multiple of 4 no smaller than the hidden size";
  if (a.T == 1 && (!scratch || (uintptr_t)scratch % 4 != 0))
    return "QBits: woq_moe_route: one row needs the scratch of woq_moe_route_scratch_bytes (zero before its first use)";
  const int n_plan = (a.sorted != nullptr) + (a.pos_of != nullptr) + (a.blocks != nullptr) + (a.nblocks != nullptr);
  if (n_plan != 0 && (n_plan != 4 || a.T != 1))
    return "QBits: woq_moe_route writes the plan tables for one row only, all four of them or none";
  return nullptr;
}

// ---- combine onto the residual stream ----------------------------------------------------------------------------------
// A thread owns one (row, column): its k products are chained by fmaf in slot order and added onto the residual once.
// With xo (one row, H % 16 == 0, so a DPP row of 16 lanes lies wholly inside the row) the 16 lanes that hold block
// n / 16 of the new row convert it for the next layer's first GEMV: xq_emit16 of value * next_norm_w and the block's sum
// of squares of the raw values, as the dense layer's down_proj epilogue does.
__global__ __launch_bounds__(256) void moe_combine_residual_kernel(const float* __restrict__ y,
                                                                   const int32_t* __restrict__ pos_of,
                                                                   const float* __restrict__ topk_w, int top_k, int H,
                                                                   const MoeResidual r) {
  const int t = (int)blockIdx.y, n = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (n >= H) return;
  float acc = 0.f;
  for (int j = 0; j < top_k; ++j) {
    const int p = pos_of[t * top_k + j];
    if (p >= 0) acc = fmaf(topk_w[t * top_k + j], y[(size_t)p * H + n], acc);  // a dropped slot contributes zero
  }
  float* h = r.hidden + (size_t)t * r.ldh + n;
  const float v = *h + acc;
  *h = v;
  if (r.xo.limbs != nullptr) {
    const float ss = r.ssq_out != nullptr ? row16_sum(v * v) : 0.f;
    xq_emit16<false>(r.next_norm_w != nullptr ? v * r.next_norm_w[n] : v, r.xo, n >> 4, n & 15, XqPub{nullptr, 0u},
                     r.ssq_out, ss);
  }
}

}  // namespace

int launch_moe_combine_residual(const float* y, const int32_t* pos_of, const float* topk_w, int T, int top_k, int H,
                                const MoeResidual& r, hipStream_t st) {
  if (!y || !pos_of || !topk_w || !r.hidden || T <= 0 || top_k <= 0 || H <= 0 || r.ldh < H)
    return woq::fail("QBits: woq_moe combine onto the residual stream: bad arguments");
  if (r.xo.limbs != nullptr && (T != 1 || H % 16 != 0))
    return woq::fail("QBits: woq_moe combine emits the next layer's XQ vector for one row of a multiple of 16 columns");
  hipLaunchKernelGGL(moe_combine_residual_kernel, dim3((unsigned)((H + 255) / 256), (unsigned)T), dim3(256), 0, st, y, pos_of,
                     topk_w, top_k, H, r);
  return 0;
}

int launch_moe_route(const float* x, int ldx, const float* norm_w, float eps, const void* router_w, int router_dtype,
                     int T, int H, int E, int top_k, int renorm, float* xn, int32_t* idx, float* w, void* scratch,
                     const MoeRoutePlan& plan, hipStream_t st) {
  RouteArgs a = {x,  ldx, norm_w, eps,     router_w, router_dtype, T, H, E, top_k, renorm,
                 xn, idx, w,      nullptr, nullptr, plan.sorted, plan.pos_of, plan.blocks, plan.nblocks};
  if (const char* why = route_problem(a, scratch)) return woq::fail(why);
  if (T == 0) return 0;
  if (T == 1) {
    a.logits = (float*)scratch;
    a.ticket = (unsigned int*)((uint8_t*)scratch + ROUTE_TICKET_OFF);
    hipLaunchKernelGGL(moe_route_decode_kernel, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, st, a);
    return 0;
  }
  const dim3 grid((unsigned)((T + ROUTE_ROWS - 1) / ROUTE_ROWS)), block(256);
  void (*kern)(const RouteArgs) = E <= 16   ? moe_route_prompt_kernel<1>
                                  : E <= 32  ? moe_route_prompt_kernel<2>
                                  : E <= 64  ? moe_route_prompt_kernel<4>
                                  : E <= 128 ? moe_route_prompt_kernel<8>
                                             : moe_route_prompt_kernel<16>;
  hipLaunchKernelGGL(kern, grid, block, 0, st, a);
  return 0;
}

}  // namespace woq

extern "C" size_t woq_moe_route_scratch_bytes(void) { return woq::ROUTE_SCRATCH_BYTES; }

extern "C" int woq_moe_route(const float* x_dev, int ldx, const float* norm_w_dev, float eps, const void* router_w_dev,
                                   int router_dtype, int T, int H, int E, int top_k, int renorm, float* xn_out,
                                   int32_t* idx_out, float* w_out, void* scratch_dev,
                                   int32_t* sorted_out, int32_t* pos_of_out, void* blocks_out, int32_t* nblocks_out,
                                   void* stream) {
  WOQ_TRY
  const woq::MoeRoutePlan plan = {sorted_out, pos_of_out, (woq::MoeBlock*)blocks_out, nblocks_out};
  if (const int rc = woq::launch_moe_route(x_dev, ldx, norm_w_dev, eps, router_w_dev, router_dtype, T, H, E, top_k, renorm,
                                           xn_out, idx_out, w_out, scratch_dev, plan, (hipStream_t)stream))
    return rc;
  WOQ_HIP(hipGetLastError());
  WOQ_END
}
