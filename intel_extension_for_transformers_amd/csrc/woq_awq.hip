// woq_awq.hip — the two searches of AWQ calibration (Lin et al. 2023, as in llm-awq / AutoAWQ, with the linear-output
// objective): tests/awq_reference.py is their float64 statement, transformers/llm/quantization/awq.py the driver.
//
//   w  fp32 [K, N] row-major, row k = input feature k (Linear.weight.T)
//   Q  the package's RTN at (bits, group, sym | asym): woq_rtn.h, the rule rtn_kernel (woq_pack.hip) writes blobs with
//
// 1. awq_scale_delta_kernel: D = diag(1 / s) Q(diag(s) W) - W for one candidate s [K] of the scale search. One thread per
//    column and group (woq_group_cols.h, the one-slice form), two passes over the group's rows (range, then codes); the
//    loss tr(D^T H D) is the caller's, a GEMM.
//    Every step is rounded on its own (no contraction): the product w * s, the dequantised code * scale, the correctly
//    rounded division by s, the subtraction. Memory bound, nothing to tune.
//
// 2. awq_clip_kernel<GROUP>: the clip search. For column n and group g (GROUP rows, a short last group as if padded with
//    zeros), candidates c_j = 1 - j / n_grid, j < n_cand: the group is clamped to +-c max|w| (sym) or to
//    [c min(min w, 0), c max(max w, 0)] (asym), each bound the double product rounded once to fp32; the clamped group's
//    RTN range is exactly those bounds, so its parameters come from them; d = Q(clamped) - w against the unclipped w;
//    e_j = d^T G d with G the group's diagonal block of h. losses[j][g][n] = e_j, best[g][n] = the first minimum,
//    w_out = w clamped by it.
//
//    Layout. A workgroup is 256 columns of one group: G sits in LDS (GROUP^2 floats, 64 KiB at 128, so two workgroups =
//    eight waves per CU) and every lane reads it at the same address, a broadcast ds_read_b128. A thread owns one column
//    and keeps the candidate's d[GROUP] in registers, every index a compile-time constant (the loops over it are
//    unrolled by template recursion, as in woq_gptq.hip). The quadratic form runs row by row,
//    e += d_i * (G[i][:] . d): the row index is a runtime value, so d_i is not taken from the register array (a runtime
//    index would send it to scratch) but computed again from w[i][n], re-read through the caches and requested one row
//    ahead — a dozen instructions beside the row's fmas, and bit-identical to d[i] because it is the same straight-line
//    rule. h is taken as symmetric (it is a Gram matrix): a row reads its own 16-column chunk of G and the chunks to
//    its right, those counted twice, 9 / 16 of the block at GROUP 128 (clip_rows). The dot product keeps four partial
//    sums. fp32 VALU throughout: d is a difference of near-equal numbers.
//    A broadcast ds_read_b128 delivers four floats per four LDS cycles, one float per clock per CU, against 128
//    fma lanes per clock: at two waves per SIMD the LDS, not the VALU, bounds the row at half the fp32 vector rate.
//    Measured (profiles/r16_awq.txt): 1.12 ms for a 4096 x 4096 linear at GROUP 128, 19 T fma/s counted on the full
//    block, about a third of that bound; the reads come in bursts that are drained before the next, and two waves
//    per SIMD do not cover them. A version that re-read all of G per row, with the row's w not requested ahead and the
//    per-row addresses hoisted out of the candidate loop (472 registers, one wave per SIMD), took 2.36 ms.
//    Registers (tools/kres.py), sym / asym: GROUP 128 = 217 / 221 VGPRs, 64 = 162 / 166, 32 = 97 / 93; 64 / 16 / 4 KiB
//    LDS; no AGPRs, no scratch, no spills; the delta kernel 24 VGPRs.
#include "woq_device.h"
#include "woq_group_cols.h"

namespace woq {
namespace {

constexpr int AWQ_THREADS = GC_THREADS;  // both kernels: 256 columns of one group per workgroup

// ---- 1. the scale search's delta ------------------------------------------------------------------------------------
__global__ __launch_bounds__(AWQ_THREADS) void awq_scale_delta_kernel(const float* __restrict__ w,
                                                                      const float* __restrict__ sc, int K, int N,
                                                                      int group, int bits, int asym,
                                                                      float* __restrict__ dout) {
  const int n = blockIdx.x * AWQ_THREADS + threadIdx.x;
  if (n >= N) return;
  const RtnRange r = rtn_range(bits);
  const int k0 = blockIdx.y * group, k1 = min(K, k0 + group);
  float mx, mn, amax;
  {
    const float v = w[(size_t)k0 * N + n] * sc[k0];
    mx = mn = v;
    amax = fabsf(v);
  }
  for (int k = k0 + 1; k < k1; ++k) {
    const float v = w[(size_t)k * N + n] * sc[k];
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
    amax = fmaxf(amax, fabsf(v));
  }
  float s;
  int z;
  rtn_params(r, asym, mx, mn, amax, s, z);
  for (int k = k0; k < k1; ++k) {
    // no contraction: the scaled weight, the dequantised value and the quotient are each rounded before the next step
    // (contracted, deq / s - w or code * scale would fuse with a neighbour and skip a rounding the definition has)
#pragma clang fp contract(off)
    const float wk = w[(size_t)k * N + n], sk = sc[k];
    const float v = wk * sk;
    const float back = rtn_deq(r, asym, v, s, z) / sk;
    dout[(size_t)k * N + n] = back - wk;
  }
}

// ---- 2. the clip search -----------------------------------------------------------------------------------------------
struct ClipArgs {
  const float* w;
  const float* h;
  int K, N, ldh, bits, asym, n_grid, n_cand;
  int32_t* best;
  float* losses;
  float* w_out;
};

struct ClipCand {
  float lo, hi, s;
  int z;
};

// d of one element under a candidate: Q(clamp(w)) - w, the product rounded before the subtraction
__device__ __forceinline__ float clip_d(const RtnRange& r, int asym, const ClipCand& c, float wv) {
#pragma clang fp contract(off)
  const float v = fminf(fmaxf(wv, c.lo), c.hi);
  const float deq = rtn_deq(r, asym, v, c.s, c.z);
  return deq - wv;
}

template <int GROUP, int R>
__device__ __forceinline__ void clip_fill(float (&d)[GROUP], const RtnRange& r, int asym, const ClipCand& c,
                                          const float* wbase, unsigned n, size_t N, int rows) {
  if constexpr (R < GROUP) {
    d[R] = R < rows ? clip_d(r, asym, c, (wbase + (size_t)R * N)[n]) : 0.f;  // rows is uniform: no load past the weight
    // sixteen loads in flight at a time: without the fence the scheduler requests all GROUP rows before the first
    // division and the kernel needs twice the registers (spills at two waves per SIMD)
    if constexpr (R % 16 == 15) asm volatile("" ::: "memory");
    clip_fill<GROUP, R + 1>(d, r, asym, c, wbase, n, N, rows);
  }
}

// one chunk of G[i][:] . d: 16 columns (four broadcast ds_read_b128), four partial sums
template <int GROUP, int C>
__device__ __forceinline__ void clip_chunk(const float (&d)[GROUP], const float* grow, float (&t)[4]) {
  const float4* p = reinterpret_cast<const float4*>(grow + 16 * C);
  const float4 a = p[0], b = p[1], c = p[2], e = p[3];
  t[0] = fmaf(a.x, d[16 * C + 0], t[0]);
  t[1] = fmaf(a.y, d[16 * C + 1], t[1]);
  t[2] = fmaf(a.z, d[16 * C + 2], t[2]);
  t[3] = fmaf(a.w, d[16 * C + 3], t[3]);
  t[0] = fmaf(b.x, d[16 * C + 4], t[0]);
  t[1] = fmaf(b.y, d[16 * C + 5], t[1]);
  t[2] = fmaf(b.z, d[16 * C + 6], t[2]);
  t[3] = fmaf(b.w, d[16 * C + 7], t[3]);
  t[0] = fmaf(c.x, d[16 * C + 8], t[0]);
  t[1] = fmaf(c.y, d[16 * C + 9], t[1]);
  t[2] = fmaf(c.z, d[16 * C + 10], t[2]);
  t[3] = fmaf(c.w, d[16 * C + 11], t[3]);
  t[0] = fmaf(e.x, d[16 * C + 12], t[0]);
  t[1] = fmaf(e.y, d[16 * C + 13], t[1]);
  t[2] = fmaf(e.z, d[16 * C + 14], t[2]);
  t[3] = fmaf(e.w, d[16 * C + 15], t[3]);
}
// the chunks C .. GROUP / 16 - 1
template <int GROUP, int C>
__device__ __forceinline__ void clip_tail(const float (&d)[GROUP], const float* grow, float (&t)[4]) {
  if constexpr (C < GROUP / 16) {
    clip_chunk<GROUP, C>(d, grow, t);
    clip_tail<GROUP, C + 1>(d, grow, t);
  }
}

// The quadratic form over the rows of chunk RC and the chunks after it. G is symmetric, so
//   d^T G d = sum_i d_i (sum_{k in i's chunk} G_ik d_k + 2 sum_{k in later chunks} G_ik d_k):
// a row reads its own chunk of G (both triangles of the diagonal 16 x 16 block, once each) and the chunks to its right,
// 9 / 16 of the matrix at GROUP 128. The chunk index is a template parameter, so the first chunk a row reads is a
// compile-time constant; the row inside the chunk is a runtime loop. The next row's w is requested before this row's
// dot product, so its latency is covered by the fmas.
template <int GROUP, int ASYM, int RC>
__device__ __forceinline__ void clip_rows(const float (&d)[GROUP], const float* gs, const RtnRange& r, const ClipCand& cd,
                                          const float* wbase, unsigned n, size_t N, int rows, float& e) {
  if constexpr (RC < GROUP / 16) {
    if (16 * RC < rows) {  // uniform
      const int i1 = min(rows, 16 * RC + 16);
      float wv = (wbase + (size_t)(16 * RC) * N)[n];
#pragma unroll 1
      for (int i = 16 * RC; i < i1; ++i) {
        const float wn = (wbase + (size_t)min(i + 1, rows - 1) * N)[n];
        float td[4] = {0.f, 0.f, 0.f, 0.f}, to[4] = {0.f, 0.f, 0.f, 0.f};
        clip_chunk<GROUP, RC>(d, gs + i * GROUP, td);
        clip_tail<GROUP, RC + 1>(d, gs + i * GROUP, to);
        const float di = clip_d(r, ASYM, cd, wv);  // = d[i], see the header
        const float off = (to[0] + to[1]) + (to[2] + to[3]);
        e = fmaf(di, ((td[0] + td[1]) + (td[2] + td[3])) + (off + off), e);
        wv = wn;
      }
      clip_rows<GROUP, ASYM, RC + 1>(d, gs, r, cd, wbase, n, N, rows, e);
    }
  }
}

template <int GROUP, int ASYM>
__global__ __launch_bounds__(AWQ_THREADS, 2) void awq_clip_kernel(const ClipArgs a) {
  __shared__ __attribute__((aligned(16))) float gs[GROUP * GROUP];
  const int g = blockIdx.y, k0 = g * GROUP, rows = min(GROUP, a.K - k0);
  const unsigned n = blockIdx.x * AWQ_THREADS + threadIdx.x;
  const size_t N = (size_t)a.N;

  // the group's diagonal block of h, zero where the group is short
  for (int i = threadIdx.x; i < GROUP * GROUP; i += AWQ_THREADS) {
    const int rr = i / GROUP, cc = i % GROUP;
    gs[i] = (rr < rows && cc < rows) ? a.h[(size_t)(k0 + rr) * (size_t)a.ldh + (size_t)(k0 + cc)] : 0.f;
  }
  __syncthreads();
  if (n >= (unsigned)a.N) return;  // after the only barrier

  const RtnRange r = rtn_range(a.bits);
  // a row's address is a uniform base plus the lane's 32-bit column: the bases live in scalar registers (per-lane
  // 64-bit row addresses, hoisted out of the candidate loop, would take two vector registers a row)
  const float* wbase = a.w + (size_t)k0 * N;
  float mx = wbase[n], mn = mx, amax = fabsf(mx);
  for (int i = 1; i < rows; ++i) {
    const float v = (wbase + (size_t)i * N)[n];
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
    amax = fmaxf(amax, fabsf(v));
  }
  const float hi0 = fmaxf(mx, 0.f), lo0 = fminf(mn, 0.f);

  const size_t cell = (size_t)g * N + n, plane = (size_t)gridDim.y * N;
  float best_e = 0.f, best_lo = 0.f, best_hi = 0.f;
  int best_j = 0;
#pragma unroll 1
  for (int j = 0; j < a.n_cand; ++j) {
    // the bounds: the double product rounded once; the clamped group's RTN range is exactly [lo, hi] (the element
    // that set the range is clamped onto the bound), so the candidate's parameters follow from the bounds
    const double c = 1.0 - (double)j / (double)a.n_grid;
    ClipCand cd;
    if constexpr (!ASYM) {
      cd.hi = (float)(c * (double)amax);
      cd.lo = -cd.hi;
      rtn_params(r, 0, cd.hi, cd.lo, cd.hi, cd.s, cd.z);
    } else {
      cd.hi = (float)(c * (double)hi0);
      cd.lo = (float)(c * (double)lo0);
      rtn_params(r, 1, cd.hi, cd.lo, 0.f, cd.s, cd.z);
    }
    // n and rows as this iteration's own values: otherwise every row's 64-bit address and every `R < rows` is
    // hoisted out of the candidate loop, two vector and two scalar registers a row, and the kernel spills
    unsigned nj = n;
    int rj = rows;
    asm volatile("" : "+v"(nj), "+s"(rj));
    float d[GROUP];
    clip_fill<GROUP, 0>(d, r, ASYM, cd, wbase, nj, N, rj);
    float e = 0.f;
    clip_rows<GROUP, ASYM, 0>(d, gs, r, cd, wbase, nj, N, rj, e);
    a.losses[(size_t)j * plane + cell] = e;
    if (j == 0 || e < best_e) best_e = e, best_j = j, best_lo = cd.lo, best_hi = cd.hi;
  }
  a.best[cell] = best_j;
  float* obase = a.w_out + (size_t)k0 * N;
  for (int i = 0; i < rows; ++i)
    (obase + (size_t)i * N)[n] = fminf(fmaxf((wbase + (size_t)i * N)[n], best_lo), best_hi);
}

template <int GROUP>
void launch_clip(const ClipArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + AWQ_THREADS - 1) / AWQ_THREADS), (unsigned)((a.K + GROUP - 1) / GROUP));
  if (a.asym)
    hipLaunchKernelGGL((awq_clip_kernel<GROUP, 1>), grid, dim3(AWQ_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((awq_clip_kernel<GROUP, 0>), grid, dim3(AWQ_THREADS), 0, st, a);
}

}  // namespace
}  // namespace woq

extern "C" int woq_awq_scale_delta(const float* w_dev, const float* s_dev, int K, int N, int group, int bits, int asym,
                                   float* d_out_dev, void* stream) {
  WOQ_TRY
  WOQ_CHECK(w_dev && s_dev && d_out_dev, "QBits: awq_scale_delta: null tensor");
  woq::GroupColsPlan p;  // the one-slice form: 256 columns of one group per workgroup
  if (const char* why = woq::group_cols_plan(K, N, group, bits, p, false))
    WOQ_FAIL(std::string("QBits: awq_scale_delta: ") + why);
  hipLaunchKernelGGL(woq::awq_scale_delta_kernel, p.grid, p.block, 0, (hipStream_t)stream, w_dev, s_dev, K, N, p.group,
                     bits, asym ? 1 : 0, d_out_dev);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

extern "C" int woq_awq_clip_search(const float* w_dev, const float* h_dev, int ldh, int K, int N, int group, int bits,
                                   int asym, int n_grid, int n_cand, int32_t* best_dev, float* losses_dev,
                                   float* w_out_dev, void* stream) {
  WOQ_TRY
  WOQ_CHECK(w_dev && h_dev && best_dev && losses_dev && w_out_dev, "QBits: awq_clip_search: null tensor");
  WOQ_CHECK(K >= 1 && N >= 1 && ldh >= K, "QBits: awq_clip_search: bad shape (h is [K, K] with a row stride >= K)");
  WOQ_CHECK(woq::rtn_bits_ok(bits), "QBits: awq_clip_search: bits must be 2, 3, 4 or 8");
  WOQ_CHECK(group == 32 || group == 64 || group == 128,
            "QBits: awq_clip_search: group must be 32, 64 or 128 (the Gram block of a group lives in LDS)");
  WOQ_CHECK(n_grid >= 1 && n_cand >= 1 && n_cand <= n_grid,
            "QBits: awq_clip_search: needs 1 <= n_cand <= n_grid (every candidate keeps a positive range)");
  // group stays as given: with K < group the one short group still runs in its own kernel form
  WOQ_CHECK(woq::rtn_group_count(K, group), "QBits: awq_clip_search: more than 65535 groups");
  const woq::ClipArgs a = {w_dev, h_dev, K, N, ldh, bits, asym ? 1 : 0, n_grid, n_cand, best_dev, losses_dev, w_out_dev};
  if (group == 128)
    woq::launch_clip<128>(a, (hipStream_t)stream);
  else if (group == 64)
    woq::launch_clip<64>(a, (hipStream_t)stream);
  else
    woq::launch_clip<32>(a, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}
