// woq_teq.hip — the quantiser of TEQ calibration (Cheng et al. 2023, "TEQ: Trainable Equivalent Transformation for
// Quantization of LLMs"): the fake-quantised weight under a trainable per-input-channel scale a [K], and the gradient
// of the loss with respect to that scale. tests/teq_reference.py is the float64 statement,
// transformers/llm/quantization/teq.py the driver.
//
//   w      fp32 [K, N] row-major, row k = input feature k (Linear.weight.T)        a  fp32 [K], positive
//   group  `group` consecutive k of one column (the last may be short)
//
//   u = w[k,n] a[k]        (s, z) = rtn_params of the group's u        deq = rtn_quant(u)        W~ = deq / a[k]
//
// the package's RTN rule (woq_rtn.h) applied to u, every step rounded on its own (no contraction): a = 1 gives RTN's
// bits.
//
// Gradient, rne straight-through, clip passing inside its range (bounds included), max / min passing to the one row
// that attains them (the first in row order), g = dL/dW~, ga = g / a[k], un = "the code was not clipped", t = u / s:
//   direct[k,n] = g (un ? w / a : 0) - g deq / a^2
//   sym    DS = sum_k ga (un ? c - t : c);      E = DS sign(u*) w[k*,n] / qmax on row k* = argmax |u|
//   asym   DS = sum_k ga (un ? q - t : q + zf), DLO = sum_k (un ? 0 : ga), q = c - z, zf = -lo / s
//          Ehi = (DS / L) w[kmax,n] on row kmax where max u > 0
//          Elo = (DLO - DS / L) w[kmin,n] on row kmin where min u < 0
//   da[k]  = sum_n direct[k,n] + the E terms that land on row k;   a group whose s was replaced by 1 has no E
//
// Layout: woq_group_cols.h. The slices' ranges are exact (min, max and, for the gradient, the first row that attains
// them: slice order is row order and the comparison is strict); DS and DLO are the two sums that meet in slice order.
//
// The reduction over the columns has no floating-point atomics and an order the layout fixes: a wave is 64 columns
// ("column block") of some rows of one group. Per row it sums direct over its lanes with a fixed xor butterfly; lane j
// keeps the sum of the wave's j-th row (mod 64) and the wave stores 64 rows at a time to partial[column block][k]. When
// DS is complete, slice 0 leaves each column's E and its row in LDS; every wave then walks its own rows again, lane j
// adding to the row it stored, in column order, the E terms that name it (a read-modify-write of a word that same
// lane wrote). A second, small launch adds partial[.][k] in column-block order. Two runs give the same bytes.
// partial is K * ceil(N / 64) floats from the launcher's scratch: 1 MiB for a 4096 x 4096 linear.
//
// fp32 VALU throughout. The forward reads w twice (the second time from L2) and writes W~, 6 - 8 B per weight from HBM,
// and divides twice per element, as the rule says; the gradient reads w twice and g once, 6 - 8 B per weight, and
// divides once per element (t) and once per row (1 / a, uniform over the wave). Measured at the Llama-2-7B shapes,
// group 128, bf16 W~ and g (profiles/r18_teq.txt): forward 42 - 193 us, 2.3 - 3.1 TB/s counted on 6 B per weight;
// gradient 76 - 344 us, 1.2 - 1.7 TB/s: it is bound by instruction issue, not by memory (per row and wave the six
// butterfly steps, each a cross-lane read and an add, beside some forty VALU instructions per element row). Requesting
// four rows' loads ahead of the arithmetic was measured 15 - 25 % slower (65 VGPRs, seven waves) and is not kept; a
// reduce-scatter butterfly over several rows at once would cut the cross-lane steps about fivefold and is open.
// Registers (tools/kres.py), 1 / 4 / 16 slices: forward 20 / 34 / 55 VGPRs, gradient 44 / 49 / 49, the final sum 15;
// 0 / 3 / 12 KiB LDS forward, 4 / 7 / 25 KiB gradient; eight waves per SIMD, no AGPRs, no scratch, no spills.
#include "woq_device.h"
#include "woq_group_cols.h"

namespace woq {
namespace {

constexpr int TEQ_WAVE = 64;  // a column block: the width of the row sum's butterfly
static_assert(GC_SPLIT_COLS == TEQ_WAVE && GC_THREADS % TEQ_WAVE == 0, "a wave is one column block of one slice");

enum { TEQ_FORWARD = 0, TEQ_GRAD = 1 };

struct TeqArgs {
  const float* w;
  const float* a;
  int K, N, group, bits, asym;
  // forward
  void* out;
  int out_dt;
  // gradient
  const void* g;
  int g_dt;
  float* partial;  // [ceil(N / 64)][K]
};

__device__ __forceinline__ float teq_wave_sum(float x) {
#pragma clang fp contract(off)
  for (int o = TEQ_WAVE / 2; o; o >>= 1) x = x + __shfl_xor(x, o, TEQ_WAVE);  // every lane ends with the same bits
  return x;
}

template <int MODE, int SLICES>
__global__ __launch_bounds__(GroupCols<SLICES>::THREADS) void teq_kernel(const TeqArgs a) {
#pragma clang fp contract(off)
  using GC = GroupCols<SLICES>;
  constexpr int COLS = GC::COLS;
  constexpr bool GRAD = MODE == TEQ_GRAD;
  __shared__ float red[SLICES == 1 ? 1 : 3 * SLICES * COLS];
  __shared__ int redk[(SLICES == 1 || !GRAD) ? 1 : 3 * SLICES * COLS];
  __shared__ float ent_e[GRAD ? 2 * COLS : 1];
  __shared__ int ent_k[GRAD ? 2 * COLS : 1];
  const int n = GC::column();
  const int lane = threadIdx.x & (TEQ_WAVE - 1);
  const int slice = GC::slice();
  const bool valid = n < a.N;
  const bool wave_live = n - lane < a.N;  // the wave's column block exists
  if (!GRAD && SLICES == 1 && !valid) return;  // no barrier and no cross-lane sum on this path
  const size_t N = (size_t)a.N;
  const GC gc(a.K, a.group, slice);
  const int r0 = gc.r0, r1 = gc.r1;

  // the range of u: 0 belongs to it, so an empty slice is neutral; a row index stays -1 where nothing exceeds 0
  float mn = 0.f, mx = 0.f, amax = 0.f;
  int kmn = -1, kmx = -1, kam = -1;
  if (valid)
#pragma unroll 4
    for (int k = r0; k < r1; ++k) {
      const float u = a.w[(size_t)k * N + n] * a.a[k];
      const float au = fabsf(u);
      if (u > mx) mx = u, kmx = k;
      if (u < mn) mn = u, kmn = k;
      if (au > amax) amax = au, kam = k;
    }
  if constexpr (SLICES > 1) {
    red[slice * COLS + threadIdx.x] = mn;
    red[(SLICES + slice) * COLS + threadIdx.x] = mx;
    red[(2 * SLICES + slice) * COLS + threadIdx.x] = amax;
    if constexpr (GRAD) {
      redk[slice * COLS + threadIdx.x] = kmn;
      redk[(SLICES + slice) * COLS + threadIdx.x] = kmx;
      redk[(2 * SLICES + slice) * COLS + threadIdx.x] = kam;
    }
    __syncthreads();
    mn = mx = amax = 0.f;
    kmn = kmx = kam = -1;
    for (int i = 0; i < SLICES; ++i) {  // slice order = row order: a strict comparison keeps the first row
      const float smn = red[i * COLS + threadIdx.x], smx = red[(SLICES + i) * COLS + threadIdx.x];
      const float sam = red[(2 * SLICES + i) * COLS + threadIdx.x];
      if (smx > mx) {
        mx = smx;
        if constexpr (GRAD) kmx = redk[(SLICES + i) * COLS + threadIdx.x];
      }
      if (smn < mn) {
        mn = smn;
        if constexpr (GRAD) kmn = redk[i * COLS + threadIdx.x];
      }
      if (sam > amax) {
        amax = sam;
        if constexpr (GRAD) kam = redk[(2 * SLICES + i) * COLS + threadIdx.x];
      }
    }
    __syncthreads();  // red is reused for the partial sums
  }

  const RtnRange r = rtn_range(a.bits);
  float s;
  int z;
  const bool dead = rtn_params(r, a.asym, mx, mn, amax, s, z);  // no gradient through a step that is not s

  if constexpr (!GRAD) {
    if (valid)
#pragma unroll 4
      for (int k = r0; k < r1; ++k) {
        const size_t i = (size_t)k * N + n;
        const float ak = a.a[k];
        const float u = a.w[i] * ak;
        store_f32(a.out, i, a.out_dt, rtn_deq(r, a.asym, u, s, z) / ak);
      }
  } else {
    const float zf = a.asym ? -fminf(mn, 0.f) / s : 0.f;
    const float cmin = a.asym ? 0.f : (float)-r.off, cmax = a.asym ? (float)r.levels : (float)r.qmax;
    const int cb = (n - lane) / TEQ_WAVE;
    float* part = a.partial + (size_t)cb * (size_t)a.K;

    float ds = 0.f, dlo = 0.f, keep = 0.f;
    for (int k = r0; k < r1; ++k) {  // uniform over the wave: the row sum needs every lane
      const size_t i = (size_t)k * N + n;
      const float ak = a.a[k];
      const float inv = 1.f / ak;
      float direct = 0.f;
      if (valid) {
        const float wk = a.w[i], gk = load_f32(a.g, i, a.g_dt);
        const float u = wk * ak;
        const float t = u / s;
        int code;
        float deq;
        rtn_quant(r, a.asym, u, s, z, code, deq);
        const float rz = rintf(t) + (float)z;
        const bool un = rz >= cmin && rz <= cmax;
        const float qf = (float)(a.asym ? code + r.off - z : code);
        const float ga = gk * inv;
        direct = gk * (un ? wk * inv : 0.f) - ga * (deq * inv);
        if (un) {
          ds = ds + ga * (qf - t);
        } else {
          ds = ds + ga * (qf + zf);
          dlo = dlo + ga;
        }
      }
      const float tot = teq_wave_sum(direct);
      const int j = (k - r0) & (TEQ_WAVE - 1);
      if (lane == j) keep = tot;
      if ((j == TEQ_WAVE - 1 || k == r1 - 1) && wave_live && lane <= j) part[k - j + lane] = keep;
    }

    GC::leave_sums(red, slice, ds, dlo);
    if (slice == 0) {
      const float2 sums = GC::take_sums(red, ds, dlo);
      ds = sums.x, dlo = sums.y;
      float e0 = 0.f, e1 = 0.f;
      int ka = -1, kb = -1;
      if (valid && !dead) {
        if (a.asym) {
          const float dhi = ds / (float)r.levels;
          if (kmx >= 0) ka = kmx, e0 = dhi * a.w[(size_t)kmx * N + n];
          if (kmn >= 0) kb = kmn, e1 = (dlo - dhi) * a.w[(size_t)kmn * N + n];
        } else if (kam >= 0) {
          const float wk = a.w[(size_t)kam * N + n];
          const float u = wk * a.a[kam];
          ka = kam, e0 = ds * (u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f)) * wk / (float)r.qmax;
        }
      }
      ent_k[threadIdx.x] = ka, ent_e[threadIdx.x] = e0;
      ent_k[COLS + threadIdx.x] = kb, ent_e[COLS + threadIdx.x] = e1;
    }
    __syncthreads();
    if (!wave_live) return;
    // the E terms of this column block, onto the rows this wave stored: lane j owns row c0 + j, as above
    const int ebase = threadIdx.x - lane;  // 0 in the split forms
    for (int c0 = r0; c0 < r1; c0 += TEQ_WAVE) {
      const int row = c0 + lane;
      float acc = 0.f;
      bool hit = false;
      for (int e = 0; e < TEQ_WAVE; ++e) {  // column order; LDS broadcast reads
        if (ent_k[ebase + e] == row) acc = acc + ent_e[ebase + e], hit = true;
        if (a.asym && ent_k[COLS + ebase + e] == row) acc = acc + ent_e[COLS + ebase + e], hit = true;
      }
      if (hit && row < r1) part[row] = part[row] + acc;
    }
  }
}

// da[k] = sum of partial[cb][k] in column-block order
__global__ __launch_bounds__(GC_THREADS) void teq_sum_kernel(const float* __restrict__ partial, int n_blocks, int K,
                                                             float* __restrict__ da) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * GC_THREADS + threadIdx.x;
  if (k >= K) return;
  float acc = 0.f;
#pragma unroll 4
  for (int cb = 0; cb < n_blocks; ++cb) acc = acc + partial[(size_t)cb * (size_t)K + k];
  da[k] = acc;
}

template <int MODE>
void teq_run(const TeqArgs& a, const GroupColsPlan& p, hipStream_t st) {
  group_cols_dispatch(p.slices, [&](auto slices) {
    hipLaunchKernelGGL((teq_kernel<MODE, decltype(slices)::value>), p.grid, p.block, 0, st, a);
  });
}

}  // namespace
}  // namespace woq

extern "C" int woq_teq_forward(const float* w_dev, const float* a_dev, int K, int N, int group, int bits, int asym,
                               void* out_dev, int out_dtype, void* stream) {
  WOQ_TRY
  WOQ_CHECK(w_dev && a_dev && out_dev, "QBits: teq_forward: null tensor");
  WOQ_CHECK(woq::fake_quant_dtype_ok(out_dtype), "QBits: teq_forward: the output is fp32, fp16 or bf16");
  woq::GroupColsPlan p;
  if (const char* why = woq::group_cols_plan(K, N, group, bits, p)) WOQ_FAIL(std::string("QBits: teq_forward: ") + why);
  woq::TeqArgs a = {};
  a.w = w_dev, a.a = a_dev;
  a.K = K, a.N = N, a.group = p.group, a.bits = bits, a.asym = asym ? 1 : 0;
  a.out = out_dev, a.out_dt = out_dtype;
  woq::teq_run<woq::TEQ_FORWARD>(a, p, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

extern "C" int woq_teq_grad(const float* w_dev, const float* a_dev, const void* g_dev, int g_dtype, int K, int N,
                            int group, int bits, int asym, float* da_dev, void* stream) {
  WOQ_TRY
  WOQ_CHECK(w_dev && a_dev && g_dev && da_dev, "QBits: teq_grad: null tensor");
  WOQ_CHECK(woq::fake_quant_dtype_ok(g_dtype), "QBits: teq_grad: the gradient is fp32, fp16 or bf16");
  woq::GroupColsPlan p;
  if (const char* why = woq::group_cols_plan(K, N, group, bits, p)) WOQ_FAIL(std::string("QBits: teq_grad: ") + why);
  woq::TeqArgs a = {};
  a.w = w_dev, a.a = a_dev;
  a.K = K, a.N = N, a.group = p.group, a.bits = bits, a.asym = asym ? 1 : 0;
  a.g = g_dev, a.g_dt = g_dtype;
  hipStream_t st = (hipStream_t)stream;
  const int n_blocks = (N + woq::TEQ_WAVE - 1) / woq::TEQ_WAVE;
  const size_t bytes = (size_t)n_blocks * (size_t)K * sizeof(float);
  bool own = false;
  a.partial = (float*)woq::scratch_take(bytes, st, &own);
  WOQ_CHECK(a.partial != nullptr, "QBits: teq_grad: scratch allocation failed");
  woq::teq_run<woq::TEQ_GRAD>(a, p, st);
  hipLaunchKernelGGL(woq::teq_sum_kernel, dim3((unsigned)((K + woq::GC_THREADS - 1) / woq::GC_THREADS)),
                     dim3(woq::GC_THREADS), 0, st, a.partial, n_blocks, K, da_dev);
  const hipError_t e = hipGetLastError();
  woq::scratch_release(a.partial, bytes, own, st);
  WOQ_HIP(e);
  WOQ_END
}
