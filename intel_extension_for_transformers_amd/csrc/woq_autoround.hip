// woq_autoround.hip — the quantiser of AutoRound calibration (Cheng et al. 2023, "Optimize Weight Rounding via Signed
// Gradient Descent"): its forward, its backward fused with the SignSGD update, and the final codes.
// tests/autoround_reference.py is the float64 statement, transformers/llm/quantization/autoround.py the driver.
//
//   w      fp32 [K, N] row-major, row k = input feature k (Linear.weight.T)
//   V      fp32 [K, N] in [-0.5, 0.5], the rounding offset         alpha, beta  fp32 [G, N] in [0, 1], the range factors
//   group  `group` consecutive k of one column (the last may be short); mn = min(min v, 0), mx = max(max v, 0)
//
//   asym   lo = alpha mn, hi = beta mx, s = (hi - lo) / L (0 -> 1), z = clip(rne(-lo / s), 0, L)
//          t = w / s + V, c = clip(rne(t) + z, 0, L), W~ = (c - z) s
//   sym    amax = beta mx >= alpha (-mn) ? beta mx : alpha (-mn), s = amax / qmax (0 -> 1)
//          t = w / s + V, c = clip(rne(t), -off, qmax), W~ = c s
//
// the package's RTN rule (woq_rtn.h, whose rtn_range this file takes) with V, alpha and beta put in, in that rule's fp32
// expression order, every step rounded on its own (no contraction): V = 0, alpha = beta = 1 gives RTN's bits. The
// codes are clamped as floats before the conversion to int (the same values wherever RTN's int arithmetic does not
// overflow; a tiny alpha makes w / s large).
//
// Gradients, rne straight-through, clip passing inside its range (bounds included), g = dL/dW~, q = c - z (asym) | c:
//   an element whose code was not clipped   dV = g s (only its sign is used: sign(g), s > 0), ds += g (q - w / s)
//   a clipped element                       dV = 0, asym: ds += g (q - lo / s), dlo += g; sym: ds += g c
//   asym   dhi = ds / L, dlo -= ds / L, dalpha = dlo mn, dbeta = dhi mx
//   sym    damax = ds / qmax, to beta (times mx) where beta mx >= alpha (-mn), else to alpha (times -mn)
//   a group whose s was replaced by 1 gives alpha and beta no gradient
// Step: p <- clamp(p - lr sign(grad)), sign(0) = 0; V in [-0.5, 0.5], alpha / beta in [0, 1]. dV is never stored.
//
// Layout: woq_group_cols.h. The slices' ranges are exact (min and max); ds and dlo are the two sums that meet in slice
// order. Both row loops are unrolled by four for loads in flight. fp32 VALU throughout. Memory bound: the forward reads
// w twice (the second time from L2: a workgroup's group is 32 KiB at group 128) and V once and writes W~, 10 B per
// weight from HBM with a 16-bit output; the step reads w, V and g and writes V, 14 - 16 B per weight. Measured at the
// Llama-2-7B shapes (profiles/r17_autoround.txt): forward 3.7 - 4.0 TB/s, step 4.1 - 4.5 TB/s, half of the 8 TB/s peak.
// Registers (tools/kres.py), 1 / 4 / 16 slices: forward 25 / 32 / 32 VGPRs, step 48 / 52 / 52, codes 33 / 39 / 39;
// 0 / 2 / 8 KiB LDS; eight waves per SIMD, no AGPRs, no scratch, no spills. The only fmas in the code are those of the
// divisions.
#include "woq_device.h"
#include "woq_group_cols.h"

namespace woq {
namespace {

enum { AR_FORWARD = 0, AR_STEP = 1, AR_CODES = 2 };

struct ArArgs {
  const float* w;
  float* v;      // read; written by the step
  float* alpha;  // read; written by the step
  float* beta;
  int K, N, group, bits, asym;
  // forward
  void* out;
  int out_dt;
  // step
  const void* g;
  int g_dt;
  float lr_v, lr_mm;
  float* dalpha;  // nullable: the raw gradients
  float* dbeta;
  // codes
  int8_t* q;
  float* scale;
  int8_t* zp;  // nullable (sym)
};

__device__ __forceinline__ float ar_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

template <int MODE, int SLICES>
__global__ __launch_bounds__(GroupCols<SLICES>::THREADS) void autoround_kernel(const ArArgs a) {
#pragma clang fp contract(off)
  using GC = GroupCols<SLICES>;
  constexpr int COLS = GC::COLS;
  __shared__ float red[SLICES == 1 ? 1 : 2 * SLICES * COLS];
  const int n = GC::column();
  const int slice = GC::slice();
  const bool valid = n < a.N;
  if (SLICES == 1 && !valid) return;  // no barrier on this path
  const size_t N = (size_t)a.N;
  const GC gc(a.K, a.group, slice);
  const int r0 = gc.r0, r1 = gc.r1;
  const size_t cell = (size_t)blockIdx.y * N + (size_t)n;

  // the range: 0 belongs to it, so an empty slice is neutral
  float mn = 0.f, mx = 0.f;
  if (valid)
#pragma unroll 4
    for (int k = r0; k < r1; ++k) {
      const float v = a.w[(size_t)k * N + n];
      mx = fmaxf(mx, v);
      mn = fminf(mn, v);
    }
  if constexpr (SLICES > 1) {
    red[slice * COLS + threadIdx.x] = mn;
    red[(SLICES + slice) * COLS + threadIdx.x] = mx;
    __syncthreads();
    for (int i = 0; i < SLICES; ++i) {
      mn = fminf(mn, red[i * COLS + threadIdx.x]);
      mx = fmaxf(mx, red[(SLICES + i) * COLS + threadIdx.x]);
    }
    __syncthreads();  // red is reused for the partial sums
  }

  const auto [qmax, levels, off] = rtn_range(a.bits);
  const float al = valid ? a.alpha[cell] : 1.f, be = valid ? a.beta[cell] : 1.f;
  float s, lo = 0.f, cmin, cmax;
  int zi = 0;
  bool beta_side = false;
  if (a.asym) {
    lo = al * mn;
    const float hi = be * mx;
    s = (hi - lo) / (float)levels;
    cmin = 0.f;
    cmax = (float)levels;
  } else {
    const float pa = be * mx, pb = al * (-mn);
    beta_side = pa >= pb;
    s = (beta_side ? pa : pb) / (float)qmax;
    cmin = (float)-off;
    cmax = (float)qmax;
  }
  const bool replaced = s == 0.f;
  if (replaced) s = 1.f;
  float los = 0.f;  // lo / s: where a clipped element's code sits, in steps
  if (a.asym) {
    zi = (int)fminf(fmaxf(rintf(-lo / s), 0.f), (float)levels);
    los = lo / s;
  }
  const float zf = (float)zi;

  float ds = 0.f, dlo = 0.f;
  if (valid)
#pragma unroll 4
    for (int k = r0; k < r1; ++k) {
      const size_t i = (size_t)k * N + n;
      const float wk = a.w[i], vk = a.v[i];
      const float wd = wk / s;
      const float t = wd + vk;
      const float rz = rintf(t) + zf;  // exact below 2^24, and clipped either way beyond
      const int qi = (int)fminf(fmaxf(rz, cmin), cmax) - zi;
      if constexpr (MODE == AR_FORWARD) {
        store_f32(a.out, i, a.out_dt, (float)qi * s);
      } else if constexpr (MODE == AR_CODES) {
        a.q[i] = (int8_t)(a.asym ? qi + zi - off : qi);
      } else {
        const float gk = load_f32(a.g, i, a.g_dt);
        const bool clipped = rz < cmin || rz > cmax;
        const float qf = (float)qi;
        if (!clipped) {
          ds = ds + gk * (qf - wd);
          a.v[i] = fminf(fmaxf(vk - a.lr_v * ar_sign(gk), -0.5f), 0.5f);
        } else if (a.asym) {
          ds = ds + gk * (qf - los);
          dlo = dlo + gk;
        } else {
          ds = ds + gk * qf;
        }
      }
    }

  if constexpr (MODE == AR_CODES) {
    if (valid && slice == 0) {
      a.scale[cell] = s;
      if (a.asym && a.zp) a.zp[cell] = (int8_t)(zi - off);
    }
  }
  if constexpr (MODE == AR_STEP) {
    GC::leave_sums(red, slice, ds, dlo);
    if (slice != 0) return;
    const float2 sums = GC::take_sums(red, ds, dlo);
    ds = sums.x, dlo = sums.y;
    if (!valid) return;
    float da = 0.f, db = 0.f;
    if (!replaced) {
      if (a.asym) {
        const float dhi = ds / (float)levels;
        da = (dlo - dhi) * mn;
        db = dhi * mx;
      } else {
        const float dm = ds / (float)qmax;
        if (beta_side)
          db = dm * mx;
        else
          da = dm * (-mn);
      }
    }
    if (a.dalpha) a.dalpha[cell] = da;
    if (a.dbeta) a.dbeta[cell] = db;
    a.alpha[cell] = fminf(fmaxf(al - a.lr_mm * ar_sign(da), 0.f), 1.f);
    a.beta[cell] = fminf(fmaxf(be - a.lr_mm * ar_sign(db), 0.f), 1.f);
  }
}

template <int MODE>
void ar_run(const ArArgs& a, const GroupColsPlan& p, hipStream_t st) {
  group_cols_dispatch(p.slices, [&](auto slices) {
    hipLaunchKernelGGL((autoround_kernel<MODE, decltype(slices)::value>), p.grid, p.block, 0, st, a);
  });
}

}  // namespace
}  // namespace woq

extern "C" int woq_autoround_forward(const float* w_dev, const float* v_dev, const float* alpha_dev,
                                     const float* beta_dev, int K, int N, int group, int bits, int asym, void* out_dev,
                                     int out_dtype, void* stream) {
  WOQ_TRY
  WOQ_CHECK(w_dev && v_dev && alpha_dev && beta_dev && out_dev, "QBits: autoround_forward: null tensor");
  WOQ_CHECK(woq::fake_quant_dtype_ok(out_dtype), "QBits: autoround_forward: the output is fp32, fp16 or bf16");
  woq::GroupColsPlan p;
  if (const char* why = woq::group_cols_plan(K, N, group, bits, p))
    WOQ_FAIL(std::string("QBits: autoround_forward: ") + why);
  woq::ArArgs a = {};
  a.w = w_dev, a.v = const_cast<float*>(v_dev), a.alpha = const_cast<float*>(alpha_dev);
  a.beta = const_cast<float*>(beta_dev);
  a.K = K, a.N = N, a.group = p.group, a.bits = bits, a.asym = asym ? 1 : 0;
  a.out = out_dev, a.out_dt = out_dtype;
  woq::ar_run<woq::AR_FORWARD>(a, p, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

extern "C" int woq_autoround_step(const float* w_dev, float* v_dev, float* alpha_dev, float* beta_dev, const void* g_dev,
                                  int g_dtype, int K, int N, int group, int bits, int asym, float lr_v, float lr_minmax,
                                  float* dalpha_out_dev, float* dbeta_out_dev, void* stream) {
  WOQ_TRY
  WOQ_CHECK(w_dev && v_dev && alpha_dev && beta_dev && g_dev, "QBits: autoround_step: null tensor");
  WOQ_CHECK(woq::fake_quant_dtype_ok(g_dtype), "QBits: autoround_step: the gradient is fp32, fp16 or bf16");
  WOQ_CHECK(lr_v >= 0.f && lr_minmax >= 0.f, "QBits: autoround_step: a learning rate is negative or not a number");
  woq::GroupColsPlan p;
  if (const char* why = woq::group_cols_plan(K, N, group, bits, p))
    WOQ_FAIL(std::string("QBits: autoround_step: ") + why);
  woq::ArArgs a = {};
  a.w = w_dev, a.v = v_dev, a.alpha = alpha_dev, a.beta = beta_dev;
  a.K = K, a.N = N, a.group = p.group, a.bits = bits, a.asym = asym ? 1 : 0;
  a.g = g_dev, a.g_dt = g_dtype, a.lr_v = lr_v, a.lr_mm = lr_minmax;
  a.dalpha = dalpha_out_dev, a.dbeta = dbeta_out_dev;
  woq::ar_run<woq::AR_STEP>(a, p, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

extern "C" int woq_autoround_codes(const float* w_dev, const float* v_dev, const float* alpha_dev, const float* beta_dev,
                                   int K, int N, int group, int bits, int asym, int8_t* q_dev, float* scale_dev,
                                   int8_t* zp_dev, void* stream) {
  WOQ_TRY
  WOQ_CHECK(w_dev && v_dev && alpha_dev && beta_dev && q_dev && scale_dev, "QBits: autoround_codes: null tensor");
  WOQ_CHECK(!asym || zp_dev, "QBits: autoround_codes: asym needs a zero-point tensor");
  woq::GroupColsPlan p;
  if (const char* why = woq::group_cols_plan(K, N, group, bits, p))
    WOQ_FAIL(std::string("QBits: autoround_codes: ") + why);
  woq::ArArgs a = {};
  a.w = w_dev, a.v = const_cast<float*>(v_dev), a.alpha = const_cast<float*>(alpha_dev);
  a.beta = const_cast<float*>(beta_dev);
  a.K = K, a.N = N, a.group = p.group, a.bits = bits, a.asym = asym ? 1 : 0;
  a.q = q_dev, a.scale = scale_dev, a.zp = zp_dev;
  woq::ar_run<woq::AR_CODES>(a, p, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}
