// woq_gptq.hip — the sequential part of GPTQ calibration (Frantar et al. 2022, "fasterquant" of AutoGPTQ): one launch
// sweeps one block of up to 128 consecutive input features of a weight in working order.
//
//   w  fp32 [K, N] row-major, row k = input feature k (Linear.weight.T), modified in place
//   u  fp32 [K, K] row-major, upper triangular, H^-1 = U^T U (the upper Cholesky factor of the inverse Hessian)
//
// For every column n on its own, j ascending over c0 <= j < c0 + B:
//   gid = col_group ? col_group[j] : j / group
//   at a group start (j % group == 0, parameters not given): (s, z) = the RTN parameters (woq_rtn.h, rtn_kernel's rule;
//     tests/quant_reference.py) of the CURRENT w[j .. min(j + group, K) - 1][n] — rows of this block as
//     updated so far, rows beyond it as they stand in memory — stored to scale[gid][n], zp[gid][n]
//   code = that rule's code of w[j][n], q[j][n] = code (the signed domain woq_repack_quantized_weight takes)
//   d = its dequantised value (one fp32 product), e = (w[j][n] - d) / u[j][j] (an fp32 subtraction and a correctly
//     rounded fp32 division), err[j - c0][n] = e
//   w[k][n] = fma(-e, u[j][k], w[k][n]) for k in j + 1 .. c0 + B - 1: FUSED, one rounding per update
//   w[j][n] = d
// The rows after the block are the caller's: w[c0 + B:] -= u[c0 : c0 + B, c0 + B:]^T err, one GEMM.
//
// State layout. The columns are independent, the rows of one column are a chain: one thread owns column n and keeps the
// block's 128 rows in registers, wr[0 .. 127], every index a compile-time constant (the j and k loops are unrolled in
// full by template recursion, so the sweep is straight-line code of about 9k fmas). Loads and stores of a row are
// coalesced over n. U's block is the same for every lane: the workgroup stages it once in LDS (64 KiB, zero where the
// block is short) and the update reads it at constant offsets — every lane the same address, a broadcast, in chunks of
// 16 columns (four ds_read_b128) requested two chunks ahead of the fmas that use them. Workgroups are one wave of 64
// columns, so N = 4096 is 64 waves: a launch uses a fraction of the chip and its time is the chain's length, not a
// rate: 160 - 177 us per launch at the Llama-2-7B shapes, 32 - 37 times faster than the same loop in torch
// (profiles/r13_gptq.txt). Spending four lanes per column on the update would shorten the chain; that form has not
// been built or measured (named as open in the same file).
// Registers: 248 (128 for the state, three chunks of U, the step's temporaries); no scratch (tools/kres.py).
//
// Group starts are found at j = 0, 32, 64, 96 of the block only: the launcher asks for c0 and the group size to be
// multiples of 32 (or one group per column) when it has to compute parameters, which is what the package's blob takes.
#include "woq_device.h"
#include "woq_launch.h"
#include "woq_rtn.h"

namespace woq {
namespace {

constexpr int GPTQ_BLOCK = 128;  // rows one launch sweeps at most = the registers a thread keeps
constexpr int GPTQ_THREADS = 64;

struct GptqArgs {
  float* w;
  const float* u;
  int K, N, c0, B, group, bits, asym, params_given;
  const int32_t* col_group;
  int8_t* q;
  float* scale;
  int8_t* zp;
  float* err;
};

// The loops over the state are unrolled by recursion on a template index: every wr[] index is then a constant and the
// array lives in registers (a `#pragma unroll` of 128 x 128 is refused by the optimizer, and the state goes to scratch).
//
// One row of U is read from LDS in chunks of 16 columns (four ds_read_b128, every lane the same address), two chunks
// ahead of the fmas that use them: the first two before the step's divisions, chunk c + 2 before the fmas of chunk c.
struct UChunk {
  float4 v[4];
};
template <int C>
__device__ __forceinline__ void gptq_uread(UChunk& r, const float* urow) {
  if constexpr (C < GPTQ_BLOCK / 16) {
    const float4* p = reinterpret_cast<const float4*>(urow + 16 * C);
    r.v[0] = p[0], r.v[1] = p[1], r.v[2] = p[2], r.v[3] = p[3];
  }
}
#define GPTQ_FMA4(i) \
  wr[16 * C + 4 * i + 0] = fmaf(-e, ua.v[i].x, wr[16 * C + 4 * i + 0]); \
  wr[16 * C + 4 * i + 1] = fmaf(-e, ua.v[i].y, wr[16 * C + 4 * i + 1]); \
  wr[16 * C + 4 * i + 2] = fmaf(-e, ua.v[i].z, wr[16 * C + 4 * i + 2]); \
  wr[16 * C + 4 * i + 3] = fmaf(-e, ua.v[i].w, wr[16 * C + 4 * i + 3]);
#define GPTQ_PIN(i) "+v"(wr[16 * C + i])
// chunk C of the update, ua = its values of U, ub = chunk C + 1's, both already requested. A chunk that begins at or
// below the step's own row also "updates" rows the sweep is done with: dead registers, nothing reads them again.
template <int C>
__device__ __forceinline__ void gptq_update(float (&wr)[GPTQ_BLOCK], const float* urow, float e, const UChunk& ua,
                                            const UChunk& ub) {
  if constexpr (C < GPTQ_BLOCK / 16) {
    UChunk un;
    gptq_uread<C + 2>(un, urow);
    GPTQ_FMA4(0) GPTQ_FMA4(1) GPTQ_FMA4(2) GPTQ_FMA4(3)
    // pins the updates here: a row's new value is used only at its own step, further down, and the compiler otherwise
    // sinks the fma there while U's values, read here, wait in scratch (5k spills); being volatile it also keeps the
    // LDS reads in the order written
    asm volatile("" : GPTQ_PIN(0), GPTQ_PIN(1), GPTQ_PIN(2), GPTQ_PIN(3), GPTQ_PIN(4), GPTQ_PIN(5), GPTQ_PIN(6),
                 GPTQ_PIN(7), GPTQ_PIN(8), GPTQ_PIN(9), GPTQ_PIN(10), GPTQ_PIN(11), GPTQ_PIN(12), GPTQ_PIN(13),
                 GPTQ_PIN(14), GPTQ_PIN(15));
    gptq_update<C + 1>(wr, urow, e, ub, un);
  }
}
#undef GPTQ_FMA4
#undef GPTQ_PIN

// min / max / max|.| over wr[K0 .. kloc - 1] (kloc uniform, > the first row, which stands in for the rows past it)
template <int K0, int K1>
__device__ __forceinline__ void gptq_range(const float (&wr)[GPTQ_BLOCK], int kloc, float first, float& mx, float& mn,
                                           float& amax) {
  if constexpr (K0 < K1) {
    const float v = K0 < kloc ? wr[K0] : first;
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
    amax = fmaxf(amax, fabsf(v));
    gptq_range<K0 + 1, K1>(wr, kloc, first, mx, mn, amax);
  }
}

template <int J0, int J1>
__device__ __forceinline__ void gptq_load(float (&wr)[GPTQ_BLOCK], const GptqArgs& g, bool valid, int n) {
  if constexpr (J0 < J1) {
    wr[J0] = (valid && J0 < g.B) ? g.w[(size_t)(g.c0 + J0) * (size_t)g.N + n] : 0.f;
    gptq_load<J0 + 1, J1>(wr, g, valid, n);
  }
}

struct GptqState {
  float s;
  int z, gid_prev;
};

template <int J>
__device__ __forceinline__ void gptq_steps(float (&wr)[GPTQ_BLOCK], const float (*us)[GPTQ_BLOCK], const GptqArgs& g,
                                           GptqState& st, bool valid, int n) {
  if constexpr (J < GPTQ_BLOCK) {
    if (J >= g.B) return;  // uniform: a short last block ends here
    const RtnRange r = rtn_range(g.bits);
    const size_t N = (size_t)g.N;
    const int ja = g.c0 + J;
    const int gid = g.col_group ? g.col_group[ja] : ja / g.group;
    bool computed = false;
    if constexpr ((J & 31) == 0) {
      if (!g.params_given && ja % g.group == 0) {
        computed = true;
        // the group's rows: registers up to the block's end, memory beyond it
        const int kend = min(ja + g.group, g.K), kloc = min(kend - g.c0, g.B);
        float mx = wr[J], mn = wr[J], amax = fabsf(wr[J]);
        gptq_range<J + 1, GPTQ_BLOCK>(wr, kloc, wr[J], mx, mn, amax);
        for (int k = g.c0 + g.B; k < kend; ++k) {
          const float v = valid ? g.w[(size_t)k * N + n] : 0.f;
          mx = fmaxf(mx, v);
          mn = fminf(mn, v);
          amax = fmaxf(amax, fabsf(v));
        }
        rtn_params(r, g.asym, mx, mn, amax, st.s, st.z);
        if (valid) {
          g.scale[(size_t)gid * N + n] = st.s;
          if (g.asym) g.zp[(size_t)gid * N + n] = (int8_t)(st.z - r.off);
        }
      }
    }
    if (!computed && (J == 0 || (g.params_given && gid != st.gid_prev))) {
      st.s = valid ? g.scale[(size_t)gid * N + n] : 1.f;
      st.z = (g.asym && valid) ? (int)g.zp[(size_t)gid * N + n] + r.off : 0;
    }
    st.gid_prev = gid;

    constexpr int C0 = (J + 1) / 16;  // the first chunk with a row after this one
    UChunk ua, ub;
    gptq_uread<C0>(ua, us[J]);
    gptq_uread<C0 + 1>(ub, us[J]);
    const float v = wr[J], s = st.s;
    int qi;
    float d, e;
    {
      // no contraction here: e is taken against the value that is stored, the product rounded first, then the
      // subtraction (contracted, v - qi * s would become one fma against the unrounded product)
#pragma clang fp contract(off)
      rtn_quant(r, g.asym, v, s, st.z, qi, d);
      e = (v - d) / us[J][J];
    }
    gptq_update<C0>(wr, us[J], e, ua, ub);
    if (valid) {
      g.q[(size_t)ja * N + n] = (int8_t)qi;
      g.err[(size_t)J * N + n] = e;
      g.w[(size_t)ja * N + n] = d;
    }
    gptq_steps<J + 1>(wr, us, g, st, valid, n);
  }
}

__global__ __launch_bounds__(GPTQ_THREADS) void gptq_sweep_kernel(const GptqArgs g) {
  __shared__ float us[GPTQ_BLOCK][GPTQ_BLOCK];
  const int n = blockIdx.x * GPTQ_THREADS + threadIdx.x;
  const bool valid = n < g.N;

  // U's block, rows and columns c0 .. c0 + 127, zero beyond the block (a short last block updates nothing there)
  for (int r = 0; r < GPTQ_BLOCK; ++r)
    for (int c = threadIdx.x; c < GPTQ_BLOCK; c += GPTQ_THREADS)
      us[r][c] = (r < g.B && c < g.B) ? g.u[(size_t)(g.c0 + r) * (size_t)g.K + (size_t)(g.c0 + c)] : 0.f;

  float wr[GPTQ_BLOCK];
  gptq_load<0, GPTQ_BLOCK>(wr, g, valid, n);
  __syncthreads();

  GptqState st = {1.f, 0, -1};
  gptq_steps<0>(wr, us, g, st, valid, n);
}

}  // namespace
}  // namespace woq

extern "C" int woq_gptq_sweep(float* w_dev, const float* u_dev, int K, int N, int c0, int B, int group, int bits,
                              int asym, int params_given, const int32_t* col_group_dev, int8_t* q_dev,
                              float* scale_dev, int8_t* zp_dev, float* err_dev, void* stream) {
  WOQ_TRY
  WOQ_CHECK(w_dev && u_dev && q_dev && scale_dev && err_dev, "QBits: gptq_sweep: null tensor");
  WOQ_CHECK(K >= 1 && N >= 1, "QBits: gptq_sweep: bad shape");
  WOQ_CHECK(B >= 1 && B <= woq::GPTQ_BLOCK && c0 >= 0 && c0 <= K - B,
            "QBits: gptq_sweep: the block must be 1 .. 128 rows inside the weight");
  WOQ_CHECK(woq::rtn_bits_ok(bits), "QBits: gptq_sweep: bits must be 2, 3, 4 or 8");
  WOQ_CHECK(!asym || zp_dev, "QBits: gptq_sweep: asym needs a zero-point tensor");
  group = woq::rtn_group(K, group);
  WOQ_CHECK(params_given || ((c0 % 32) == 0 && ((group % 32) == 0 || group == K)),
            "QBits: gptq_sweep: computing parameters needs c0 and the group size to be multiples of 32 (or group -1)");
  const woq::GptqArgs g = {w_dev, u_dev, K, N, c0, B, group, bits, asym ? 1 : 0, params_given ? 1 : 0, col_group_dev,
                           q_dev, scale_dev, zp_dev, err_dev};
  hipLaunchKernelGGL(woq::gptq_sweep_kernel, dim3((unsigned)((N + woq::GPTQ_THREADS - 1) / woq::GPTQ_THREADS)),
                     dim3(woq::GPTQ_THREADS), 0, (hipStream_t)stream, g);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}
