// woq_lora.hip — unmerged LoRA adapters beside the packed projections of the decode engine.
//
// y = x . W_deq (+ bias) + s * (x . A^T) . B^T per targeted projection (reference nn/modules.py QuantizedLoraLinearQBits,
// transformers/llm/quantization/lora.py here): A [r][K], B [N][r], s = lora_alpha / r, all fp32 with fp32 accumulation.
// The base GEMV / GEMM kernels keep their code: the adapter term travels through slots they already have.
//   decode step  one launch per fused projection in front of its GEMV writes d[n] = base_bias[n] + s_p * B_p[n'] . t_p,
//                t_p = inv * A_p . x, into an fp32 [N] buffer which the GEMV takes as its `bias` (added after the RMSNorm
//                factor, before SiLU * mul, the residual add and the XQ output). Every workgroup recomputes all of t (at
//                most 192 dot products over K, A from L2 after the first touch) and owns 256 columns: one launch, no
//                hand-off between workgroups, no atomics, a fixed summation order.
//   prompt pass  `shrink` T[m][j] = inv_m * sum_k A[j][k] g_k X[m][k] and `expand` D[m][n] = s_p * T[m] . B_p[n'] on the
//                f32-input MFMA (v_mfma_f32_16x16x4_f32: exact fp32, a k-ordered fmaf chain), the expand in three store
//                modes (woq_host.h LoraExpandMode).
// The parts of a fused projection (q | k | v concatenated along N; gate / up interleaved per 16-column tile as
// runtime.fuse_gate_up lays the blob out) and their ranks are read from a device-resident LoraDesc, so another adapter
// of the same targets changes no pointer and no launch geometry.
#include "woq_device.h"
#include "woq_host.h"
#include "../../include/woq_hip_experimental.h"

namespace woq {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// (part, local index) of stacked row / concatenated column `i`: parts in order, `count(p)` entries each
template <typename F>
__device__ __forceinline__ int lora_find_part(const LoraDesc* __restrict__ d, int& i, int& roff, F count) {
  int p = 0;
  roff = 0;
  const int np = d->n_parts;
  while (p + 1 < np && i >= count(p)) {
    i -= count(p);
    roff += d->part[p].r;
    ++p;
  }
  return p;
}

// ---- decode: the delta vector --------------------------------------------------------------------------------------
// LDS: xs[K] the input as the projection sees it (decoded XQ values, or x * norm_w), ts[LORA_MAX_ROWS], red[4].
template <bool XQ>
__global__ __launch_bounds__(256) void lora_delta_kernel(const LoraDesc* __restrict__ d, XqPtrs xin,
                                                         const float* __restrict__ x, const float* __restrict__ norm_w,
                                                         const float* __restrict__ ssq_in, float eps, int K, int N,
                                                         const float* __restrict__ base, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lora_lds[];
  float* xs = lora_lds;
  float* ts = xs + K;
  float* red = ts + LORA_MAX_ROWS;
  const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int np = d->n_parts;
  int r_tot = 0;
  for (int p = 0; p < np; ++p) r_tot += d->part[p].r;

  // 1. the input, and the RMSNorm factor of the consumer
  float ss = 0.f;
  bool norm;
  if constexpr (XQ) {
    norm = ssq_in != nullptr;
    const int8_t* limbs = (const int8_t*)xin.limbs;
    for (int k = tid; k < K; k += 256) {
      const int8_t* l = limbs + (size_t)(k >> 4) * 48 + (k & 15);
      const int v = (int)l[0] + 256 * (int)l[16] + 65536 * (int)l[32];  // |v| <= 2^21: exact in fp32
      xs[k] = (float)v * (xin.u[k >> 4] * 16.f);                         // times a power of two: exact
    }
    if (norm)
      for (int b = tid; b < (K >> 4); b += 256) ss += ssq_in[b];
  } else {
    norm = norm_w != nullptr;
    for (int k = tid; k < K; k += 256) {
      const float v = x[k];
      ss = fmaf(v, v, ss);
      xs[k] = norm ? v * norm_w[k] : v;
    }
  }
  ss = wave_sum(ss);
  if (lane == 0) red[wid] = ss;
  __syncthreads();
  const float inv = norm ? 1.0f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)K + eps) : 1.f;

  // 2. t: stacked row `row` = row j of part p's A; one wave per row, lanes stride over k four values at a time
  for (int row = wid; row < r_tot; row += 4) {
    int j = row, roff;
    const int p = lora_find_part(d, j, roff, [&](int q) { return d->part[q].r; });
    const float* a = d->part[p].A + (size_t)j * K;
    float acc = 0.f;
#pragma unroll 4
    for (int k = lane * 4; k < K; k += 256) {
      const float4_t av = *(const float4_t*)(a + k);
      const float4_t xv = *(const float4_t*)(xs + k);
      acc = fmaf(av.x, xv.x, acc);
      acc = fmaf(av.y, xv.y, acc);
      acc = fmaf(av.z, xv.z, acc);
      acc = fmaf(av.w, xv.w, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) ts[row] = acc * inv;
  }
  __syncthreads();

  // 3. this thread's column, in blob column order
  const int n = (int)blockIdx.x * 256 + tid;
  if (n >= N) return;
  int p, nn = n, roff = 0;
  if (d->interleave) {
    p = (n >> 4) & 1;
    nn = ((n >> 5) << 4) + (n & 15);
    roff = p ? d->part[0].r : 0;
  } else {
    p = lora_find_part(d, nn, roff, [&](int q) { return d->part[q].n; });
  }
  const int r = d->part[p].r;
  const float b0 = base != nullptr ? base[n] : 0.f;
  if (r == 0 || nn >= d->part[p].n) {  // no adapter on this part: the static bias bit for bit
    out[n] = b0;
    return;
  }
  const float* brow = d->part[p].B + (size_t)nn * r;
  float acc = 0.f;
  for (int j = 0; j < r; ++j) acc = fmaf(brow[j], ts[roff + j], acc);
  out[n] = b0 + d->part[p].s * acc;
}

static size_t lora_delta_lds(int K) { return ((size_t)K + LORA_MAX_ROWS + 4) * sizeof(float); }

template <bool XQ>
static int launch_lora_delta(const LoraDesc* desc, const XqPtrs& xin, const float* x, const float* norm_w,
                             const float* ssq_in, float eps, int K, int N, const float* base, float* out,
                             hipStream_t st) {
  if (desc == nullptr || out == nullptr || K < 16 || (K & 15) != 0 || N < 1)
    return woq::fail("QBits: bad LoRA delta arguments (K must be a positive multiple of 16)");
  const size_t lds = lora_delta_lds(K);
  if (lds > LORA_DELTA_MAX_LDS) return woq::fail("QBits: the LoRA delta launch holds K up to 40000 input values");
  if (lds > 48 * 1024)
    if (const int rc = allow_dynamic_lds<lora_delta_kernel<XQ>>(LORA_DELTA_MAX_LDS)) return rc;
  hipLaunchKernelGGL((lora_delta_kernel<XQ>), dim3((N + 255) / 256), dim3(256), lds, st, desc, xin, x, norm_w, ssq_in,
                     eps, K, N, base, out);
  return 0;
}

int launch_lora_delta_xq(const LoraDesc* desc, const XqPtrs& xin, const float* ssq_in, float eps, int K, int N,
                         const float* base_bias, float* out, hipStream_t st) {
  if (xin.limbs == nullptr || xin.u == nullptr) return woq::fail("QBits: the LoRA delta launch needs its XQ input");
  return launch_lora_delta<true>(desc, xin, nullptr, nullptr, ssq_in, eps, K, N, base_bias, out, st);
}

int launch_lora_delta_f32(const LoraDesc* desc, const float* x, const float* norm_w, float eps, int K, int N,
                          const float* base_bias, float* out, hipStream_t st) {
  if (x == nullptr) return woq::fail("QBits: the LoRA delta launch needs its input");
  return launch_lora_delta<false>(desc, XqPtrs{nullptr, nullptr, nullptr}, x, norm_w, nullptr, eps, K, N, base_bias, out,
                                  st);
}

// ---- prompt pass: shrink -------------------------------------------------------------------------------------------
// One workgroup = 16 rows of X times 16 stacked rows of A; its four waves take interleaved 16-k runs of K and are
// summed in wave order through LDS. v_mfma_f32_16x16x4_f32: lane l supplies A-operand X[m0 + (l & 15)][k] and B-operand
// A[j0 + (l & 15)][k] for ONE k per instruction; a lane loads four consecutive k at once and feeds them to four
// instructions, both operands alike, so the k order inside a 16-k run is a fixed permutation. D: register v of lane l =
// row 4 (l >> 4) + v, column l & 15.
__device__ __forceinline__ float4_t lora_load4(const float* p) { return *(const float4_t*)p; }
__device__ __forceinline__ float4_t lora_load4(const _Float16* p) {
  typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
  const half4_t h = *(const half4_t*)p;
  return float4_t{(float)h.x, (float)h.y, (float)h.z, (float)h.w};
}

template <typename XT>
__global__ __launch_bounds__(256) void lora_shrink_kernel(const LoraDesc* __restrict__ d, const XT* __restrict__ X,
                                                          int ldx, int M, int K, const float* __restrict__ gamma,
                                                          float eps, float* __restrict__ T, int ldt) {
  __shared__ f32x4 part[4][64];
  __shared__ float ssl[4][16];
  const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int np = d->n_parts;
  int r_tot = 0;
  for (int p = 0; p < np; ++p) r_tot += d->part[p].r;
  const int m0 = (int)blockIdx.x * 16, j0 = (int)blockIdx.y * 16;
  if (j0 >= r_tot) return;  // (the whole workgroup)
  const int m = m0 + (lane & 15);
  const XT* xrow = m < M ? X + (size_t)m * ldx : nullptr;
  const float* arow = nullptr;
  {
    int j = j0 + (lane & 15), roff;
    if (j < r_tot) {
      const int p = lora_find_part(d, j, roff, [&](int q) { return d->part[q].r; });
      arow = d->part[p].A + (size_t)j * K;
    }
  }
  const bool norm = gamma != nullptr;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float ss = 0.f;
  const float4_t zero = {0.f, 0.f, 0.f, 0.f};
  for (int k = wid * 16 + (lane >> 4) * 4; k < K; k += 64) {
    float4_t xv = xrow != nullptr ? lora_load4(xrow + k) : zero;
    const float4_t av = arow != nullptr ? *(const float4_t*)(arow + k) : zero;
    if (norm) {
      ss = fmaf(xv.x, xv.x, ss);
      ss = fmaf(xv.y, xv.y, ss);
      ss = fmaf(xv.z, xv.z, ss);
      ss = fmaf(xv.w, xv.w, ss);
      xv *= *(const float4_t*)(gamma + k);
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.x, av.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.y, av.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.z, av.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.w, av.w, acc, 0, 0, 0);
  }
  ss += __shfl_xor(ss, 16, 64);  // the four lanes that share row l & 15
  ss += __shfl_xor(ss, 32, 64);
  if (lane < 16) ssl[wid][lane] = ss;
  part[wid][lane] = acc;
  __syncthreads();
  if (wid != 0) return;
  const f32x4 sum = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
  const int col = j0 + (lane & 15);
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int rl = 4 * (lane >> 4) + v, row = m0 + rl;
    float inv = 1.f;
    if (norm) inv = 1.0f / sqrtf(((ssl[0][rl] + ssl[1][rl]) + (ssl[2][rl] + ssl[3][rl])) / (float)K + eps);
    if (row < M && col < r_tot) T[(size_t)row * ldt + col] = sum[v] * inv;
  }
}

int launch_lora_shrink(const LoraDesc* desc, int r_tot, const void* X, int x_dtype, int ldx, int M, int K,
                       const float* norm_w, float eps, float* T, int ldt, hipStream_t st) {
  if (desc == nullptr || X == nullptr || T == nullptr || M < 1 || K < 16 || (K & 15) != 0 || (ldx & 3) != 0 || ldx < K ||
      r_tot < 0 || r_tot > LORA_MAX_ROWS || ldt < r_tot)
    return woq::fail("QBits: bad LoRA shrink arguments (K a multiple of 16, ldx a multiple of 4, at most 192 stacked rows)");
  if (x_dtype != WOQ_F32 && x_dtype != WOQ_F16) return woq::fail("QBits: the LoRA shrink takes fp32 or fp16 rows");
  if (x_dtype == WOQ_F16 && norm_w != nullptr) return woq::fail("QBits: the LoRA shrink normalises fp32 rows only");
  if (r_tot == 0) return 0;
  const dim3 grid((M + 15) / 16, (r_tot + 15) / 16), block(256);
  if (x_dtype == WOQ_F32)
    hipLaunchKernelGGL(lora_shrink_kernel<float>, grid, block, 0, st, desc, (const float*)X, ldx, M, K, norm_w, eps, T, ldt);
  else
    hipLaunchKernelGGL(lora_shrink_kernel<_Float16>, grid, block, 0, st, desc, (const _Float16*)X, ldx, M, K, norm_w, eps,
                       T, ldt);
  return 0;
}

// ---- prompt pass: expand -------------------------------------------------------------------------------------------
// One wave = 16 rows times one 16-column tile of one part: D = T[m][roff .. roff + r) . B_p[n'][0 .. r)^T, r / 4 MFMAs
// (ranks that are no multiple of 4 are padded with zeros in the operands).
__device__ __forceinline__ f32x4 lora_expand_tile(const LoraPart& P, const float* __restrict__ trow, int roff, int nn,
                                                  int lane) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int r = P.r;
  const float* brow = P.B + (size_t)nn * r;
  for (int j0 = 0; j0 < r; j0 += 4) {
    const int j = j0 + (lane >> 4);
    const float a = (trow != nullptr && j < r) ? trow[roff + j] : 0.f;
    const float b = j < r ? brow[j] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

template <int MODE>
__global__ __launch_bounds__(256) void lora_expand_kernel(const LoraDesc* __restrict__ d, const float* __restrict__ T,
                                                          int ldt, int M, int n_tiles, void* __restrict__ out, int ldo,
                                                          const _Float16* __restrict__ gu, int ld_gu) {
  const int lane = (int)threadIdx.x & 63, wid = (int)threadIdx.x >> 6;
  const int tile = (int)blockIdx.y * 4 + wid;
  if (tile >= n_tiles) return;  // (the whole wave; no barrier below)
  const int m0 = (int)blockIdx.x * 16, m = m0 + (lane & 15);
  const float* trow = m < M ? T + (size_t)m * ldt : nullptr;
  const int c = lane & 15;
  if constexpr (MODE == LORA_EXPAND_SILU) {
    // output tile `tile` of [M][inter]: gate = part 0, up = part 1, both at local columns 16 tile + c
    const LoraPart& G = d->part[0];
    const LoraPart& U = d->part[1];
    const int nn = tile * 16 + c;
    const f32x4 dg = G.r > 0 ? lora_expand_tile(G, trow, 0, nn, lane) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 du = U.r > 0 ? lora_expand_tile(U, trow, G.r, nn, lane) : f32x4{0.f, 0.f, 0.f, 0.f};
    _Float16* o = (_Float16*)out;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = m0 + 4 * (lane >> 4) + v;
      if (row >= M) continue;
      const _Float16* g = gu + (size_t)row * ld_gu + (size_t)tile * 32 + c;
      const float gv = (float)g[0] + G.s * dg[v];
      const float uv = (float)g[16] + U.s * du[v];
      o[(size_t)row * ldo + nn] = (_Float16)(gv / (1.0f + __expf(-gv)) * uv);
    }
  } else {
    int nn = tile * 16, roff;
    const int p = lora_find_part(d, nn, roff, [&](int q) { return d->part[q].n; });
    const LoraPart& P = d->part[p];
    if (P.r == 0 || nn >= P.n) return;
    const f32x4 dd = lora_expand_tile(P, trow, roff, nn + c, lane);
    const int n = tile * 16 + c;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = m0 + 4 * (lane >> 4) + v;
      if (row >= M) continue;
      if constexpr (MODE == LORA_EXPAND_ADD_F32) {
        float* o = (float*)out + (size_t)row * ldo + n;
        *o += P.s * dd[v];
      } else {
        _Float16* o = (_Float16*)out + (size_t)row * ldo + n;
        *o = (_Float16)((float)*o + P.s * dd[v]);
      }
    }
  }
}

int launch_lora_expand(const LoraDesc* desc, const float* T, int ldt, int M, int N, int mode, void* out, int ldo,
                       const _Float16* gu, int ld_gu, hipStream_t st) {
  if (desc == nullptr || T == nullptr || out == nullptr || M < 1 || N < 16 || (N & 15) != 0)
    return woq::fail("QBits: bad LoRA expand arguments (N must be a positive multiple of 16)");
  if (mode == LORA_EXPAND_SILU) {
    if (gu == nullptr || (N & 31) != 0 || ld_gu < N || ldo < N / 2)
      return woq::fail("QBits: the LoRA gate/up expand needs the [M][2 * inter] gate/up rows");
    const int n_tiles = N / 32;
    hipLaunchKernelGGL(lora_expand_kernel<LORA_EXPAND_SILU>, dim3((M + 15) / 16, (n_tiles + 3) / 4), dim3(256), 0, st,
                       desc, T, ldt, M, n_tiles, out, ldo, gu, ld_gu);
    return 0;
  }
  if (ldo < N) return woq::fail("QBits: bad LoRA expand arguments (row stride below N)");
  const int n_tiles = N / 16;
  const dim3 grid((M + 15) / 16, (n_tiles + 3) / 4), block(256);
  if (mode == LORA_EXPAND_ADD_F32)
    hipLaunchKernelGGL(lora_expand_kernel<LORA_EXPAND_ADD_F32>, grid, block, 0, st, desc, T, ldt, M, n_tiles, out, ldo,
                       nullptr, 0);
  else if (mode == LORA_EXPAND_ADD_F16)
    hipLaunchKernelGGL(lora_expand_kernel<LORA_EXPAND_ADD_F16>, grid, block, 0, st, desc, T, ldt, M, n_tiles, out, ldo,
                       nullptr, 0);
  else
    return woq::fail("QBits: unknown LoRA expand mode");
  return 0;
}

// null when `d` (host copy) describes parts the kernels take for a projection of N blob columns, else the reason
const char* lora_desc_problem(const LoraDesc& d, int N) {
  if (d.n_parts < 1 || d.n_parts > LORA_MAX_PARTS) return "QBits: a LoRA projection has one to three parts";
  if (d.interleave && d.n_parts != 2) return "QBits: the interleaved LoRA layout has two parts (gate, up)";
  long long n = 0;
  for (int p = 0; p < d.n_parts; ++p) {
    const LoraPart& P = d.part[p];
    if (P.r < 0 || P.r > LORA_MAX_RANK) return "QBits: LoRA ranks run from 1 to 64";
    if (P.n < 16 || (P.n & 15) != 0) return "QBits: a LoRA part's columns must be a positive multiple of 16";
    if (P.r > 0 && (P.A == nullptr || P.B == nullptr || ((uintptr_t)P.A & 15) != 0))
      return "QBits: a LoRA part needs its A (16-byte aligned) and B tables";
    n += P.n;
  }
  if (d.interleave && d.part[0].n != d.part[1].n) return "QBits: gate and up have the same number of columns";
  if (n != N) return "QBits: the LoRA parts' columns do not add up to the projection's";
  return nullptr;
}

}  // namespace woq

// ---- test entry points (include/woq_hip_experimental.h): each forwards to the engine's own launcher -----------------
namespace {
// the descriptor of a probe call on the device, from host arrays of n_parts entries; released by `free`
struct ProbeDesc {
  woq::LoraDesc host;
  woq::LoraDesc* dev = nullptr;
  int init(int n_parts, int interleave, const void* const* a, const void* const* b, const int* r, const int* n,
           const float* s, int N, hipStream_t st) {
    if (n_parts < 1 || n_parts > woq::LORA_MAX_PARTS || !a || !b || !r || !n || !s)
      return woq::fail("QBits: bad LoRA probe arguments");
    host = woq::LoraDesc{};
    host.n_parts = n_parts, host.interleave = interleave != 0;
    for (int p = 0; p < n_parts; ++p) host.part[p] = woq::LoraPart{(const float*)a[p], (const float*)b[p], r[p], n[p], s[p], 0};
    if (const char* why = woq::lora_desc_problem(host, N)) return woq::fail(why);
    WOQ_HIP(hipMallocAsync((void**)&dev, sizeof(host), st));
    WOQ_HIP(hipMemcpyAsync(dev, &host, sizeof(host), hipMemcpyHostToDevice, st));
    WOQ_HIP(hipStreamSynchronize(st));  // (the copy reads this object)
    return 0;
  }
  int r_tot() const {
    int t = 0;
    for (int p = 0; p < host.n_parts; ++p) t += host.part[p].r;
    return t;
  }
  void free(hipStream_t st) {
    if (dev) hipFreeAsync(dev, st);
    dev = nullptr;
  }
};
}  // namespace

extern "C" {

WOQ_API int woq_probe_lora_delta(int form, const void* x, const float* xq_u, const float* xq_sx, const float* aux,
                                 float eps, int K, int N, int n_parts, int interleave, const void* const* a_dev,
                                 const void* const* b_dev, const int* ranks, const int* cols, const float* scalings,
                                 const float* base_bias, float* out, void* stream) {
  WOQ_TRY
  WOQ_CHECK((form == 0 || form == 1) && x != nullptr && out != nullptr, "QBits: bad LoRA delta probe arguments");
  WOQ_CHECK(form == 1 || (xq_u != nullptr && xq_sx != nullptr), "QBits: an XQ input needs all of its parts");
  const hipStream_t st = (hipStream_t)stream;
  ProbeDesc pd;
  if (const int rc = pd.init(n_parts, interleave, a_dev, b_dev, ranks, cols, scalings, N, st)) return rc;
  const int rc = form == 0 ? woq::launch_lora_delta_xq(pd.dev, woq::XqPtrs{(uint8_t*)x, (float*)xq_u, (float*)xq_sx}, aux,
                                                       eps, K, N, base_bias, out, st)
                           : woq::launch_lora_delta_f32(pd.dev, (const float*)x, aux, eps, K, N, base_bias, out, st);
  const hipError_t le = hipGetLastError();
  pd.free(st);
  if (rc) return rc;
  WOQ_HIP(le);
  WOQ_END
}

WOQ_API int woq_probe_lora_shrink(const void* X, int x_dtype, int ldx, int M, int K, const float* norm_w, float eps,
                                  int n_parts, const void* const* a_dev, const int* ranks, float* T, int ldt,
                                  void* stream) {
  WOQ_TRY
  const hipStream_t st = (hipStream_t)stream;
  WOQ_CHECK(n_parts >= 1 && n_parts <= woq::LORA_MAX_PARTS && a_dev && ranks, "QBits: bad LoRA probe arguments");
  // (the shrink reads A and the ranks only: B, the columns and the scalings are placeholders)
  const void* b[woq::LORA_MAX_PARTS];
  int n[woq::LORA_MAX_PARTS];
  float s[woq::LORA_MAX_PARTS];
  for (int p = 0; p < n_parts; ++p) b[p] = a_dev[p], n[p] = 16, s[p] = 1.f;
  ProbeDesc pd;
  if (const int rc = pd.init(n_parts, 0, a_dev, b, ranks, n, s, 16 * n_parts, st)) return rc;
  const int rc = woq::launch_lora_shrink(pd.dev, pd.r_tot(), X, x_dtype, ldx, M, K, norm_w, eps, T, ldt, st);
  const hipError_t le = hipGetLastError();
  pd.free(st);
  if (rc) return rc;
  WOQ_HIP(le);
  WOQ_END
}

WOQ_API int woq_probe_lora_expand(int mode, const float* T, int ldt, int M, int N, int n_parts,
                                  const void* const* b_dev, const int* ranks, const int* cols, const float* scalings,
                                  void* out, int ldo, const void* gu, int ld_gu, void* stream) {
  WOQ_TRY
  const hipStream_t st = (hipStream_t)stream;
  int r_tot = 0;
  for (int p = 0; ranks != nullptr && p < n_parts && p < woq::LORA_MAX_PARTS; ++p) r_tot += ranks[p];
  WOQ_CHECK(ldt >= r_tot, "QBits: bad LoRA expand probe arguments (ldt below the stacked ranks)");
  ProbeDesc pd;  // (the expand reads B only: A is a placeholder)
  if (const int rc = pd.init(n_parts, mode == woq::LORA_EXPAND_SILU, b_dev, b_dev, ranks, cols, scalings, N, st)) return rc;
  const int rc = woq::launch_lora_expand(pd.dev, T, ldt, M, N, mode, out, ldo, (const _Float16*)gu, ld_gu, st);
  const hipError_t le = hipGetLastError();
  pd.free(st);
  if (rc) return rc;
  WOQ_HIP(le);
  WOQ_END
}

}  // extern "C"
