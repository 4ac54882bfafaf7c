// woq_gemv_xq.hip — host side of the batch-1 decode GEMV over an XQ activation vector (kernel: woq_gemv_xqs.h) and
// the standalone fp32 -> XQ conversion. Reference path replaced: qbits.cpp:113-140 (woq_linear at M = 1).
// It replaced the round-2 kernel (every tile requested up front, offset-binary limbs); same-box A/B in
// profiles/r03*_xq_probe.txt.
#include <algorithm>

#include "woq_gemv_common.h"
#include "woq_gemv_launch.h"
#ifdef WOQ_XQS_STAMPS  // measurement build only (tools/xqs_stamps.py): per-(workgroup, wave) wall-clock stamps of the stages
__device__ unsigned long long* g_xqs_probe = nullptr;
#endif
#include "woq_gemv_xqs.h"
#include "woq_host.h"
#include "woq_xq.h"
#include "../../include/woq_hip_experimental.h"

#ifdef WOQ_XQS_STAMPS
extern "C" __attribute__((visibility("default"))) int woq_xqs_set_probe(void* buf_dev) {
  unsigned long long* p = (unsigned long long*)buf_dev;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_xqs_probe), &p, sizeof(p), 0, hipMemcpyHostToDevice) == hipSuccess ? 0 : 1;
}
#endif

namespace woq {

// what a launch of the XQ kernel carries beside the blob (BlobView)
struct XqLaunch {
  XqPtrs xin;
  int flags;
  float* out;
  const float* bias;
  const float* residual;
  float eps;
  const float* ssq_in;
  int n_ssq;
  XqPtrs xo;
  const float* next_norm_w;
  float* ssq_out;
  const CommDev* tp;  // tensor parallel: push the outputs (partial sums) into the peers' inboxes from the epilogue
  int nw, grid, kt_begin, kt_count;
};

// window depth by tiles per wave (profiles/r03c_xq_probe.txt)
// round 6 (profiles/r06ad_gemv_occupancy_and_window.txt): 6 — same-box A/Bs on the round-6 kernel read 4 / 6 / 8 -> 993.5 / 1001.5 / 992.6 tokens/s and
// 4 / 5 / 7 -> 999.8 / 1002.7 / 1003.2 (round 4 had measured no difference); it only reaches the 8-tile waves (o, down)
constexpr int XQ_WINDOW_DEPTH = 6;

template <int TPW, int CB, int SMODE, bool ASYM, bool S32, int NDIG>
static int launch_xq_t(const BlobView& v, const XqLaunch& a, hipStream_t st) {
  typedef XqsLds<TPW, CB, SMODE, ASYM, S32> L;
  const size_t lds = L::total(a.nw);
  if (lds > 160 * 1024) return woq::fail("QBits: XQ GEMV geometry does not fit LDS");
  constexpr auto kern = gemv_xqs_kernel<TPW, CB, (TPW < XQ_WINDOW_DEPTH ? TPW : XQ_WINDOW_DEPTH), SMODE, ASYM, S32, NDIG>;
  if (const int rc = allow_dynamic_lds<kern>(160 * 1024)) return rc;
  const int base = a.kt_count / a.nw, rem = a.kt_count % a.nw;
  XqsLate late;
  late.zp = v.zp, late.xsx = a.xin.sx, late.out = a.out, late.bias = a.bias, late.residual = a.residual;
  late.ssq_in = a.ssq_in, late.next_norm_w = a.next_norm_w, late.ssq_out = a.ssq_out, late.tp = a.tp;
  late.tag_seq = nullptr, late.tag_layer = 0, late.xo = a.xo, late.eps = a.eps, late.N = v.N, late.K = v.K;
  late.n_ssq = a.n_ssq, late.lut = v.lut;
  hipLaunchKernelGGL(kern, dim3(a.grid), dim3(a.nw * 64), lds, st, v.q, v.scales, a.xin.limbs, a.xin.u, v.tiles_k,
                     a.kt_begin, base, rem, v.n_groups, v.tpg_shift | (a.flags << 8) | (a.nw << 16), late);
  return 0;
}

// Geometry: nw waves x tpw tiles cover a K range of tiles_k tiles. Measured per projection of the Llama-2-7B layer
// (profiles/r03c_xq_probe.txt): 8 tiles per wave for single column tiles with long K, 4 for the fused gate/up pairs
// (twice the bytes per tile step) and short K.
static bool xq_geometry(int tiles_k, int cb, int smode, int& nw, int& tpw, int ndig = 0) {
  tpw = (tiles_k > 16 && cb == 1) ? 8 : 4;
  const bool wide = cb == 2 && ndig == 3;  // table weights, three digit planes, column-tile pairs: 512-thread launches
  if (wide && tiles_k > 32 && smode == 0) tpw = 8;
  nw = (tiles_k + tpw - 1) / tpw;
  return nw >= 1 && nw <= ((cb * tpw > 8 || wide) ? 8 : 16);  // the kernel's __launch_bounds__
}
// the chained launches of a batch-1 projection: walked by the GEMV and by its measurement twins alike
static KPlan xq_k_plan(const BlobView& v, int epi) {
  const int cb = epi == 1 ? 2 : 1;
  return plan_k_ranges(v.tiles_k, epi == 0, [&](int tiles, int& nw, int& tpw) {
    return xq_geometry(tiles, cb, v.smode, nw, tpw, v.ndig);
  });
}

// view and K-range plan of a blob the XQ kernel takes as a batch-1 projection; false = it does not
static bool xq_view(const void* blob, const woq_blob_header& h, int epi, BlobView& v, KPlan& plan) {
  const bool table = is_table_type(h.weight_type) && h.off_zp == 0;
  if ((h.weight_type != WOQ_W_INT4_CLIP && !table) || h.off_shuffle != 0 || (h.K % WOQ_TILE_K) != 0 || h.K != h.Kpad)
    return false;
  if (!blob_view(blob, h, v) || (epi == 1 && (v.tiles_n & 1))) return false;
  plan = xq_k_plan(v, epi);
  return plan.chunks > 0;
}

bool gemv_xq_supported(const woq_blob_header& h, int epi) {
  BlobView v;
  KPlan plan;
  return xq_view(nullptr, h, epi, v, plan);
}

int launch_gemv_xq(const XqPtrs& xin, const void* blob, const woq_blob_header& h, const float* bias, float* out,
                   const float* ssq_in, float eps, const float* residual, int epi, const XqPtrs& xo,
                   const float* next_norm_w, float* ssq_out, hipStream_t st, const CommDev* tp) {
  BlobView v;
  KPlan plan;
  if (!xq_view(blob, h, epi, v, plan)) return woq::fail("QBits: shape not covered by the XQ GEMV");
  XqLaunch a;
  a.xin = xin;
  a.flags = (v.sbf16 ? 1 : 0) | (epi == 1 ? 2 : 0);
  a.eps = eps;
  a.n_ssq = h.K / 16;
  if (ssq_in != nullptr && a.n_ssq > 1024) return woq::fail("QBits: RMSNorm partials beyond K = 16384");
  a.next_norm_w = next_norm_w;
  a.ssq_out = ssq_out;
  const int cb = epi == 1 ? 2 : 1;
  if (plan.chunks > 1 && (ssq_in != nullptr || out == nullptr))
    return woq::fail("QBits: a K range split over chained launches takes no norm and needs an fp32 output");
  a.grid = v.tiles_n / cb;
  a.out = out;
  a.ssq_in = ssq_in;
  return for_each_k_chunk(plan, [&](int c, int kt_begin, int kt_count, bool last) {
    a.kt_begin = kt_begin;
    a.kt_count = kt_count;
    a.nw = plan.nw[c];
    a.bias = c == 0 ? bias : nullptr;
    a.residual = c == 0 ? residual : out;  // chunk c > 0 adds onto the previous chunk's output
    a.xo = last ? xo : XqPtrs{nullptr, nullptr, nullptr};
    a.tp = last ? tp : nullptr;
    return select_tpw_cb(plan.tpw[c], cb, [&](auto TPW, auto CB) {
      // 4-bit table types (nf4 / fp4): one digit plane (fp4_e2m1), two (bitsandbytes fp4, nf4 at reduced-precision
      // compute) or three (nf4 at compute fp32)
      return select_qform(v.smode, v.asym, v.s32, v.ndig, "QBits: bad XQ GEMV configuration",
                          [&](auto SM, auto AS, auto S3, auto ND) {
                            return launch_xq_t<TPW(), CB(), SM(), AS(), S3(), ND()>(v, a, st);
                          });
    });
  });
}

// ---- measurement twins (bench.py roofline.ceiling): what THIS launch structure reaches with the arithmetic taken out --
// load-only twin: the same grid, waves, K slices and non-temporal 16-byte requests as the GEMV of this blob, nothing else
template <int TPW, int CB>
__global__ __launch_bounds__(1024) void gemv_stream_twin_kernel(const u32x4* __restrict__ q, int tiles_k, int kt_off,
                                                                int base_tiles, int rem_tiles,
                                                                unsigned int* __restrict__ sink) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kt0 = kt_off + wid * base_tiles + min(wid, rem_tiles);
  const int cnt = base_tiles + (wid < rem_tiles ? 1 : 0);
  u32x4 acc = {0, 0, 0, 0};
  u32x4 w[CB][TPW];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int kt = min(kt0 + min(t, cnt - 1), tiles_k - 1);
      w[cb][t] = __builtin_nontemporal_load(q + ((size_t)(blockIdx.x * CB + cb) * tiles_k + kt) * 64 + lane);
    }
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc |= w[cb][t];
  if ((acc.x | acc.y | acc.z | acc.w) == 0x12345u) sink[0] = 1;  // keeps the loads alive; never true for real blobs
}
__global__ void gemv_empty_twin_kernel(unsigned int* __restrict__ sink) {
  if (threadIdx.x == 0x7fffffffu) sink[0] = 1;
}

int launch_gemv_twin(const void* blob, const woq_blob_header& h, int epi, int mode, unsigned int* sink, hipStream_t st) {
  BlobView v;
  blob_view(blob, h, v);  // (the twins load tiles and touch no scale: any group size)
  const int cb = epi == 1 ? 2 : 1;
  const KPlan plan = xq_k_plan(v, epi);  // K ranges beyond one launch: the same chained launches as the GEMV
  if (plan.chunks == 0) return woq::fail("QBits: shape not covered by the XQ GEMV");
  return for_each_k_chunk(plan, [&](int c, int kt_begin, int kt_count, bool) {
    const int nw = plan.nw[c], base = kt_count / nw, rem = kt_count % nw;
    const dim3 grid(v.tiles_n / cb), block(nw * 64);
    if (mode == 1) {
      hipLaunchKernelGGL(gemv_empty_twin_kernel, grid, block, 0, st, sink);
      return 0;
    }
    return select_tpw_cb(plan.tpw[c], cb, [&](auto TPW, auto CB) {
      hipLaunchKernelGGL((gemv_stream_twin_kernel<TPW(), CB()>), grid, block, 0, st, v.q, v.tiles_k, kt_begin, base, rem,
                         sink);
      return 0;
    });
  });
}

// ---- standalone conversion: fp32 vector (optionally times a norm weight) -> XQ, one block per 16 threads ----------
__global__ __launch_bounds__(256) void xq_from_f32_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                          int K, XqPtrs xo, float* __restrict__ ssq_out) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;  // K % 16 == 0 and 256 % 16 == 0: rows are whole blocks
  const bool live = i < K;
  const float v = live ? x[i] : 0.f;
  if (ssq_out != nullptr) {
    const float ss = row16_sum(v * v);
    if (live && (i & 15) == 0) ssq_out[i >> 4] = ss;
  }
  const float y = live && g != nullptr ? v * g[i] : v;
  if (i < ((K + 15) & ~15)) xq_emit16(y, xo, i >> 4, i & 15);
}

void launch_xq_from_f32(const float* x, const float* norm_w, int K, const XqPtrs& xo, float* ssq_out, hipStream_t st) {
  hipLaunchKernelGGL(xq_from_f32_kernel, dim3((K + 255) / 256), dim3(256), 0, st, x, norm_w, K, xo, ssq_out);
}

}  // namespace woq

extern "C" {

// test entry points (include/woq_hip_experimental.h): the conversion and the XQ GEMV on caller-owned buffers
WOQ_API int woq_probe_xq_from_f32(const float* x, const float* norm_w, int K, void* limbs_out, float* u_out,
                                  float* sx_out, float* ssq_out, void* stream) {
  WOQ_TRY
  WOQ_CHECK(x && limbs_out && u_out && sx_out && K >= 16 && (K & 15) == 0, "QBits: bad XQ conversion probe arguments");
  woq::launch_xq_from_f32(x, norm_w, K, woq::XqPtrs{(uint8_t*)limbs_out, u_out, sx_out}, ssq_out, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

// `comm` (woq_probe_gemv_xq_tp; null = none): the last chained launch pushes its outputs, this rank's partial sums, into
// the peers' inboxes
static int probe_gemv_xq(const float* x, const float* in_norm_w, float eps, const void* blob, int epi, const float* bias,
                         const float* residual, const float* next_norm_w, float* out, void* xo_limbs, float* xo_u,
                         float* xo_sx, float* ssq_out, void* stream, woq_comm* comm) {
  WOQ_TRY
  const woq::CommDev* tp = comm != nullptr ? woq_comm_dev_ptr(comm) : nullptr;
  WOQ_CHECK(comm == nullptr || tp != nullptr, "QBits: tensor-parallel communicator is not connected");
  WOQ_CHECK(x && blob && (epi == 0 || epi == 1), "QBits: bad XQ GEMV probe arguments");
  WOQ_CHECK(out != nullptr || xo_limbs != nullptr, "QBits: the XQ GEMV probe needs an output");
  WOQ_CHECK(xo_limbs == nullptr || (xo_u && xo_sx), "QBits: an XQ output needs all of its parts");
  WOQ_CHECK(xo_limbs != nullptr || (next_norm_w == nullptr && ssq_out == nullptr),
            "QBits: next_norm_w and ssq_out belong to the XQ output");
  const hipStream_t st = (hipStream_t)stream;
  woq_blob_header h;
  WOQ_HIP(hipMemcpyAsync(&h, blob, sizeof(h), hipMemcpyDeviceToHost, st));
  WOQ_HIP(hipStreamSynchronize(st));
  WOQ_CHECK(h.magic == WOQ_BLOB_MAGIC, "QBits: not a WQH1 packed weight");
  if (!woq::gemv_xq_supported(h, epi)) return woq::fail("QBits: shape not covered by the XQ GEMV");
  WOQ_CHECK(tp == nullptr || (size_t)(epi == 1 ? h.N / 2 : h.N) <= woq_comm_max_elems(comm),
            "QBits: more output columns than the communicator's inbox holds");
  // scratch: the input as an XQ vector, then its K / 16 RMSNorm partials
  const size_t xq_sz = woq::xq_bytes(h.K), nblk = (size_t)h.K / 16;
  uint8_t* ws = nullptr;
  WOQ_HIP(hipMallocAsync((void**)&ws, xq_sz + nblk * sizeof(float), st));
  const woq::XqPtrs xin = woq::xq_carve(ws, h.K);
  float* ssq_in = in_norm_w != nullptr ? (float*)(ws + xq_sz) : nullptr;
  woq::launch_xq_from_f32(x, in_norm_w, h.K, xin, ssq_in, st);
  const int rc = woq::launch_gemv_xq(xin, blob, h, bias, out, ssq_in, eps, residual, epi,
                                     woq::XqPtrs{(uint8_t*)xo_limbs, xo_u, xo_sx}, next_norm_w, ssq_out, st, tp);
  const hipError_t le = hipGetLastError();
  hipFreeAsync(ws, st);
  if (rc) return rc;
  WOQ_HIP(le);
  WOQ_END
}

WOQ_API int woq_probe_gemv_xq(const float* x, const float* in_norm_w, float eps, const void* blob, int epi,
                              const float* bias, const float* residual, const float* next_norm_w, float* out,
                              void* xo_limbs, float* xo_u, float* xo_sx, float* ssq_out, void* stream) {
  return probe_gemv_xq(x, in_norm_w, eps, blob, epi, bias, residual, next_norm_w, out, xo_limbs, xo_u, xo_sx, ssq_out,
                       stream, nullptr);
}

WOQ_API int woq_probe_gemv_xq_tp(const float* x, const float* in_norm_w, float eps, const void* blob, int epi,
                                 const float* bias, const float* residual, const float* next_norm_w, float* out,
                                 void* xo_limbs, float* xo_u, float* xo_sx, float* ssq_out, void* stream,
                                 woq_comm* comm) {
  if (comm == nullptr) return woq::fail("QBits: the tensor-parallel XQ GEMV probe needs a communicator");
  return probe_gemv_xq(x, in_norm_w, eps, blob, epi, bias, residual, next_norm_w, out, xo_limbs, xo_u, xo_sx, ssq_out,
                       stream, comm);
}

}  // extern "C"
