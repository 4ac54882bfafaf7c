// woq_moe_bwd.hip — backward of the routed expert block (woq_moe.hip states the forward) with respect to its rows and
// its routing weights, through frozen quantised experts. Per routed slot s = (t, j), e = idx[t][j]:
//
//     forward   [g | u] = x_t Wgu_e      h = SiLU(g) * u      y_s = h Wd_e      out_t = sum_j w[t][j] y_s
//     backward  dh'_s = dOut_t Wd_e^T                                   (summed over H, I columns)
//               dw[t][j] = <dh'_s, h_s>                                 (= <dOut_t, y_s>: y is never needed)
//               dh = w[t][j] dh'     dg = dh * u * SiLU'(g)     du = dh * SiLU(g)
//               dx_s = [dg | du] Wgu_e^T                                (summed over 2 I, H columns)
//               dX_t = sum_j dx_s, j ascending; a dropped slot (id outside [0, E)) adds zero and has dw = 0
//
// Nine launches shaped by (T, top_k, E, hidden, inter) alone; the host never learns the routing. No floating-point
// atomics, every sum in a fixed order: the same inputs give the same bytes.
//  1-3  plan: woq_moe_prompt.hip's count, scan and scatter (launch_moe_prompt_plan) -> sorted[], pos_of[], the table of
//       blocks {expert, first, rows <= 128}. Not a second plan.
//  4    pack (moe_bwd_pack_kernel): image row p = dOut row sorted[p] / top_k times an exact power of two 2^-e[p] (row
//       max into [2^13, 2^14)), rounded once to fp16: the dense pack pass (woq_bwd_tile.h bwd_pack_row) plus the gather.
//       Rows from the last valid slot to S + 128 are zeros: block b reads rows first .. first + 127 whatever its `rows`.
//       Its last workgroups find max |scale| over ALL experts' scale sections, one word per blob kind (an integer atomic
//       max): 2^E is one power of two per kind, not per expert. One E keeps the kernel free of a per-block word, and the
//       experts of one layer are quantised from weights of one scale; an expert whose scales lie 2^14 below the largest
//       of its layer would lose relative-scale bits to fp16 — the same exposure the dense kernel has inside one blob.
//       The word comes from the FIRST plane's scale section, as in the dense kernel: for an int8 composite that is the HI
//       plane, whose scales are 16 x the LO plane's, so it bounds both. Limit, stated and not refused (finding it would
//       take a second sweep and a host read): a scale s with |s| 2^-E < 2^-24 rounds to fp16 zero and its group
//       contributes nothing to the gradient; from 2^-14 down it keeps fewer than 11 bits. That is a group 2^14 ..
//       2^24 times smaller than the largest of all experts of its kind; tests/moe_backward_reference.py charges it
//       through the 2^-22 n max|dY| max|W| term, taken over all experts.
//  5    recompute of g and u: moe_prompt_gemm_kernel with its RAW epilogue (launch_moe_prompt_product, MOE_GATE_UP_RAW)
//       -> fp32 [sorted slot][2 I]. Always this product, whatever form served the forward: nothing but the call's inputs is kept.
//  6    product 1 (moe_bwd_product_kernel over the down blobs) -> dh' fp32 [sorted slot][I].
//  7    activation backward (moe_bwd_act_kernel), a workgroup per sorted row: dw reduced in a fixed order (a thread's
//       chunks ascending, the xor butterfly of a wave, the four waves as (0 + 1) + (2 + 3)) and stored through the slot
//       index; dg and du formed in fp32, the row maximum, and [dg | du] written directly as the fp16 image + row scale of
//       product 2 (two sweeps, the second finds the row in L2): dgu never exists in fp32 in memory. The workgroup of
//       index s < S also stores dw = 0 for slot s when it is dropped.
//  8    product 2 (the same kernel over the gate/up blobs) -> dx fp32 [sorted slot][H].
//  9    combine (moe_bwd_combine_kernel): dX_t = sum_j dx[pos_of[t k + j]], rounded once to the output type. Not
//       launch_moe_combine: unit weights would need a [T, k] array of ones in memory and a multiply per term.
//  (+ one 8-byte memset of the two scale-max words, as the dense backward has.)
//
// The grouped transposed product. A workgroup of four waves takes one table block (<= 128 rows of one expert) by 128
// output columns = one blob K tile of THAT expert (blobs + expert stride + plane offset), and runs woq_bwd_tile.h's
// bwd_tile, the n loop the dense backward runs: steps of 64 over the summed dimension, each wave streaming one 1-KiB
// blob tile a step, dequantising it into the swizzled [n][k] fp16 LDS image (two stages of 16 KiB, loads requested two
// steps ahead) and reading it back with ds_read_b64_tr_b16 in four fenced phases into v_mfma_f32_16x16x32_f16, fp32
// accumulation, both nibble planes of an int8 composite in one chain. LDS: 32 KiB of image + 64 B of table; the row
// operand goes from the packed image straight to registers. What differs from the dense kernel:
//  * rows are in sorted-slot order: wave w reads image rows first + 32 w .. + 31. Rows past `rows` are another expert's
//    (or the zero padding); they are multiplied and never stored. A row of the product depends on its own row of the
//    image alone, so nothing of them reaches a stored element;
//  * a workgroup past *nblocks returns before the loop, whole: EXEC is all ones at every transposed read;
//  * no act-order (moe_header_problem refuses such blobs), fp32 stores (the next stage reads them), epilogue factor
//    2^e[row] 2^E with the kind's E;
//  * workgroup ids map plainly: x = column tile, y = table block. The dense kernel's XCD-aware 8 x 8 super-tiles were
//    not measured here and are left out: a block's column tiles all read the same 128 image rows and the blocks of one
//    expert the same blob, which neighbouring ids already share.
//
// Measured (MI355X, int4 sym g128, bf16 gradients, medians of the whole call, profiles/r27_moe_backward.txt), T = 256 /
// 1024 / 4096: Mixtral-8x7B expert shape 1.50 / 3.35 / 13.1 ms against 9.85 / 11.3 / 15.1 ms for per-expert dequantise ->
// bf16 matmuls under autograd; Qwen3-30B-A3B shape 0.86 / 1.03 / 3.52 ms against 61 / 60 / 61 ms. Product kernel 198
// VGPRs (190 for the table types), no scratch, two workgroups per CU. Open: per-kernel times were not taken; the lead
// over the torch arm shrinks with T as the dense kernel's does (1.16x at the Mixtral shape at 4096), for the reasons its
// header gives (dequantisation on the critical path of a step); blocks of few rows (E = 128) still pay a whole 128-row
// tile; the plain workgroup mapping against the dense kernel's super-tiles; gu could be kept in fp16 to halve its scratch.
//
// Workspace (woq_moe_backward_workspace), S = T top_k, P = S + 128, r256 = rounded up to 256:
//     moe_prompt_plan_bytes(T, top_k, E)                      the plan tables
//   + 2 P ru64(H) + 2 P ru64(2 I)                             the two fp16 images
//   + 2 r256(4 P)                                             their row scales
//   + 256                                                     the two scale-max words
//   + r256(4 S 2 I) + r256(4 S I) + r256(4 S H)               gu, dh', dx in fp32
// It grows with T k (H + I) and never holds an image of a weight.
#include <string>

#include "woq_bwd_tile.h"
#include "woq_host.h"

namespace woq {
namespace {

// one kind of expert blobs as the product walks it: plane offsets relative to an expert's blob (int8 composite: HI then LO)
struct MoeBwdBlob {
  const uint8_t* blobs;
  size_t stride, off_q[2], off_scale[2], off_zp[2];  // off_zp 0: the plane is symmetric
  BwdGeom geom;  // ldp = N rounded up to 64
  int K, N;
  uint32_t weight_type;
  size_t n_scale;  // elements of the first plane's scale section
};

struct MoeBwdPackArgs {
  const void* g;  // dOut [T][ldg]
  int g_dtype, ldg, g_vec, top_k, H, rows;  // rows = S + 128 image rows
  const int32_t* sorted;
  const MoeBlock* blocks;
  const int32_t* nblocks;
  _Float16* gp;
  float* rs;
  int ldp;
  MoeBwdBlob w[2];  // down, gate/up: their scale sections
  int E, scale_blocks;
  unsigned int* smax;  // [2]
};

// sorted positions that hold a slot: the blocks cover [0, valid) in order
__device__ __forceinline__ int moe_bwd_valid(const MoeBlock* blocks, const int32_t* nblocks) {
  const int nb = *nblocks;
  return nb > 0 ? blocks[nb - 1].first + blocks[nb - 1].rows : 0;
}

// Blocks [0, rows): one workgroup per image row. Blocks beyond: scale_blocks per blob kind, max |scale| over all experts.
template <int DT>
__global__ __launch_bounds__(256) void moe_bwd_pack_kernel(const MoeBwdPackArgs a) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= a.rows) {
    const int j = (int)blockIdx.x - a.rows, kind = j / a.scale_blocks, sb = j - kind * a.scale_blocks;
    const MoeBwdBlob& w = a.w[kind];
    float mx = 0.f;
    for (int e = 0; e < a.E; ++e)
      mx = bwd_scale_sweep(w.blobs + (size_t)e * w.stride + w.off_scale[0], w.geom.scale_type, w.n_scale,
                           (size_t)sb * 256 + tid, (size_t)a.scale_blocks * 256, mx);
    bwd_scale_publish(mx, a.smax + kind);
    return;
  }
  const int r = blockIdx.x;
  _Float16* dst = a.gp + (size_t)r * a.ldp;
  if (r >= moe_bwd_valid(a.blocks, a.nblocks)) {
    bwd_pack_zero_row(dst, a.ldp, a.rs + r);
    return;
  }
  const int t = a.sorted[r] / a.top_k;
  bwd_pack_row<DT>(a.g, (size_t)t * a.ldg, a.H, a.g_vec != 0, dst, a.ldp, a.rs + r, red);
}

struct MoeBwdProductArgs {
  MoeBwdBlob w;
  const _Float16* gp;  // [S + 128][w.geom.ldp]
  const float* rs;
  const unsigned int* smax;
  const MoeBlock* blocks;
  const int32_t* nblocks;
  float* out;  // [sorted slot][ldo]
  int ldo;
};

template <bool TABLE>
__global__ __launch_bounds__(256, 2) void moe_bwd_product_kernel(const MoeBwdProductArgs a) {
  __shared__ __attribute__((aligned(1024))) unsigned char sm[2 * BWD_STAGE];
  __shared__ float lut_s[16];
  const int b = (int)blockIdx.y, kb = (int)blockIdx.x;
  if (b >= *a.nblocks) return;  // whole workgroups: no wave reaches the loop with a partial EXEC
  const MoeBlock blk = a.blocks[b];
  const int expert = __builtin_amdgcn_readfirstlane(blk.expert), first = __builtin_amdgcn_readfirstlane(blk.first);
  const int R = __builtin_amdgcn_readfirstlane(blk.rows);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;
  if (TABLE && tid < 16) lut_s[tid] = lut_value(a.w.weight_type, tid);

  const uint8_t* blob = a.w.blobs + (size_t)expert * a.w.stride;
  BwdPlane pl[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    pl[p].q = (const u32x4*)(blob + a.w.off_q[p]);
    pl[p].scales = blob + a.w.off_scale[p];
    pl[p].zp = a.w.off_zp[p] != 0 ? blob + a.w.off_zp[p] : nullptr;
  }
  const int E = bwd_scale_exp(a.smax);
  const int ldp = a.w.geom.ldp, m0 = first + wid * 32;  // rows m0 .. m0 + 31 of the image: all below S + 128
  const _Float16* const arow[2] = {a.gp + (size_t)(m0 + i16) * ldp + kq * 8, a.gp + (size_t)(m0 + 16 + i16) * ldp + kq * 8};
  float4_t acc[2][8];
  bwd_tile<TABLE>(a.w.geom, pl, kb, arow, ldexpf(1.f, -E), sm, lut_s, acc);

  // epilogue: lane holds column i16 of fragment kf, rows 4 kq + i of fragment mf; only the block's own rows are stored
  const float upE = ldexpf(1.f, E);
#pragma unroll
  for (int mf = 0; mf < 2; ++mf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wid * 32 + mf * 16 + 4 * kq + i;
      if (row >= R) continue;
      const float f = a.rs[first + row] * upE;
      float* orow = a.out + (size_t)(first + row) * a.ldo;
#pragma unroll
      for (int kf = 0; kf < 8; ++kf) {
        const int k = kb * BWD_BK + kf * 16 + i16;
        if (k < a.w.K) orow[k] = acc[mf][kf][i] * f;
      }
    }
  }
}

struct MoeBwdActArgs {
  const float* dhp;  // dh' [sorted slot][I]
  const float* gu;   // [g | u] [sorted slot][2 I]
  const float* topk_w;
  const int32_t* sorted;
  const int32_t* pos_of;
  const MoeBlock* blocks;
  const int32_t* nblocks;
  int I, S, rows;  // rows = S + 128 image rows
  _Float16* gp;    // [rows][ldp]: [dg | du], zeros from 2 I on
  float* rs;
  int ldp;
  float* grad_w;  // [S] by slot, nullable
};

// eight columns c0 .. c0 + 7 of one row: dg, du and the row's part of <dh', h>
__device__ __forceinline__ float moe_bwd_act8(const float* d, const float* g, const float* u, int c0, float w,
                                              float (&dg)[8], float (&du)[8]) {
  const float4_t dv[2] = {*(const float4_t*)(d + c0), *(const float4_t*)(d + c0 + 4)};
  const float4_t gv[2] = {*(const float4_t*)(g + c0), *(const float4_t*)(g + c0 + 4)};
  const float4_t uv[2] = {*(const float4_t*)(u + c0), *(const float4_t*)(u + c0 + 4)};
  float dot = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float dj = dv[j >> 2][j & 3], gj = gv[j >> 2][j & 3], uj = uv[j >> 2][j & 3];
    const float sg = 1.0f / (1.0f + expf(-gj)), silu = gj * sg;
    dot = fmaf(dj, silu * uj, dot);
    const float dh = w * dj;
    dg[j] = dh * uj * (sg * (1.0f + gj * (1.0f - sg)));  // SiLU'(g) = sg (1 + g (1 - sg))
    du[j] = dh * silu;
  }
  return dot;
}

__global__ __launch_bounds__(256) void moe_bwd_act_kernel(const MoeBwdActArgs a) {
  __shared__ float red[4], sums[4];
  const int tid = threadIdx.x, r = blockIdx.x;
  if (a.grad_w != nullptr && tid == 0 && r < a.S && a.pos_of[r] < 0) a.grad_w[r] = 0.f;  // r as a slot: dropped
  _Float16* dst = a.gp + (size_t)r * a.ldp;
  if (r >= moe_bwd_valid(a.blocks, a.nblocks)) {
    bwd_pack_zero_row(dst, a.ldp, a.rs + r);
    return;
  }
  const int slot = a.sorted[r], I = a.I, chunks = I >> 3;  // I % 16 == 0
  const float w = a.topk_w[slot];
  const float* d = a.dhp + (size_t)r * I;
  const float* g = a.gu + (size_t)r * 2 * I;
  const float* u = g + I;
  float amax = 0.f, dot = 0.f;
  for (int c = tid; c < chunks; c += 256) {
    float dg[8], du[8];
    dot += moe_bwd_act8(d, g, u, 8 * c, w, dg, du);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fmaxf(fabsf(dg[j]), fabsf(du[j])));
  }
  dot = wave_sum(dot);
  if ((tid & 63) == 0) sums[tid >> 6] = dot;
  amax = bwd_block_max(amax, red);  // its barrier publishes sums too
  if (a.grad_w != nullptr && tid == 0) a.grad_w[slot] = (sums[0] + sums[1]) + (sums[2] + sums[3]);
  const int e = bwd_row_exp(amax);
  const float p2 = ldexpf(1.f, -e);
  if (tid == 0) a.rs[r] = ldexpf(1.f, e);
  for (int c = tid; c < chunks; c += 256) {
    float dg[8], du[8];
    moe_bwd_act8(d, g, u, 8 * c, w, dg, du);
    h8 og, ou;
#pragma unroll
    for (int j = 0; j < 8; ++j) og[j] = (_Float16)(dg[j] * p2), ou[j] = (_Float16)(du[j] * p2);
    *(h8*)(dst + 8 * c) = og;
    *(h8*)(dst + I + 8 * c) = ou;
  }
  const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = 2 * chunks + tid; c < (a.ldp >> 3); c += 256) *(h8*)(dst + 8 * c) = zero;
}

__global__ __launch_bounds__(256) void moe_bwd_combine_kernel(const float* __restrict__ dx, const int32_t* __restrict__ pos_of,
                                                              int top_k, int H, void* __restrict__ out, int out_dtype,
                                                              int ldo) {
  const int t = (int)blockIdx.y, n = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (n >= H) return;
  float acc = 0.f;
  for (int j = 0; j < top_k; ++j) {
    const int p = pos_of[t * top_k + j];
    if (p >= 0) acc += dx[(size_t)p * H + n];  // a dropped slot contributes zero
  }
  store_f32(out, (size_t)t * ldo + n, out_dtype, acc);
}

MoeBwdBlob moe_bwd_blob(const void* blobs, const woq_blob_header& hdr, size_t stride) {  // hdr has passed moe_header_problem
  MoeBwdBlob w = {};
  w.blobs = (const uint8_t*)blobs, w.stride = stride;
  woq_blob_header h = hdr;
  if (hdr.weight_type == WOQ_W_INT8) {  // the dense backward's reading of the composite: each plane under its own scales
    woq_blob_header o, hi, lo;
    woq_int8_headers(&o, &hi, &lo, hdr.K, hdr.N, hdr.group, hdr.scale_type, hdr.compute_type, hdr.off_zp != 0, 0);
    w.off_q[0] = hdr.off_q + hi.off_q, w.off_scale[0] = hdr.off_q + hi.off_scale;
    w.off_zp[0] = hi.off_zp ? hdr.off_q + hi.off_zp : 0;
    w.off_q[1] = hdr.off_scale + lo.off_q, w.off_scale[1] = hdr.off_scale + lo.off_scale;
    w.off_zp[1] = lo.off_zp ? hdr.off_scale + lo.off_zp : 0;
    w.geom.planes = 2;
    h = hi;
  } else {
    for (int p = 0; p < 2; ++p) w.off_q[p] = h.off_q, w.off_scale[p] = h.off_scale, w.off_zp[p] = h.off_zp;
    w.geom.planes = 1;
  }
  w.K = h.K, w.N = h.N, w.weight_type = h.weight_type;
  w.geom.tiles_k = h.Kpad / 128, w.geom.tiles_n = h.Npad / 16, w.geom.n_groups = h.n_groups, w.geom.group = h.group;
  w.geom.scale_type = (int)h.scale_type, w.geom.scale_mode = (int)h.scale_mode;
  w.geom.ldp = (int)woq_round_up((size_t)h.N, BWD_BN);
  w.n_scale = h.scale_mode == 0 ? (size_t)w.geom.tiles_n * h.n_groups * 16 : (size_t)w.geom.tiles_n * w.geom.tiles_k * 64;
  return w;
}

struct MoeBwdWorkspace {
  size_t img1, img2, rs1, rs2, smax, gu, dhp, dx, total;  // byte offsets (the plan tables lie at 0), and the size
};
MoeBwdWorkspace moe_bwd_ws(int T, int top_k, int E, int hidden, int inter) {
  const size_t S = (size_t)T * top_k, P = S + BWD_BM;
  MoeBwdWorkspace w;
  w.img1 = moe_prompt_plan_bytes(T, top_k, E);  // a multiple of 256, and so is every image (ld a multiple of 64)
  w.img2 = w.img1 + P * woq_round_up((size_t)hidden, BWD_BN) * 2;
  w.rs1 = w.img2 + P * woq_round_up((size_t)2 * inter, BWD_BN) * 2;
  w.rs2 = w.rs1 + woq_round_up(P * 4, 256);
  w.smax = w.rs2 + woq_round_up(P * 4, 256);
  w.gu = w.smax + 256;
  w.dhp = w.gu + woq_round_up(S * 2 * inter * 4, 256);
  w.dx = w.dhp + woq_round_up(S * inter * 4, 256);
  w.total = w.dx + woq_round_up(S * hidden * 4, 256);
  return w;
}

bool moe_bwd_shape_ok(int T, int top_k, int E, int hidden, int inter) {
  return T > 0 && T <= 65535 && top_k > 0 && E > 0 && hidden > 0 && inter > 0 && E <= MOE_MAX_EXPERTS &&
         (long long)T * top_k <= MOE_BACKWARD_MAX_SLOTS;  // T: the combine's grid has a workgroup row per token
}

void moe_bwd_launch_product(const MoeBwdProductArgs& a, int max_blocks, hipStream_t st) {
  const dim3 grid((unsigned)a.w.geom.tiles_k, (unsigned)max_blocks);
  if (is_table_type(a.w.weight_type))
    hipLaunchKernelGGL(moe_bwd_product_kernel<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(moe_bwd_product_kernel<false>, grid, dim3(256), 0, st, a);
}

}  // namespace
}  // namespace woq

extern "C" size_t woq_moe_backward_workspace(int T, int top_k, int E, int hidden, int inter) {
  if (!woq::moe_bwd_shape_ok(T, top_k, E, hidden, inter)) return 0;
  return woq::moe_bwd_ws(T, top_k, E, hidden, inter).total;
}

extern "C" int woq_moe_backward(const void* grad_out_dev, int grad_dtype, int ldg, const void* x_dev, int x_dtype, int ldx,
                                const void* topk_idx_dev, int idx_is_int64, const float* topk_w_dev, int T, int top_k, int E,
                                const void* gate_up_blobs_dev, const woq_blob_header* gate_up_hdr, size_t gate_up_stride,
                                const void* down_blobs_dev, const woq_blob_header* down_hdr, size_t down_stride,
                                void* grad_x_dev, int grad_x_dtype, int ldgx, float* grad_w_dev, void* workspace_dev,
                                size_t workspace_bytes, void* stream) {
  WOQ_TRY
  using namespace woq;
  auto fp8 = [](const woq_blob_header* h) { return h != nullptr && woq_weight_is_fp8(h->weight_type); };
  WOQ_CHECK(!fp8(gate_up_hdr) && !fp8(down_hdr),
            "QBits: woq_moe_backward: fp8 expert blobs are not built; they take the dequantise-and-matmul arm");
  WOQ_CHECK(grad_dtype == WOQ_F32 || grad_dtype == WOQ_BF16 || grad_dtype == WOQ_F16, "QBits: unsupported qbits data type.");
  if (T > 0) {  // (a call of no rows returns 0 from the shared checks, whatever its pointers)
    WOQ_CHECK(grad_out_dev, "QBits: woq_moe_backward: null tensor");
    WOQ_CHECK(!down_hdr || ldg >= down_hdr->N, "QBits: woq_moe_backward: leading dimension smaller than hidden");
  }
  MoeCall m = {x_dev, x_dtype, ldx, topk_idx_dev, idx_is_int64 != 0, topk_w_dev, T, top_k, E,
               gate_up_blobs_dev, gate_up_hdr, gate_up_stride, down_blobs_dev, down_hdr, down_stride,
               grad_x_dev, grad_x_dtype, ldgx, workspace_dev};
  static const MoeEntry entry = {"woq_moe_backward", woq_moe_backward_workspace, "woq_moe_backward_workspace",
                                 MOE_BACKWARD_MAX_SLOTS, 256};  // (its workspace function also holds T to 65535)
  if (const int rc = moe_entry_checks(entry, m, workspace_bytes)) return rc < 0 ? 0 : rc;
  const int H = down_hdr->N, I = down_hdr->K;
  const MoeBwdWorkspace w = moe_bwd_ws(T, top_k, E, H, I);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace_dev;
  const int S = T * top_k, P = S + BWD_BM;
  const MoeRoutePlan plan = moe_plan_tables(MOE_PROMPT, ws, T, top_k, E);
  unsigned int* smax = (unsigned int*)(ws + w.smax);
  float* gu = (float*)(ws + w.gu);
  float* dhp = (float*)(ws + w.dhp);
  float* dx = (float*)(ws + w.dx);

  launch_moe_prompt_plan(topk_idx_dev, idx_is_int64 != 0, S, E, plan, st);
  WOQ_HIP(hipMemsetAsync(smax, 0, 2 * sizeof(unsigned int), st));

  MoeBwdPackArgs pk = {};
  pk.g = grad_out_dev, pk.g_dtype = grad_dtype, pk.ldg = ldg, pk.top_k = top_k, pk.H = H, pk.rows = P;
  pk.g_vec = ((uintptr_t)grad_out_dev % 16 == 0 && ((size_t)ldg * woq_dtype_size((uint32_t)grad_dtype)) % 16 == 0) ? 1 : 0;
  pk.sorted = plan.sorted, pk.blocks = plan.blocks, pk.nblocks = plan.nblocks;
  pk.w[0] = moe_bwd_blob(down_blobs_dev, *down_hdr, down_stride);
  pk.w[1] = moe_bwd_blob(gate_up_blobs_dev, *gate_up_hdr, gate_up_stride);
  pk.gp = (_Float16*)(ws + w.img1), pk.rs = (float*)(ws + w.rs1), pk.ldp = pk.w[0].geom.ldp;
  pk.E = E, pk.smax = smax;
  pk.scale_blocks = (int)std::min<size_t>(128, (std::max(pk.w[0].n_scale, pk.w[1].n_scale) + 1023) / 1024);
  const dim3 pgrid((unsigned)(P + 2 * pk.scale_blocks));
  if (grad_dtype == WOQ_F32)
    hipLaunchKernelGGL(moe_bwd_pack_kernel<WOQ_F32>, pgrid, dim3(256), 0, st, pk);
  else if (grad_dtype == WOQ_BF16)
    hipLaunchKernelGGL(moe_bwd_pack_kernel<WOQ_BF16>, pgrid, dim3(256), 0, st, pk);
  else
    hipLaunchKernelGGL(moe_bwd_pack_kernel<WOQ_F16>, pgrid, dim3(256), 0, st, pk);

  if (const int rc = launch_moe_prompt_product(MOE_GATE_UP_RAW, m, plan, nullptr, gu, st)) return rc;

  MoeBwdProductArgs p1 = {};
  p1.w = pk.w[0], p1.gp = pk.gp, p1.rs = pk.rs, p1.smax = smax;
  p1.blocks = plan.blocks, p1.nblocks = plan.nblocks, p1.out = dhp, p1.ldo = I;
  moe_bwd_launch_product(p1, plan.max_blocks, st);

  MoeBwdActArgs ac = {};
  ac.dhp = dhp, ac.gu = gu, ac.topk_w = topk_w_dev, ac.sorted = plan.sorted, ac.pos_of = plan.pos_of;
  ac.blocks = plan.blocks, ac.nblocks = plan.nblocks, ac.I = I, ac.S = S, ac.rows = P;
  ac.gp = (_Float16*)(ws + w.img2), ac.rs = (float*)(ws + w.rs2), ac.ldp = pk.w[1].geom.ldp, ac.grad_w = grad_w_dev;
  hipLaunchKernelGGL(moe_bwd_act_kernel, dim3((unsigned)P), dim3(256), 0, st, ac);

  MoeBwdProductArgs p2 = {};
  p2.w = pk.w[1], p2.gp = ac.gp, p2.rs = ac.rs, p2.smax = smax + 1;
  p2.blocks = plan.blocks, p2.nblocks = plan.nblocks, p2.out = dx, p2.ldo = H;
  moe_bwd_launch_product(p2, plan.max_blocks, st);

  hipLaunchKernelGGL(moe_bwd_combine_kernel, dim3((unsigned)((H + 255) / 256), (unsigned)T), dim3(256), 0, st, dx,
                     plan.pos_of, top_k, H, grad_x_dev, grad_x_dtype, ldgx);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}
