// woq_ops.hip — the ops between the quantised linears, as gfx950 kernels.
//
// In the reference these are stock HF transformers module forwards run by PyTorch CPU ops
// (LlamaRMSNorm, apply_rotary_pos_emb, SiLU*mul in LlamaMLP, GPT-2 gelu_new);
// ITREX contributes no code there. All are HBM/latency-bound vector kernels: 16-byte loads, fp32 math,
// wave64 shuffles; no MFMA. Also here: the head (embedding row) and the token tail (lm_head, argmax) of the
// engine's decode step; its attention is woq_attn_decode.hip.
#include <algorithm>

#include "woq_device.h"
#include "woq_host.h"
#include "woq_xq.h"
#include "../../include/woq_hip_experimental.h"

namespace woq {

// ---- RMSNorm: one workgroup (256 threads) per row ------------------------------------------------
__global__ __launch_bounds__(256) void rmsnorm_kernel(const void* __restrict__ x, int dtype,
                                                      const float* __restrict__ w, float eps, int d,
                                                      void* __restrict__ out, int out_dtype) {
  __shared__ float part[4];
  const size_t row = blockIdx.x;
  const int tid = threadIdx.x;
  float ss = 0.f;
  for (int i = tid; i < d; i += 256) {
    float v = load_f32(x, row * d + i, dtype);
    ss = fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  if ((tid & 63) == 0) part[tid >> 6] = ss;
  __syncthreads();
  const float tot = part[0] + part[1] + part[2] + part[3];
  const float inv = 1.0f / sqrtf(tot / (float)d + eps);
  for (int i = tid; i < d; i += 256) {
    float v = load_f32(x, row * d + i, dtype);
    store_f32(out, row * d + i, out_dtype, v * inv * w[i]);
  }
}

// ---- RoPE (rotate_half), in place on [tokens, heads, D] -------------------------------------------
__global__ void rope_kernel(void* __restrict__ x, int dtype, const int32_t* __restrict__ pos,
                            const float* __restrict__ cs, const float* __restrict__ sn, int heads, int D,
                            size_t total_pairs) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total_pairs) return;
  const int half = D >> 1;
  const int i = (int)(idx % half);
  const size_t th = idx / half;  // token*heads + head
  const int t = (int)(th / heads);
  const int p = pos[t];
  const float c = cs[(size_t)p * half + i], s = sn[(size_t)p * half + i];
  const size_t base = th * D;
  const float a = load_f32(x, base + i, dtype), b = load_f32(x, base + i + half, dtype);
  store_f32(x, base + i, dtype, a * c - b * s);
  store_f32(x, base + i + half, dtype, b * c + a * s);
}

__global__ void silu_mul_kernel(const void* __restrict__ g, const void* __restrict__ u, int dtype, size_t n,
                                void* __restrict__ out) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; idx < n; idx += stride) {
    const float a = load_f32(g, idx, dtype), b = load_f32(u, idx, dtype);
    store_f32(out, idx, dtype, a / (1.0f + expf(-a)) * b);
  }
}

__global__ void gelu_kernel(const void* __restrict__ x, int dtype, size_t n, int approximate,
                            void* __restrict__ out) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; idx < n; idx += stride) {
    const float v = load_f32(x, idx, dtype);
    float r;
    if (approximate)
      r = 0.5f * v * (1.0f + tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v)));
    else
      r = 0.5f * v * (1.0f + erff(v * 0.7071067811865476f));
    store_f32(out, idx, dtype, r);
  }
}

// ---- engine kernels (batch-1 decode) --------------------------------------------------------------

// hidden[h] = embed[token][h]  (fp32 residual stream)
// xo (optional): the row also leaves as the first layer's XQ vector (times its input norm weight) with the per-block
// sums of squares — hidden % 16 == 0, so every 16-lane row is one whole block
__global__ void embed_kernel(const void* __restrict__ embed, int dtype, const int32_t* __restrict__ token, int hidden,
                             float* __restrict__ out, const float* __restrict__ norm_w, XqPtrs xo,
                             float* __restrict__ ssq_out, unsigned int* __restrict__ step_seq,
                             int32_t* __restrict__ pos, int max_ctx, int* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {  // first kernel of a decode step
    if (step_seq != nullptr) step_seq[0] = step_seq[0] + 1u;  // new hand-off tags
    // the position lives on the device (greedy chaining advances it there): the KV cache, the RoPE tables and the token
    // log are indexed by it unchecked, so a step that starts out of range is moved to the last slot and flagged
    if (pos != nullptr && pos[0] >= max_ctx) {
      pos[0] = max_ctx - 1;
      if (status != nullptr) atomicOr(status, 2);
    }
  }
  if (i < hidden) {
    const float v = load_f32(embed, (size_t)token[0] * hidden + i, dtype);
    out[i] = v;
    if (xo.limbs != nullptr) {
      const float ss = row16_sum(v * v);
      if ((i & 15) == 0) ssq_out[i >> 4] = ss;
      xq_emit16(v * norm_w[i], xo, i >> 4, i & 15);
    }
  }
}

// The greedy tail of step t and the head of step t + 1 in ONE launch (round 5; inside a graph of chained steps every
// interior token boundary was argmax [1 workgroup] -> boundary -> embed [hidden / 256 workgroups]): every workgroup
// reduces the lm_head's (max, index) pairs itself — vocab / 16 pairs, 8 per thread, the same tie rule (lowest index) in
// the same order everywhere, so all agree — and embeds its 256 columns of the winner's row; workgroup 0 also does the
// bookkeeping of both kernels (token, token log, position + 1, the new step's hand-off tag, the max_ctx guard).
__global__ __launch_bounds__(256) void argmax_embed_kernel(const float* __restrict__ pmax, const int32_t* __restrict__ pidx,
                                                           int n_pairs, int32_t* __restrict__ token,
                                                           int32_t* __restrict__ pos, int32_t* __restrict__ log,
                                                           const void* __restrict__ embed, int dtype, int hidden,
                                                           float* __restrict__ out, const float* __restrict__ norm_w,
                                                           XqPtrs xo, float* __restrict__ ssq_out,
                                                           unsigned int* __restrict__ step_seq, int max_ctx,
                                                           int* __restrict__ status) {
  __shared__ float bv[4];
  __shared__ int bi[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int i = tid; i < n_pairs; i += 256) {
    const float v = pmax[i];
    const int ci = pidx[i];
    if (v > best || (v == best && ci < idx)) best = v, idx = ci;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) best = ov, idx = oi;
  }
  if (lane == 0) bv[wid] = best, bi[wid] = idx;
  __syncthreads();
  best = bv[0], idx = bi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (bv[w] > best || (bv[w] == best && bi[w] < idx)) best = bv[w], idx = bi[w];
  // no candidate won (every logit NaN): the sentinel must not index the embedding table — token 0 and a status bit
  const bool no_winner = idx < 0 || (size_t)idx >= (size_t)n_pairs * 16;
  if (no_winner) idx = 0;
  if (blockIdx.x == 0 && tid == 0) {
    if (no_winner && status != nullptr) atomicOr(status, 4);
    token[0] = idx;
    int p = pos[0];
    if (log != nullptr) log[p] = idx;
    p += 1;
    if (step_seq != nullptr) step_seq[0] = step_seq[0] + 1u;
    if (p >= max_ctx) {  // the next step would start out of range: the embedding kernel's guard
      p = max_ctx - 1;
      if (status != nullptr) atomicOr(status, 2);
    }
    pos[0] = p;
  }
  const int i = blockIdx.x * 256 + tid;
  if (i < hidden) {
    const float v = load_f32(embed, (size_t)idx * hidden + i, dtype);
    out[i] = v;
    if (xo.limbs != nullptr) {
      const float ss = row16_sum(v * v);
      if ((i & 15) == 0) ssq_out[i >> 4] = ss;
      xq_emit16(v * norm_w[i], xo, i >> 4, i & 15);
    }
  }
}

// logits[v] = sum_h xn[h] * W[v][h], W dense fp16/bf16 [vocab, hidden] (lm_head is NOT quantised:
// utils/config.py:836-837). Final RMSNorm fused in the prologue. One wave per vocab row, 4 rows per WG.
__global__ __launch_bounds__(256) void lm_head_kernel(const float* __restrict__ hidden_in,
                                                      const float* __restrict__ norm_w, float eps,
                                                      const void* __restrict__ W, int w_dtype, int hidden, int vocab,
                                                      float* __restrict__ logits, float* __restrict__ pmax,
                                                      int32_t* __restrict__ pidx) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* xs = sm;  // [hidden]
  __shared__ float part[4];
  __shared__ float bestv[4];
  __shared__ int besti[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float wbest = -INFINITY;  // this wave's best (logit, row) — rows ascend, so '>' keeps the lowest index on ties
  int wbi = 0x7fffffff;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  float ss = 0.f;
  for (int i = tid; i < hidden; i += 256) {
    const float v = hidden_in[i];
    xs[i] = v;
    ss = fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  if (lane == 0) part[wid] = ss;
  __syncthreads();
  const float inv = 1.0f / sqrtf((part[0] + part[1] + part[2] + part[3]) / (float)hidden + eps);
  for (int i = tid; i < hidden; i += 256) xs[i] = xs[i] * inv * norm_w[i];
  __syncthreads();
  const int rows_per_wg = 16;
  auto consume = [&](const u32x4& raw, int k0, float& acc) {
    const uint32_t rr[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float lo, hi;
      if (w_dtype == WOQ_BF16) {
        lo = bf16_bits_to_f32(rr[j] & 0xffff);
        hi = bf16_bits_to_f32(rr[j] >> 16);
      } else {
        lo = f16_bits_to_f32(rr[j] & 0xffff);
        hi = f16_bits_to_f32(rr[j] >> 16);
      }
      acc = fmaf(lo, xs[k0 + 2 * j], acc);
      acc = fmaf(hi, xs[k0 + 2 * j + 1], acc);
    }
  };
  auto finish = [&](int v, float acc) {
    acc = wave_sum(acc);
    if (lane == 0) logits[v] = acc;
    if (acc > wbest) {
      wbest = acc;
      wbi = v;
    }
  };
  for (int r = wid; r < rows_per_wg; r += 4) {
    const int v = blockIdx.x * rows_per_wg + r;
    if (v >= vocab) break;
    const uint16_t* wr = (const uint16_t*)W + (size_t)v * hidden;
    float acc = 0.f;
    for (int k0 = lane * 8; k0 < hidden; k0 += 512) consume(__builtin_nontemporal_load((const u32x4*)(wr + k0)), k0, acc);
    finish(v, acc);
  }
  // per-workgroup (max, index) for the greedy argmax: it then reduces vocab / 16 pairs instead of vocab logits
  if (pmax) {
    if (lane == 0) {
      bestv[wid] = wbest;
      besti[wid] = wbi;
    }
    __syncthreads();
    if (tid == 0) {
      float b = bestv[0];
      int bi = besti[0];
      for (int w = 1; w < 4; ++w)
        if (bestv[w] > b || (bestv[w] == b && besti[w] < bi)) {
          b = bestv[w];
          bi = besti[w];
        }
      pmax[blockIdx.x] = b;
      pidx[blockIdx.x] = bi;
    }
  }
}

// greedy: token = argmax(logits) (lowest index on ties, like torch.argmax), pos += 1. One workgroup.
// `cand` null: candidate i is logit i; else (logits[i], cand[i]) are the per-workgroup pairs lm_head_kernel left.
// `log` (optional): log[position of the token that was just fed] = the new token, so a host that replays several steps
// back to back can read them all afterwards instead of synchronising on every step.
// No candidate won (every logit NaN or -inf): argmax_embed_kernel's rule — token 0 and status bit 2 — so that the
// sentinel never reaches the next step's embedding lookup and the eager and the chained tail agree.
__global__ __launch_bounds__(1024) void argmax_kernel(const float* __restrict__ logits, const int32_t* __restrict__ cand,
                                                      int vocab, int32_t* __restrict__ token,
                                                      int32_t* __restrict__ pos, int32_t* __restrict__ log,
                                                      int* __restrict__ status) {
  __shared__ float bv[16];
  __shared__ int bi[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int i = tid; i < vocab; i += 1024) {
    const float v = logits[i];
    const int ci = cand ? cand[i] : i;
    if (v > best || (v == best && ci < idx)) {
      best = v;
      idx = ci;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) {
      best = ov;
      idx = oi;
    }
  }
  if (lane == 0) {
    bv[wid] = best;
    bi[wid] = idx;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w)
      if (bv[w] > best || (bv[w] == best && bi[w] < idx)) {
        best = bv[w];
        idx = bi[w];
      }
    if (idx < 0 || (size_t)idx >= (cand ? (size_t)vocab * 16 : (size_t)vocab)) {
      idx = 0;
      if (status != nullptr) atomicOr(status, 4);
    }
    token[0] = idx;
    if (log != nullptr) log[pos[0]] = idx;
    pos[0] = pos[0] + 1;
  }
}

// ---- host launchers used by the engine ------------------------------------------------------------
void launch_embed(const void* embed, int dtype, const int32_t* token, int hidden, float* out, const float* norm_w,
                  const XqPtrs& xo, float* ssq_out, unsigned int* step_seq, int32_t* pos, int max_ctx, int* status,
                  hipStream_t st) {
  hipLaunchKernelGGL(embed_kernel, dim3((hidden + 255) / 256), dim3(256), 0, st, embed, dtype, token, hidden, out,
                     norm_w, xo, ssq_out, step_seq, pos, max_ctx, status);
}

void launch_lm_head(const float* hidden_in, const float* norm_w, float eps, const void* W, int w_dtype, int hidden,
                    int vocab, float* logits, float* pmax, int32_t* pidx, hipStream_t st) {
  hipLaunchKernelGGL(lm_head_kernel, dim3((vocab + 15) / 16), dim3(256), (size_t)hidden * 4, st, hidden_in, norm_w,
                     eps, W, w_dtype, hidden, vocab, logits, pmax, pidx);
}

void launch_argmax(const float* logits, int vocab, int32_t* token, int32_t* pos, hipStream_t st) {
  hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, st, logits, (const int32_t*)nullptr, vocab, token, pos,
                     (int32_t*)nullptr, (int*)nullptr);
}

void launch_argmax_pairs(const float* pmax, const int32_t* pidx, int n, int32_t* token, int32_t* pos, int32_t* log,
                         int* status, hipStream_t st) {
  hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, st, pmax, pidx, n, token, pos, log, status);
}

void launch_argmax_embed(const float* pmax, const int32_t* pidx, int n, int32_t* token, int32_t* pos, int32_t* log,
                         const void* embed, int dtype, int hidden, float* out, const float* norm_w, const XqPtrs& xo,
                         float* ssq_out, unsigned int* step_seq, int max_ctx, int* status, hipStream_t st) {
  hipLaunchKernelGGL(argmax_embed_kernel, dim3((hidden + 255) / 256), dim3(256), 0, st, pmax, pidx, n, token, pos, log,
                     embed, dtype, hidden, out, norm_w, xo, ssq_out, step_seq, max_ctx, status);
}

}  // namespace woq

using namespace woq;

// the element ops' load_f32 / store_f32 read every code that is not fp32 or bf16 as two-byte fp16
static bool elem_dtype_ok(int dt) { return dt == WOQ_F32 || dt == WOQ_F16 || dt == WOQ_BF16; }

extern "C" {

int woq_rmsnorm(const void* x_dev, int dtype, const float* weight_dev, float eps, int rows, int d, void* out_dev,
                int out_dtype, void* stream) {
  WOQ_TRY
  WOQ_CHECK(rows >= 0 && d > 0, "QBits: bad rmsnorm shape");
  WOQ_CHECK(elem_dtype_ok(dtype) && elem_dtype_ok(out_dtype), "QBits: rmsnorm takes fp32, fp16 or bf16 in and out");
  if (rows == 0) return 0;
  WOQ_CHECK(x_dev && weight_dev && out_dev, "QBits: rmsnorm: null x, weight or out");
  hipLaunchKernelGGL(rmsnorm_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x_dev, dtype, weight_dev, eps, d,
                     out_dev, out_dtype);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

int woq_rope(void* x_dev, int dtype, const int32_t* pos_dev, const float* cos_dev, const float* sin_dev, int tokens,
             int heads, int D, void* stream) {
  WOQ_TRY
  WOQ_CHECK((D & 1) == 0, "QBits: rope head_dim must be even");
  WOQ_CHECK(tokens >= 0 && heads >= 0 && D >= 0, "QBits: bad rope shape");
  WOQ_CHECK(elem_dtype_ok(dtype), "QBits: rope takes fp32, fp16 or bf16");
  size_t total = (size_t)tokens * heads * (D / 2);
  if (total == 0) return 0;
  WOQ_CHECK(x_dev && pos_dev && cos_dev && sin_dev, "QBits: rope: null x, pos, cos or sin");
  hipLaunchKernelGGL(rope_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_dev,
                     dtype, pos_dev, cos_dev, sin_dev, heads, D, total);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

int woq_silu_mul(const void* gate_dev, const void* up_dev, int dtype, size_t n, void* out_dev, void* stream) {
  WOQ_TRY
  WOQ_CHECK(elem_dtype_ok(dtype), "QBits: silu_mul takes fp32, fp16 or bf16");
  if (n == 0) return 0;
  WOQ_CHECK(gate_dev && up_dev && out_dev, "QBits: silu_mul: null gate, up or out");
  unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(silu_mul_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, gate_dev, up_dev, dtype, n,
                     out_dev);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

int woq_gelu(const void* x_dev, int dtype, size_t n, int approximate, void* out_dev, void* stream) {
  WOQ_TRY
  WOQ_CHECK(elem_dtype_ok(dtype), "QBits: gelu takes fp32, fp16 or bf16");
  if (n == 0) return 0;
  WOQ_CHECK(x_dev && out_dev, "QBits: gelu: null x or out");
  unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(gelu_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x_dev, dtype, n, approximate,
                     out_dev);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

// test entry points (include/woq_hip_experimental.h): the token tail's launches on caller-owned buffers
WOQ_API int woq_probe_lm_head(const float* hidden_in, const float* norm_w, float eps, const void* W, int w_dtype,
                              int hidden, int vocab, float* logits, float* pmax, int32_t* pidx, void* stream) {
  WOQ_TRY
  WOQ_CHECK(hidden_in && norm_w && W && logits && hidden >= 8 && (hidden & 7) == 0 && hidden <= 16384 && vocab >= 1,
            "QBits: bad lm_head probe arguments");
  WOQ_CHECK(w_dtype == WOQ_F16 || w_dtype == WOQ_BF16, "QBits: the lm_head is fp16 or bf16");
  WOQ_CHECK((pmax == nullptr) == (pidx == nullptr), "QBits: pmax and pidx come together");
  launch_lm_head(hidden_in, norm_w, eps, W, w_dtype, hidden, vocab, logits, pmax, pidx, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

WOQ_API int woq_probe_greedy_tail(int mode, const float* logits, int vocab, const float* pmax, const int32_t* pidx,
                                  int32_t* token, int32_t* pos, int32_t* log, const void* embed, int embed_dtype,
                                  int hidden, float* out, const float* norm_w, void* xo_limbs, float* xo_u, float* xo_sx,
                                  float* ssq_out, unsigned int* step_seq, int max_ctx, int* status, void* stream) {
  WOQ_TRY
  WOQ_CHECK(mode >= 0 && mode <= 2 && vocab >= 1 && token && pos, "QBits: bad greedy tail probe arguments");
  const hipStream_t st = (hipStream_t)stream;
  const int n_pairs = (vocab + 15) / 16;
  if (mode == 0) {
    WOQ_CHECK(logits != nullptr, "QBits: mode 0 reduces logits");
    launch_argmax(logits, vocab, token, pos, st);
  } else if (mode == 1) {
    WOQ_CHECK(pmax && pidx, "QBits: modes 1 and 2 reduce the lm_head's pairs");
    launch_argmax_pairs(pmax, pidx, n_pairs, token, pos, log, status, st);
  } else {
    WOQ_CHECK(pmax && pidx && embed && out && hidden >= 16 && (hidden & 15) == 0 && max_ctx >= 1,
              "QBits: mode 2 needs the pairs and an embedding table");
    WOQ_CHECK(embed_dtype == WOQ_F16 || embed_dtype == WOQ_BF16 || embed_dtype == WOQ_F32, "QBits: bad embedding type");
    WOQ_CHECK(xo_limbs == nullptr || (norm_w && xo_u && xo_sx && ssq_out), "QBits: an XQ output needs all of its parts");
    launch_argmax_embed(pmax, pidx, n_pairs, token, pos, log, embed, embed_dtype, hidden, out, norm_w,
                        XqPtrs{(uint8_t*)xo_limbs, xo_u, xo_sx}, ssq_out, step_seq, max_ctx, status, st);
  }
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

WOQ_API int woq_probe_embed(const void* embed, int embed_dtype, const int32_t* token, int hidden, float* out,
                            const float* norm_w, void* xo_limbs, float* xo_u, float* xo_sx, float* ssq_out,
                            unsigned int* step_seq, int32_t* pos, int max_ctx, int* status, void* stream) {
  WOQ_TRY
  WOQ_CHECK(embed && token && out && hidden >= 16 && (hidden & 15) == 0, "QBits: bad embed probe arguments");
  WOQ_CHECK(embed_dtype == WOQ_F16 || embed_dtype == WOQ_BF16 || embed_dtype == WOQ_F32, "QBits: bad embedding type");
  WOQ_CHECK(xo_limbs == nullptr || (norm_w && xo_u && xo_sx && ssq_out), "QBits: an XQ output needs all of its parts");
  launch_embed(embed, embed_dtype, token, hidden, out, norm_w, XqPtrs{(uint8_t*)xo_limbs, xo_u, xo_sx}, ssq_out,
               step_seq, pos, max_ctx, status, (hipStream_t)stream);
  WOQ_HIP(hipGetLastError());
  WOQ_END
}

}  // extern "C"
