// woq_kv_shift.hip — the rolling KV cache's shift (StreamingLLM, reference docs/streamingllm.md: the first n_keep positions
// stay as attention sinks, the n_discard positions after them are dropped, generation goes on with positions counted
// inside the cache). For one sequence, every layer and every p in [n_keep + n_discard, n_cached):
//   V[p - n_discard] = V[p]                                            (bit copy)
//   K[p - n_discard] = K[p] rotated back by the angle of n_discard     (HF rotate_half pairing d, d + D/2)
//     a = K[p][d], b = K[p][d + D/2], c = cos[n_discard][d], s = sin[n_discard][d]   (exact from the cache type / fp32)
//     K[p - n_discard][d] = a * c + b * s,  K[p - n_discard][d + D/2] = b * c - a * s   (kv_store8's rounding)
//   The two products and their sum run in fp64 (each product of an at most 11-bit value with an fp32 one is exact there),
//   the sum is rounded to fp32 and kv_store8 rounds that to the cache type. Plain fp32 would do for fp16 and e4m3, whose
//   smallest steps are absolute; a bf16 step shrinks with the value, so where a * c and b * s cancel an fp32 sum is
//   several bf16 steps off (tests/test_kv_shift_cpu.py measures 2 on standard-normal rows). The kernel moves bytes and
//   waits for memory; the fp64 rate does not show.
// RoPE is a rotation, so a row the append kernels wrote at position p becomes the row of position p - n_discard, up to
// one more rounding to the cache type. The table row is the engine's own (woq_engine_set_head).
//
// Why the in-place move cannot race. Row r is the destination of row r + n_discard and the source of row r - n_discard,
// so a grid that hands ROWS to workgroups would need an order between workgroups. This kernel hands out COLUMNS instead:
// a thread owns a fixed set of columns of one layer — one 16-byte chunk of the row for V, one 8-element chunk of a head
// and its partner chunk D/2 further for K (the two halves a rotation mixes) — and walks the positions in ascending order
// by itself. No other thread ever reads or writes those columns, so nothing between threads, waves or workgroups needs
// ordering. Inside the thread, rows p .. p + AHEAD - 1 are loaded before rows p - n_discard .. are stored: every store
// goes to a row that thread has already loaded (or, below n_keep + n_discard, never loads), and a later load reads a
// higher row than any store so far has written. That is plain program order of one thread on its own addresses, which
// the pointers (no __restrict__: source and destination alias) make the compiler keep and the hardware guarantees.
// Several loads are in flight because loads only ever run ahead of stores.
//
// Cost: few threads (layers * kv_heads * D / 16 for K, twice that for V: 8192 + 16384 at the Llama-2-7B shape), each
// streaming its columns; a shift happens once per n_discard tokens (profiles/r12_streaming_kv.txt).
#include "woq_device.h"
#include "woq_host.h"
#include "woq_kv_codec.h"

namespace woq {
namespace {

constexpr int SHIFT_THREADS = 256;
constexpr int SHIFT_K_AHEAD = 8;   // rows a K thread loads (two 8-element chunks each) before it stores them
constexpr int SHIFT_V_AHEAD = 16;  // rows a V thread loads (16 bytes each) before it stores them

struct KvShiftArgs {
  uint8_t *k, *v;        // the sequence's caches, [layer][position][kv_heads * D] in the cache type
  const float *cs, *sn;  // row n_discard of the cos / sin tables, fp32 [D / 2]
  int layers, kv_heads, D, max_ctx;
  int first, n_cached, n_discard;  // first = n_keep + n_discard: the lowest source row
};

// rows p .. p + N - 1 of one K thread's two chunks: all loads, then rotate and store n_discard rows lower
template <int KVD, int N>
__device__ __forceinline__ void shift_k_rows(void* kc, size_t lo0, size_t row, int half, int p, int nd, const double (&c)[8],
                                             const double (&s)[8]) {
  float a[N][8], b[N][8];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const size_t at = lo0 + (size_t)(p + u) * row;
    kv_load8_f32<KVD>(kc, at, a[u]);
    kv_load8_f32<KVD>(kc, at + half, b[u]);
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    float lo[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double aj = (double)a[u][j], bj = (double)b[u][j];
      lo[j] = (float)(aj * c[j] + bj * s[j]);
      hi[j] = (float)(bj * c[j] - aj * s[j]);
    }
    const size_t at = lo0 + (size_t)(p + u - nd) * row;
    kv_store8<KVD>(kc, at, lo);
    kv_store8<KVD>(kc, at + half, hi);
  }
}

template <int N>
__device__ __forceinline__ void shift_v_rows(uint8_t* vc, size_t at0, size_t row_bytes, int p, int nd) {
  u32x4 w[N];
#pragma unroll
  for (int u = 0; u < N; ++u) w[u] = *(const u32x4*)(vc + at0 + (size_t)(p + u) * row_bytes);
#pragma unroll
  for (int u = 0; u < N; ++u) *(u32x4*)(vc + at0 + (size_t)(p + u - nd) * row_bytes) = w[u];
}

// blockIdx.y == 0: K threads, one per (layer, kv head, 8-element chunk of the head's first half);
// blockIdx.y == 1: V threads, one per (layer, 16-byte chunk of the row). See the file comment for why this is ordered.
template <int KVD>
__global__ __launch_bounds__(SHIFT_THREADS) void kv_shift_kernel(const KvShiftArgs g) {
  const int t = blockIdx.x * SHIFT_THREADS + threadIdx.x;
  const size_t row = (size_t)g.kv_heads * g.D;  // elements of one position
  if (blockIdx.y == 0) {
    const int per_head = g.D / 16, per_layer = g.kv_heads * per_head;
    if (t >= g.layers * per_layer) return;
    const int l = t / per_layer, h = (t % per_layer) / per_head, ch = t % per_head;
    const int half = g.D / 2;
    const size_t lo0 = (size_t)l * g.max_ctx * row + (size_t)h * g.D + 8 * ch;  // the chunk's element in row 0
    double c[8], s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = (double)g.cs[8 * ch + j], s[j] = (double)g.sn[8 * ch + j];
    int p = g.first;
    for (; p + SHIFT_K_AHEAD <= g.n_cached; p += SHIFT_K_AHEAD)
      shift_k_rows<KVD, SHIFT_K_AHEAD>(g.k, lo0, row, half, p, g.n_discard, c, s);
    for (; p < g.n_cached; ++p) shift_k_rows<KVD, 1>(g.k, lo0, row, half, p, g.n_discard, c, s);
  } else {
    const size_t row_bytes = row * (KVD == WOQ_FP8_E4M3 ? 1 : 2);
    const int per_layer = (int)(row_bytes / 16);
    if (t >= g.layers * per_layer) return;
    const int l = t / per_layer, ch = t % per_layer;
    const size_t at0 = (size_t)l * g.max_ctx * row_bytes + (size_t)16 * ch;
    int p = g.first;
    for (; p + SHIFT_V_AHEAD <= g.n_cached; p += SHIFT_V_AHEAD) shift_v_rows<SHIFT_V_AHEAD>(g.v, at0, row_bytes, p, g.n_discard);
    for (; p < g.n_cached; ++p) shift_v_rows<1>(g.v, at0, row_bytes, p, g.n_discard);
  }
}

// the two device words of a shift that also moves the chain: the next step feeds position n_cached - n_discard, and the
// sampled tail's Philox counter (position + discarded) goes on counting
__global__ void kv_shift_words_kernel(int32_t* pos, int32_t* discarded, int n_discard) {
  pos[0] -= n_discard;
  discarded[0] = (int32_t)((uint32_t)discarded[0] + (uint32_t)n_discard);
}
__global__ void i32_store_kernel(int32_t* dst, int32_t v) { dst[0] = v; }

}  // namespace

int launch_kv_shift(void* kseq, void* vseq, int kv_dtype, int layers, int kv_heads, int D, int max_ctx, const float* cs,
                    const float* sn, int n_keep, int n_discard, int n_cached, hipStream_t st) {
  const int first = n_keep + n_discard;
  if (kseq == nullptr || vseq == nullptr || cs == nullptr || sn == nullptr || layers < 1 || kv_heads < 1 || D < 16 ||
      (D % 16) != 0 || n_keep < 0 || n_discard < 1 || first > n_cached || n_cached > max_ctx)
    return fail("QBits: bad KV shift geometry");
  if (first == n_cached) return 0;  // nothing moves (and row n_discard of the tables may not exist: n_discard == max_ctx)
  const int es = kv_dtype == WOQ_FP8_E4M3 ? 1 : 2;
  const long long k_threads = (long long)layers * kv_heads * (D / 16);
  const long long v_threads = (long long)layers * ((long long)kv_heads * D * es / 16);
  const long long most = k_threads > v_threads ? k_threads : v_threads;
  if (most > 0x7fffffffll - SHIFT_THREADS) return fail("QBits: KV shift: the cache has too many columns for one launch");
  const KvShiftArgs g = {(uint8_t*)kseq, (uint8_t*)vseq, cs + (size_t)n_discard * (D / 2), sn + (size_t)n_discard * (D / 2),
                         layers, kv_heads, D, max_ctx, first, n_cached, n_discard};
  const dim3 grid((unsigned)((most + SHIFT_THREADS - 1) / SHIFT_THREADS), 2);
  switch (kv_dtype) {
    case WOQ_F16: hipLaunchKernelGGL(kv_shift_kernel<WOQ_F16>, grid, dim3(SHIFT_THREADS), 0, st, g); break;
    case WOQ_BF16: hipLaunchKernelGGL(kv_shift_kernel<WOQ_BF16>, grid, dim3(SHIFT_THREADS), 0, st, g); break;
    case WOQ_FP8_E4M3: hipLaunchKernelGGL(kv_shift_kernel<WOQ_FP8_E4M3>, grid, dim3(SHIFT_THREADS), 0, st, g); break;
    default: return fail("QBits: kv_dtype must be fp16, bf16 or fp8_e4m3");
  }
  return 0;
}

void launch_kv_shift_words(int32_t* pos, int32_t* discarded, int n_discard, hipStream_t st) {
  hipLaunchKernelGGL(kv_shift_words_kernel, dim3(1), dim3(1), 0, st, pos, discarded, n_discard);
}

void launch_i32_store(int32_t* dst, int32_t v, hipStream_t st) {
  hipLaunchKernelGGL(i32_store_kernel, dim3(1), dim3(1), 0, st, dst, v);
}

}  // namespace woq
