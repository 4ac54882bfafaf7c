// woq_group_cols.h — the layout the per-group quantiser kernels run on: autoround_kernel (woq_autoround.hip),
// teq_kernel (woq_teq.hip) and, in its one-slice form, awq_scale_delta_kernel (woq_awq.hip).
//
// w is fp32 [K, N] row-major; a group is `group` consecutive rows of one column (the last may be short). A thread owns
// one column of one group (blockIdx.y) and makes a range pass, then a main pass, over its rows; lanes sit side by side
// along N, so every row access is coalesced. One thread per column and group is only N G / 64 waves (two per SIMD for a
// 4096 x 4096 linear at group 128, each with 128 serially issued rows), so groups of 64 rows or more are split over 4
// threads of a workgroup (64 columns x 4 slices) and groups longer than 256 rows (group -1 on a wide layer) over 16
// (1024 threads); a slice (threadIdx.y) is contiguous rows. Against the one-slice form: 1.3 - 2.5 x at group 128
// (profiles/r17_autoround.txt).
//
// What the slices of a column find meets in LDS and is combined in slice order, which is row order: the ranges in the
// kernels' own files (they differ on purpose), the two partial sums of the main pass here. No floating-point atomics;
// a slice adds its rows in row order in registers, slice 0 adds the slices in slice order: (K, N, group) alone fix the
// order of every sum, and two runs give the same bytes.
#pragma once
#include <type_traits>

#include "woq_launch.h"
#include "woq_rtn.h"

namespace woq {

constexpr int GC_THREADS = 256;     // one slice: 256 columns of one group per workgroup
constexpr int GC_SPLIT_COLS = 64;   // a split group: 64 columns (one wave) per workgroup, times the slices
constexpr int GC_MID_ROWS = 64;     // groups of at least this many rows: GC_MID_SLICES threads per column,
constexpr int GC_MID_SLICES = 4;
constexpr int GC_SPLIT_ROWS = 256;  // groups longer than this: GC_SLICES (1024 threads)
constexpr int GC_SLICES = 16;

// ---- device: where a thread stands, SLICES in {1, GC_MID_SLICES, GC_SLICES} ----------------------------------------
template <int SLICES>
struct GroupCols {
  static constexpr int COLS = SLICES == 1 ? GC_THREADS : GC_SPLIT_COLS;
  static constexpr int THREADS = SLICES * COLS;  // the launch bound: 256, 256 or 1024
  int k0, k1;  // the group's rows
  int r0, r1;  // this slice's rows, empty where the group is shorter than the slices before it

  // the thread's column (valid where < N: the last column block may be ragged; threadIdx.x is its place in a row of
  // red[]) and slice. The one-slice form may leave on an invalid column at once; the others meet at barriers.
  static __device__ __forceinline__ int column() { return blockIdx.x * COLS + threadIdx.x; }
  static __device__ __forceinline__ int slice() { return SLICES == 1 ? 0 : (int)threadIdx.y; }
  __device__ __forceinline__ GroupCols(int K, int group, int slice) {
    k0 = blockIdx.y * group, k1 = min(K, k0 + group);
    const int per = (k1 - k0 + SLICES - 1) / SLICES;
    r0 = min(k1, k0 + slice * per), r1 = min(k1, r0 + per);
  }

  // The slices' partial sums (x, y) of the main pass, through red[2 * SLICES * COLS] (behind a barrier since its last
  // reader): every thread leaves its own and meets the barrier; slice 0 then takes the column's, added in slice order.
  // By value, as the column stands apart from the rows: sums by reference or one object for both changed the kernels'
  // register allocation and load order (profiles/r20_calibration_layout.txt).
  static __device__ __forceinline__ void leave_sums(float* red, int slice, float x, float y) {
    if constexpr (SLICES > 1) {
      red[slice * COLS + threadIdx.x] = x;
      red[(SLICES + slice) * COLS + threadIdx.x] = y;
      __syncthreads();
    }
  }
  static __device__ __forceinline__ float2 take_sums(const float* red, float x, float y) {
#pragma clang fp contract(off)
    if constexpr (SLICES > 1) {
      x = 0.f, y = 0.f;
      for (int i = 0; i < SLICES; ++i) {
        x = x + red[i * COLS + threadIdx.x];
        y = y + red[(SLICES + i) * COLS + threadIdx.x];
      }
    }
    return make_float2(x, y);  // the one-slice form: the thread's own
  }
};

// ---- host: the launch of (K, N, group, bits) -----------------------------------------------------------------------
struct GroupColsPlan {
  int group;   // as the kernels take it
  int slices;  // 1, GC_MID_SLICES or GC_SLICES
  dim3 grid, block;
};

// fills `p`, or says why not. split = false: the one-slice form whatever the group.
inline const char* group_cols_plan(int K, int N, int group, int bits, GroupColsPlan& p, bool split = true) {
  if (K < 1 || N < 1) return "bad shape";
  if (!rtn_bits_ok(bits)) return "bits must be 2, 3, 4 or 8";
  p.group = rtn_group(K, group);
  const int n_groups = rtn_group_count(K, p.group);
  if (!n_groups) return "more than 65535 groups";
  p.slices = !split ? 1 : (p.group > GC_SPLIT_ROWS ? GC_SLICES : (p.group >= GC_MID_ROWS ? GC_MID_SLICES : 1));
  const int cols = p.slices > 1 ? GC_SPLIT_COLS : GC_THREADS;
  p.grid = dim3((unsigned)((N + cols - 1) / cols), (unsigned)n_groups);
  p.block = p.slices > 1 ? dim3(GC_SPLIT_COLS, p.slices) : dim3(GC_THREADS);
  return nullptr;
}

// launch(std::integral_constant<int, SLICES>) for the plan's slice count: the three instantiations of a kernel
template <class Launch>
void group_cols_dispatch(int slices, Launch&& launch) {
  if (slices == GC_SLICES)
    launch(std::integral_constant<int, GC_SLICES>());
  else if (slices == GC_MID_SLICES)
    launch(std::integral_constant<int, GC_MID_SLICES>());
  else
    launch(std::integral_constant<int, 1>());
}

// a W~ and its gradient: fp32, fp16 or bf16
inline bool fake_quant_dtype_ok(int dt) { return dt == WOQ_F32 || dt == WOQ_BF16 || dt == WOQ_F16; }

}  // namespace woq
