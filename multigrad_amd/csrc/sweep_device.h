// Device scaffolding of the optimizer vector kernels (gram.hip, box_dual.hip, lbfgs.hip,
// hmc.hip): the group loads of a column sweep over a short, wide matrix (box_dual.hip), the
// fixed-order slab-row store (box_dual.hip, lbfgs.hip) and slab entry sum (all four) that make
// their reductions bitwise reproducible, and the index of an upper-triangle entry.  The
// two sweep loops themselves stay in the kernels.  Everything takes register arrays by
// reference, carries no __restrict__ and is force-inlined, so a kernel compiles to what it
// did with the code written out.
#pragma once
#include <type_traits>

#include "common.h"

namespace mg {

// Group j of G columns of one vector: one 16-byte load (G = 4) or one element (G = 1).
template <int G>
__device__ __forceinline__ void load_group(const float* p, int64_t j, float (&v)[G]) {
  static_assert(G == 1 || G == 4, "load_group: one element or one float4");
  if constexpr (G == 4) {
    const float4 t = reinterpret_cast<const float4*>(p)[j];
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[j];
  }
}

// The same group of each of T rows.
template <int T, int G>
__device__ __forceinline__ void load_group_rows(const float* (&rows)[T], int64_t j,
                                                float (&x)[T][G]) {
#pragma unroll
  for (int a = 0; a < T; ++a) load_group<G>(rows[a], j, x[a]);
}

// Entry e of a thread's accumulators, a register array [NE] or [R][C] (row by row).
template <int NE, typename A>
__device__ __forceinline__ double slab_value(const A (&acc)[NE], int e) {
  return (double)acc[e];
}
template <int R, int C, typename A>
__device__ __forceinline__ double slab_value(const A (&acc)[R][C], int e) {
  return (double)acc[e / C][e % C];
}

// Fixed-order block sums of a thread's NE accumulators, 8 at a time, into out[0 .. NE): this
// workgroup's slab row.  Every thread of the workgroup calls it.
template <int THREADS, typename Acc>
__device__ __forceinline__ void slab_row_store(double* out, const Acc& acc) {
  constexpr int NE = sizeof(Acc) / sizeof(std::remove_all_extents_t<Acc>);
  __shared__ double scratch[8 * (THREADS / kWave)];
#pragma unroll
  for (int e0 = 0; e0 < NE; e0 += 8) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = e0 + q < NE ? slab_value(acc, e0 + q) : 0.0;
    block_sum_n<8>(v, scratch);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (e0 + q < NE) out[e0 + q] = v[q];
    }
    __syncthreads();
  }
}

// The workgroup's fixed-order sum of at(r), r < rows: each thread a fixed strided subset, then
// the shuffle/LDS tree.  The result is valid in thread 0.
template <int THREADS, typename At>
__device__ __forceinline__ double slab_entry_sum(int rows, At&& at) {
  double s[1] = {0.0};
  for (int r = threadIdx.x; r < rows; r += THREADS) s[0] += at(r);
  __shared__ double scratch[THREADS / kWave];
  block_sum_n<1>(s, scratch);
  return s[0];
}

// Entry e of the upper triangle of a T x T matrix stored row by row: (a, b), a <= b.
__device__ __forceinline__ void triangle_index(int e, int T, int& a, int& b) {
  a = 0;
  while (e >= T - a) {
    e -= T - a;
    ++a;
  }
  b = a + e;
}

}  // namespace mg
