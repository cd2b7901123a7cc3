// The fixed-order slab reduces of the Gaussian-binned-sum ops (declared in binned_host.h): every
// op that runs more than one workgroup leaves one slab row per workgroup, and one of these two
// one-workgroup kernels sums the rows with slab_column_sum (binned_common.h), whose order
// depends only on the row count and the column count of the call.
#include <torch/extension.h>

#include "binned_host.h"

namespace mg {

namespace {

// Forward slabs (binned.hip, binned_jvp.hip, binned_hvp.hip: one group of NB columns;
// binned_multi.hip: one group per channel; binned2d.hip: groups of up to 32 cells).
__global__ __launch_bounds__(kRedThreads) void binned_reduce_fwd_kernel(const float* slab,
                                                                        int64_t rows, ReduceFwd s,
                                                                        float* out) {
  __shared__ float part[kRedThreads];
  float t;
  const int col0 = blockIdx.x * s.gcols;
  if (slab_column_sum(slab, rows, s.ld, col0, s.gcols, part, t)) {
    const int c = col0 + threadIdx.x;
    const int j = c / s.nbp, k = c % s.nbp;
    if (j < s.nrows_out && k < s.nb) out[j * s.nb + k] = t;
  }
}

// Backward slabs of broadcast gradients: [blocks, 2] (sigma, w), [blocks, 4] (binned2d.hip) and
// [blocks, 8] (binned_multi.hip, whose later channel passes add to sigma's gradient).
__global__ __launch_bounds__(kRedThreads) void binned_reduce_bwd_kernel(const float* slab,
                                                                        int64_t rows, int ncols,
                                                                        ReduceBwd r) {
  __shared__ float part[kRedThreads];
  float t;
  if (slab_column_sum(slab, rows, ncols, 0, ncols, part, t)) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if ((int)threadIdx.x == k && r.out[k] != nullptr)
        r.out[k][0] = k == 0 && r.add0 ? r.out[k][0] + t : t;
    }
  }
}

}  // namespace

void launch_reduce_fwd(const float* slab, int64_t rows, const ReduceFwd& s, float* out,
                       hipStream_t stream) {
  hipLaunchKernelGGL(binned_reduce_fwd_kernel, dim3(s.ngroups), dim3(kRedThreads), 0, stream, slab,
                     rows, s, out);
}

void launch_reduce_bwd(const float* slab, int64_t rows, int ncols, const ReduceBwd& r,
                       hipStream_t stream) {
  TORCH_CHECK(ncols == 2 || ncols == 4 || ncols == 8, "launch_reduce_bwd: 2, 4 or 8 columns");
  hipLaunchKernelGGL(binned_reduce_bwd_kernel, dim3(1), dim3(kRedThreads), 0, stream, slab, rows,
                     ncols, r);
}

}  // namespace mg
