// The chunk walk the sampler's vector kernels share (hmc.hip, prior.hip): a vector is walked
// in chunks of 4 elements, chunk j by the same thread of the same grid whether the chunk is
// read as one float4 (all pointers 16-byte aligned) or as guarded scalars (any other view, and
// the last partial chunk), so an energy summed along the walk has the same bits on both load
// paths.  Here: the chunk load and store, the workgroup's slab row, the grid of a pass and
// the argument checks of the host entry points.  Everything is force-inlined or static, so a
// kernel compiles to what it did with the code written out in its own file.
#pragma once
#include "sweep_device.h"
#include "sweep_host.h"

#include <torch/extension.h>

namespace mg {

constexpr int kHmcThreads = 256;
constexpr int kHmcMaxBlocks = 2048;  // slab rows of the workspace (per energy)

// the cnt <= 4 elements of the chunk at off: one float4 when VEC and the chunk is whole
template <bool VEC>
__device__ __forceinline__ void load_chunk(const float* __restrict__ x, int64_t off, int cnt,
                                           float (&v)[4]) {
  if (VEC && cnt == 4) {
    const float4 t = *reinterpret_cast<const float4*>(x + off);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < cnt ? x[off + e] : 0.0f;
  }
}

template <bool VEC>
__device__ __forceinline__ void store_chunk(float* __restrict__ x, int64_t off, int cnt,
                                            const float (&v)[4]) {
  if (VEC && cnt == 4) {
    *reinterpret_cast<float4*>(x + off) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) x[off + e] = v[e];
  }
}

// the workgroup's sum into its slab row (every thread of the workgroup calls it)
__device__ __forceinline__ void slab_row(double acc, double* __restrict__ partial) {
  __shared__ double scratch[kHmcThreads / kWave];
  double s[1] = {acc};
  block_sum_n<1>(s, scratch);
  if (threadIdx.x == 0) partial[blockIdx.x] = s[0];
}

// Grid of a pass: the chunk count capped at what the GPU holds resident at once (as
// launch_dot / the streaming passes of lbfgs.hip).  One cap per kernel family -- the least
// of its instantiations -- so the float4 and the scalar path launch the same grid and sum
// their energies in the same order.
template <typename... K>
static int hmc_grid(int64_t n, GridCap& cap, K... kernels) {
  return chunk_grid((n + 3) >> 2, kHmcThreads,
                    resident_cap(cap, kHmcMaxBlocks, kHmcThreads, kernels...));
}

static inline void check_vec(const torch::Tensor& t, int64_t n, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == n,
              what, ": contiguous fp32 device vector of n elements");
}

static inline bool has(const c10::optional<torch::Tensor>& t) {
  return t.has_value() && t->defined();
}

}  // namespace mg
