// Host-side helpers shared by the SMF kernel families (smf_tiles.hip, smf_lanes.hip,
// smf2.hip), and the launchers of the kernels that another family's host code needs: every
// kernel is instantiated in ONE translation unit, next to its launcher.
#pragma once
#include "smf_device.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cmath>
#include <vector>

namespace mg {

inline int padded_bins(int nb) {
  const int sizes[] = {1, 2, 4, 8, 10, 16, 32};
  for (int s : sizes)
    if (nb <= s) return s;
  TORCH_CHECK(false, "at most ", kMaxBins, " bins supported, got ", nb);
  return 0;
}

inline SmfBins make_bins(const std::vector<double>& edges, const std::vector<double>& scale, int nbp) {
  const int nb = (int)scale.size();
  TORCH_CHECK((int)edges.size() == nb + 1, "need nb+1 edges");
  SmfBins b;
  for (int e = 0; e <= kMaxBins; ++e) b.edge[e] = (float)edges[std::min(e, nb)];
  for (int k = 0; k < kMaxBins; ++k) b.scale[k] = k < nb ? (float)scale[k] : 0.0f;
  // uniform spacing (the recurrence path also requires no zero-width padded bins)
  const double d = (edges[nb] - edges[0]) / nb;
  bool uni = nb == nbp && d > 0;
  for (int e = 0; e <= nb && uni; ++e)
    uni = std::fabs(edges[e] - (edges[0] + e * d)) <= 1e-6 * std::max(1.0, std::fabs(edges[e]));
  b.delta = uni ? (float)d : 0.0f;
  return b;
}

#define MG_DISPATCH_NB(NBP, ...)                             \
  switch (NBP) {                                             \
    case 1: { constexpr int NB = 1; __VA_ARGS__; break; }    \
    case 2: { constexpr int NB = 2; __VA_ARGS__; break; }    \
    case 4: { constexpr int NB = 4; __VA_ARGS__; break; }    \
    case 8: { constexpr int NB = 8; __VA_ARGS__; break; }    \
    case 10: { constexpr int NB = 10; __VA_ARGS__; break; }  \
    case 16: { constexpr int NB = 16; __VA_ARGS__; break; }  \
    default: { constexpr int NB = 32; __VA_ARGS__; break; }  \
  }

inline void check_dev(const torch::Tensor& t, const char* name, at::ScalarType st) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == st, name, " has wrong dtype");
}

// Runtime flags -> template arguments.
template <typename F>
inline void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

// Resident workgroups of `kernel` on the whole chip (occupancy x CUs): a grid that fills the
// chip in a single round of workgroups.  The device-property and occupancy queries cost
// ~20 us of host time, so call sites on a step's critical path cache the result.
inline int64_t resident_blocks(const void* kernel, int threads) {
  int dev = 0, occ = 0;
  (void)hipGetDevice(&dev);
  hipDeviceProp_t prop;
  (void)hipGetDeviceProperties(&prop, dev);
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, 0);
  return (int64_t)std::max(1, occ) * prop.multiProcessorCount;
}

// smf_tiles.hip: the fused sumstat epilogue (smf_epilogue_kernel) -- checked arguments (peers
// empty = single rank) and the one-workgroup launch -- and the fixed-order finalize of split
// populations (smf_vjp_finalize_kernel; giant [G, 3] = {pop, part_begin, part_end}).
EpiArgs make_epi(torch::Tensor slab, int64_t nrows, int nb, int nbp, torch::Tensor target,
                 double eps, torch::Tensor S, torch::Tensor loss, torch::Tensor h,
                 const std::vector<int64_t>& peers, int64_t rank, int* seq, int* err,
                 double timeout_s, int* adv);
void launch_epilogue(int nbp, const EpiArgs& E, const SmfBins& b, hipStream_t stream);
void launch_vjp_finalize(const torch::Tensor& giant, const float2* partials, const float2* theta,
                         float2* grad, bool log_sigma, hipStream_t stream);

}  // namespace mg
