// Host-side helpers shared by the one-axis Gaussian-binned-sum translation units (binned.hip:
// forward and first backward; binned_hvp.hip: second backward; binned_jvp.hip: tangent): checked arguments, the padded
// dispatch and the launcher of the slab reduce, which is instantiated in binned.hip.
#pragma once
#include "binned_common.h"
#include "smf_host.h"

namespace mg {

inline int binned_padded(int nb) {
  TORCH_CHECK(nb >= 1 && nb <= kMaxBins, "gaussian_binned_sum: 1 <= nb <= ", kMaxBins, ", got ", nb);
  return nb <= 4 ? 4 : nb <= 8 ? 8 : nb <= 16 ? 16 : 32;
}

#define MG_DISPATCH_BINNED(NBP, ...)                        \
  switch (NBP) {                                            \
    case 4: { constexpr int NB = 4; __VA_ARGS__; break; }   \
    case 8: { constexpr int NB = 8; __VA_ARGS__; break; }   \
    case 16: { constexpr int NB = 16; __VA_ARGS__; break; } \
    default: { constexpr int NB = 32; __VA_ARGS__; break; } \
  }

inline bool aligned16(const void* p) { return aligned_to(p, 16); }

// Workgroups that fill the chip once (occupancy x CU count of the device), per kernel.
template <auto Kernel>
int64_t chip_blocks() {
  static int64_t cap = resident_blocks(reinterpret_cast<const void*>(Kernel), kBinThreads);
  return cap;
}

inline BinnedArgs make_args(const torch::Tensor& mu, const torch::Tensor& sigma,
                            const c10::optional<torch::Tensor>& w, const std::vector<double>& edges) {
  check_dev(mu, "mu", at::kFloat);
  check_dev(sigma, "sigma", at::kFloat);
  BinnedArgs a;
  a.n = mu.numel();
  a.nb = (int)edges.size() - 1;
  binned_padded(a.nb);
  for (int e = 1; e <= a.nb; ++e)
    TORCH_CHECK(edges[e] > edges[e - 1], "gaussian_binned_sum: edges must be strictly increasing");
  for (int e = 0; e <= kMaxBins; ++e) a.edge[e] = (float)edges[std::min(e, a.nb)];
  TORCH_CHECK(sigma.numel() == a.n || sigma.numel() == 1, "sigma must have N elements or one");
  a.mu = mu.data_ptr<float>();
  a.sigma = sigma.data_ptr<float>();
  a.sig_b = sigma.numel() == 1 && a.n != 1;
  a.w = nullptr;
  a.w_b = 0;
  if (w.has_value() && w->defined()) {
    check_dev(*w, "weights", at::kFloat);
    TORCH_CHECK(w->numel() == a.n || w->numel() == 1, "weights must have N elements or one");
    a.w = w->data_ptr<float>();
    a.w_b = w->numel() == 1 && a.n != 1;
  }
  a.vec = aligned16(a.mu) && (a.sig_b || aligned16(a.sigma)) &&
          (a.w == nullptr || a.w_b || aligned16(a.w));
  return a;
}

// binned.hip: fixed-order sum of slab rows [rows, ncols] (ncols a power of two <= 32) by one
// workgroup.  Columns [0, na) go to out_a, column na to out_b (either may be null: dropped).
void launch_binned_reduce(const float* slab, int64_t rows, int ncols, float* out_a, int na,
                          float* out_b, hipStream_t stream);

// binned.hip: the forward, which binned_jvp.hip calls for a tangent of the weights alone.
torch::Tensor binned_forward(torch::Tensor mu, torch::Tensor sigma, c10::optional<torch::Tensor> w,
                             std::vector<double> edges);

}  // namespace mg
