// The host layer of the Gaussian-binned-sum translation units (binned.hip, binned_hvp.hip,
// binned_jvp.hip, binned2d.hip, binned_multi.hip, binned_group.hip, binned_fine.hip; the slab
// reduces live in binned_reduce.hip): bin padding and its dispatch, the resident-workgroup
// cache, checked edges and operands, gradient allocation, and the two launch shapes that the
// ops share -- a forward that writes `out` directly from one workgroup or goes through a slab
// and the fixed-order reduce, and an object-parallel backward whose broadcast gradients do.
#pragma once
#include <map>
#include <mutex>
#include <utility>

#include "binned_common.h"
#include "smf_host.h"
#include "sweep_host.h"

namespace mg {

// The template bin count (4 / 8 / 16 / 32) that covers nb real bins; `axis` names the axis of
// a two-axis op in the message.
inline int padded_bins(int nb, const char* op_name, const char* axis = "") {
  TORCH_CHECK(nb >= 1 && nb <= kMaxBins, op_name, ": 1 <= nb", axis, " <= ", kMaxBins, ", got ", nb);
  return nb <= 4 ? 4 : nb <= 8 ? 8 : nb <= 16 ? 16 : 32;
}

#define MG_DISPATCH_PAD(NBP, NAME, ...)                       \
  switch (NBP) {                                              \
    case 4: { constexpr int NAME = 4; __VA_ARGS__; break; }   \
    case 8: { constexpr int NAME = 8; __VA_ARGS__; break; }   \
    case 16: { constexpr int NAME = 16; __VA_ARGS__; break; } \
    default: { constexpr int NAME = 32; __VA_ARGS__; break; } \
  }
#define MG_DISPATCH_BINNED(NBP, ...) MG_DISPATCH_PAD(NBP, NB, __VA_ARGS__)

// Workgroups that fill the chip once (occupancy x CU count of the device), per kernel.
template <auto Kernel>
int64_t chip_blocks() {
  static int64_t cap = resident_blocks(reinterpret_cast<const void*>(Kernel), kBinThreads);
  return cap;
}

// The same with `lds` bytes of dynamic LDS per workgroup; the query costs ~20 us of host time,
// so the answer is kept per kernel and LDS size.
inline int64_t chip_blocks(const void* kernel, size_t lds) {
  static std::mutex mu;
  static std::map<std::pair<const void*, size_t>, int64_t> cache;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair(kernel, lds);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int dev = 0, occ = 0;
  (void)hipGetDevice(&dev);
  hipDeviceProp_t prop;
  (void)hipGetDeviceProperties(&prop, dev);
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, kBinThreads, lds);
  const int64_t cap = (int64_t)std::max(1, occ) * prop.multiProcessorCount;
  cache[key] = cap;
  return cap;
}

// Workgroups of kBinThreads threads that cover n objects in groups of `per`.
inline int64_t blocks_for(int64_t n, int per = 4) {
  return ((n + per - 1) / per + kBinThreads - 1) / kBinThreads;
}

// nb + 1 strictly increasing edges as floats, the last one repeated up to kMaxBins + 1.
inline void set_edges(const std::vector<double>& edges, int nb, float (&dst)[kMaxBins + 1],
                      const char* op_name) {
  for (int e = 1; e <= nb; ++e)
    TORCH_CHECK(edges[e] > edges[e - 1], op_name, ": edges must be strictly increasing");
  for (int e = 0; e <= kMaxBins; ++e) dst[e] = (float)edges[std::min(e, nb)];
}

// A float32 device operand of n elements or one: its pointer, whether it is broadcast, and
// its 16-byte alignment folded into `wide` (a broadcast operand is read as a scalar).
inline const float* operand(const torch::Tensor& t, const char* name, int64_t n, int& bcast,
                            bool& wide) {
  check_dev(t, name, at::kFloat);
  TORCH_CHECK(t.numel() == n || t.numel() == 1, name, " must have N elements or one");
  bcast = t.numel() == 1 && n != 1;
  const float* p = t.data_ptr<float>();
  wide = wide && (bcast || aligned16(p));
  return p;
}

// The pointer of an optional tangent or cotangent with `numel` elements (nullptr: absent, a
// zero).
inline const float* optional_operand(const c10::optional<torch::Tensor>& t, const char* name,
                                     int64_t numel) {
  if (!t.has_value() || !t->defined()) return nullptr;
  check_dev(*t, name, at::kFloat);
  TORCH_CHECK(t->numel() == numel, name, " has ", t->numel(), " elements, expected ", numel);
  return t->data_ptr<float>();
}

inline BinnedArgs make_args(const torch::Tensor& mu, const torch::Tensor& sigma,
                            const c10::optional<torch::Tensor>& w, const std::vector<double>& edges) {
  const char* op_name = "gaussian_binned_sum";
  BinnedArgs a;
  a.n = mu.numel();
  a.nb = (int)edges.size() - 1;
  bool wide = true;
  int none = 0;
  a.mu = operand(mu, "mu", a.n, none, wide);
  a.sigma = operand(sigma, "sigma", a.n, a.sig_b, wide);
  padded_bins(a.nb, op_name);
  set_edges(edges, a.nb, a.edge, op_name);
  a.w = nullptr;
  a.w_b = 0;
  if (w.has_value() && w->defined()) a.w = operand(*w, "weights", a.n, a.w_b, wide);
  a.vec = wide;
  return a;
}

// A gradient of `numel` floats when it is needed (undefined, ptr null, otherwise).
inline torch::Tensor alloc_grad(bool need, int64_t numel, const torch::Tensor& like, float*& ptr) {
  torch::Tensor t;
  ptr = nullptr;
  if (need) {
    t = torch::empty({numel}, like.options());
    ptr = t.data_ptr<float>();
  }
  return t;
}

// f(M, S, W) with the three gradient requests as std::bool_constants; nothing when none is set.
template <typename F>
void with_need3(bool mu, bool sigma, bool w, F&& f) {
  with_bool(mu, [&](auto M) {
    with_bool(sigma, [&](auto S) {
      with_bool(w, [&](auto W) {
        if constexpr (decltype(M)::value || decltype(S)::value || decltype(W)::value) f(M, S, W);
      });
    });
  });
}

// binned_reduce.hip: the fixed-order sums of slab rows (slab_column_sum), one workgroup each.
// Forward: workgroup b sums the columns [b * gcols, (b + 1) * gcols) of the rows [rows, ld];
// column c is cell (c / nbp, c % nbp) of a padded row-major table, and the cells inside
// [nrows_out, nb] are written to the dense row-major `out`.
struct ReduceFwd {
  int ld, gcols, ngroups, nbp, nrows_out, nb;
};
void launch_reduce_fwd(const float* slab, int64_t rows, const ReduceFwd& s, float* out,
                       hipStream_t stream);

// Backward: the ncols (2, 4 or 8) columns of the rows [rows, ncols]; column k goes to out[k][0]
// (null: dropped), and with add0 column 0 is added to what is there.
struct ReduceBwd {
  float* out[8];
  int add0;
};
void launch_reduce_bwd(const float* slab, int64_t rows, int ncols, const ReduceBwd& r,
                       hipStream_t stream);

// A forward Kernel(lead..., slab, out, direct) over min(need, one chip-filling round)
// workgroups: one workgroup writes `out` itself, several write slab rows [blocks, s.ld] that
// the fixed-order reduce sums into `out`.
template <auto Kernel, typename... Lead>
void launch_slab_fwd(int64_t need, const ReduceFwd& s, float* out, const torch::Tensor& like,
                     hipStream_t stream, const Lead&... lead) {
  const int64_t blocks = std::min(need, chip_blocks<Kernel>());
  if (blocks == 1) {
    hipLaunchKernelGGL(Kernel, dim3(1), dim3(kBinThreads), 0, stream, lead..., (float*)nullptr, out,
                       1);
  } else {
    auto slab = torch::empty({blocks, (int64_t)s.ld}, like.options());
    hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(kBinThreads), 0, stream, lead...,
                       slab.data_ptr<float>(), (float*)nullptr, 0);
    launch_reduce_fwd(slab.data_ptr<float>(), blocks, s, out, stream);
  }
}

// An object-parallel backward Kernel(a, o, direct) over min(need, one chip-filling round)
// workgroups with `lds` bytes of dynamic LDS.  Per-object gradients are stored by the kernel;
// the broadcast ones, r.out, come from one workgroup directly, from several through the slab
// [blocks, ncols] (o.slab) and the fixed-order reduce.
template <auto Kernel, typename Args, typename Grad>
void launch_slab_bwd(const Args& a, Grad& o, int64_t need, int ncols, const ReduceBwd& r,
                     const torch::Tensor& like, hipStream_t stream, size_t lds = 0) {
  const int64_t cap =
      lds == 0 ? chip_blocks<Kernel>() : chip_blocks(reinterpret_cast<const void*>(Kernel), lds);
  const int64_t blocks = std::min(need, cap);
  bool any = false;
  for (int k = 0; k < ncols; ++k) any = any || r.out[k] != nullptr;
  const bool two = any && blocks > 1;
  torch::Tensor slab;
  if (two) {
    slab = torch::empty({blocks, (int64_t)ncols}, like.options());
    o.slab = slab.data_ptr<float>();
  }
  hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(kBinThreads), lds, stream, a, o,
                     blocks == 1 ? 1 : 0);
  if (two) launch_reduce_bwd(o.slab, blocks, ncols, r, stream);
}

// The reduce of the two-column slab of BinnedGrad: sigma's and w's broadcast gradients.
inline ReduceBwd reduce_sigma_w(float* dsigma, float* dw) {
  ReduceBwd r = {};
  r.out[0] = dsigma;
  r.out[1] = dw;
  return r;
}

// binned.hip: the forward, which binned_jvp.hip calls for a tangent of the weights alone.
torch::Tensor binned_forward(torch::Tensor mu, torch::Tensor sigma, c10::optional<torch::Tensor> w,
                             std::vector<double> edges);

}  // namespace mg
