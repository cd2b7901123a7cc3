// Gaussian-binned sum over many fine bins, 33 <= nb <= 4096 (ops/binned_fine.py):
//   out[k] = sum_i w_i * (Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i))
// The one-axis op (binned.hip) keeps an accumulator per bin in registers and evaluates every
// edge for every object; here an object visits only its window, the bins that overlap
// (mu - T sigma, mu + T sigma) with T = 5.5, found by two binary searches over the edges in LDS.
// The first and last bin of a window are evaluated at their true edges; per object and side the
// bins beyond the window lose at most Phi(-5.5) = 1.9e-8 of the weight.
//
// Forward : a scatter to data-dependent bins has no fixed float summation order, so every term
//           t = w_i * dPhi_ik is rounded once to float32 and accumulated as a 64-bit fixed-point
//           integer, q = rint(t * 2^s) with s = 30 - e and max_i |w_i| = m * 2^e, m in [0.5, 1):
//           |q| <= 2^30 (1 + 1e-6), so N < 2^31 terms stay below 2^62.  Integer addition is
//           associative: the sums do not depend on arrival order, on the grid or on the order of
//           the objects.  A workgroup keeps an nb-entry int64 histogram in LDS (ds_add_u64),
//           adds its non-zero bins to a zero-filled int64 [nb] buffer (global_atomic_add_x2),
//           and a last kernel writes out[k] = float(double(acc[k]) * 2^-s).  max |w| comes from
//           a max-reduction kernel (integer atomicMax on the bits of |w|: exact, any order) and
//           never leaves the device.  No weights or a one-element weight skip that pass: dPhi
//           is accumulated at s = 30 and the last kernel multiplies by w.  A non-finite weight
//           or term, or a window that is not an interval (NaN mu or sigma), sets a flag, and the
//           last kernel then writes NaN to every bin.
// Backward: per object in the original order, recomputing from mu / sigma / w (no residuals),
//           with the cotangent and the edges in LDS; the walk covers the edges of the window.
//           Per-object gradients are stored 16 bytes at a time; gradients of broadcast operands
//           go block sum -> slab -> fixed-order reduce, as in binned_group.hip.
// No float atomics, no host synchronisation; launches on the current stream.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>
#include <tuple>
#include <utility>

#include "binned_host.h"

namespace mg {

namespace {

constexpr int kFineMaxBins = 4096;
constexpr float kFineT = 5.5f;  // half width of a window in sigmas
constexpr int kFineShift = 30;  // s when the terms are dPhi alone

struct FineArgs {
  const float* mu;
  const float* sigma;
  const float* w;     // nullptr: every weight is 1
  const float* edge;  // [nb + 1] on the device
  int64_t n;
  int nb;
  int sig_b;  // sigma has one element
  int w_b;    // w has one element
  int vec;    // every per-object operand is 16-byte aligned
};

// The work buffer of the forward: nb int64 sums, then one int64 whose low half holds the bits of
// max |w| and whose high half is the non-finite flag.
__device__ __forceinline__ unsigned* fine_meta(unsigned long long* acc, int nb) {
  return reinterpret_cast<unsigned*>(acc + nb);
}

// s = 30 - e with max |w| = m * 2^e, m in [0.5, 1); max |w| = 0 gives s = 30 (every term is 0).
__device__ __forceinline__ int fine_shift(unsigned maxbits) {
  int e = 0;
  (void)frexpf(__uint_as_float(maxbits), &e);
  return kFineShift - e;
}

// The window of an object: bins [k0, k1] overlap (lo, hi); empty when k0 > k1.  e holds nb + 1
// increasing edges; every index read lies in [0, nb] whatever lo and hi are.
__device__ __forceinline__ void fine_window(const float* e, int nb, float lo, float hi, int& k0,
                                            int& k1) {
  int a = 1, b = nb + 1;  // first j in [1, nb + 1) with e[j] > lo
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (e[mid] <= lo) a = mid + 1;
    else b = mid;
  }
  k0 = a - 1;
  a = min(k0, nb - 1);  // e[j] < hi for every j <= k0 < nb (e[k0] <= lo < hi, or k0 = 0)
  b = nb;               // first j in [a, nb) with e[j] >= hi
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (e[mid] < hi) a = mid + 1;
    else b = mid;
  }
  k1 = a - 1;
}

__global__ __launch_bounds__(kBinThreads) void fine_maxabs_kernel(const float* w, int64_t n,
                                                                  int vec, unsigned long long* acc,
                                                                  int nb) {
  __shared__ unsigned part[kBinThreads / kWave];
  unsigned m = 0;  // the bits of a non-negative float order as unsigned integers
  bool bad = false;
  const int64_t nq = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < nq; q += stride) {
    float w4[4];
    load_group<4>(w, q * 4, n, vec && q * 4 + 4 <= n, false, 0.0f, 0.0f, w4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = fabsf(w4[j]);
      if (v <= 3.4028234664e38f) m = max(m, __float_as_uint(v));
      else bad = true;  // infinite or NaN
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x >> 6] = m;
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) {
    for (int k = 1; k < kBinThreads / kWave; ++k) m = max(m, part[k]);
    unsigned* meta = fine_meta(acc, nb);
    if (m != 0) atomicMax(meta, m);
    if (any_bad) atomicOr(meta + 1, 1u);
  }
}

// PERW: per-object weights, scaled by the exponent of max |w|; else the terms are dPhi at s = 30.
template <bool PERW>
__global__ __launch_bounds__(kBinThreads) void fine_fwd_kernel(FineArgs a,
                                                               unsigned long long* acc) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fine_lds[];
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(fine_lds);
  float* edge = reinterpret_cast<float*>(hist + a.nb);
  const int nb = a.nb;
  for (int k = threadIdx.x; k < nb; k += kBinThreads) hist[k] = 0ull;
  for (int k = threadIdx.x; k <= nb; k += kBinThreads) edge[k] = a.edge[k];
  unsigned* meta = fine_meta(acc, nb);
  const int s = PERW ? fine_shift(meta[0]) : kFineShift;
  const int lane = threadIdx.x & (kWave - 1);
  __syncthreads();
  bool bad = false;
  const int64_t nq = (a.n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < nq; q += stride) {
    const int64_t i0 = q * 4;
    const bool full = a.vec && i0 + 4 <= a.n;
    float m4[4], s4[4], w4[4];
    load_group<4>(a.mu, i0, a.n, full, false, 0.0f, 0.0f, m4);
    load_group<4>(a.sigma, i0, a.n, full, a.sig_b != 0, 1.0f, 1.0f, s4);
    if constexpr (PERW) load_group<4>(a.w, i0, a.n, full, false, 1.0f, 0.0f, w4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j >= a.n) continue;
      const float m = m4[j], sg = s4[j];
      const float lo = m - kFineT * sg, hi = m + kFineT * sg;
      if (!(hi >= lo)) {  // NaN mu or sigma, or a negative width
        bad = true;
        continue;
      }
      int k0, k1;
      fine_window(edge, nb, lo, hi, k0, k1);
      if (k0 > k1) continue;
      const float inv = 1.0f / sg;
      // With wide objects the lanes of a wave walk the same window in step, and 64 adds to one
      // LDS address serialise.  When a quarter of the wave starts at the same bin, windows
      // of 8 bins or more are therefore walked cyclically from a start that is spread over the
      // window by lane (wave-uniform choice; the cyclic walk costs one more edge CDF).  The
      // terms and their integer sum are the same in any order.
      const int len = k1 - k0 + 1;
      const bool same = k0 == __builtin_amdgcn_readfirstlane(k0);
      const bool spread = __popcll(__ballot(same)) >= kWave / 4;
      int k = k0 + (spread && len >= 8 ? (lane * len) >> 6 : 0);
      float b0, f0, gs;
      edge_cdf((edge[k] - m) * inv, b0, f0, gs);
      for (int it = 0; it < len; ++it) {
        float b1, f1;
        edge_cdf((edge[k + 1] - m) * inv, b1, f1, gs);
        float t = (b1 - b0) + (f1 - f0);
        if constexpr (PERW) t *= w4[j];
        b0 = b1;
        f0 = f1;
        const float x = ldexpf(t, s);  // |x| <= 2^30 (1 + 1e-6)
        if (!(fabsf(x) <= 0x1p+31f)) {
          bad = true;
        } else {
          const long long v = __float2ll_rn(x);
          if (v != 0) atomicAdd(&hist[k], (unsigned long long)v);
        }
        if (++k > k1 && it + 1 < len) {  // wrap to the first bin of the window
          k = k0;
          edge_cdf((edge[k0] - m) * inv, b0, f0, gs);
        }
      }
    }
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  for (int k = threadIdx.x; k < nb; k += kBinThreads) {
    const unsigned long long v = hist[k];
    if (v != 0ull) atomicAdd(&acc[k], v);
  }
  if (threadIdx.x == 0 && any_bad) atomicOr(meta + 1, 1u);
}

// out[k] = float(double(acc[k]) * 2^-s * wscale), or NaN everywhere when the flag is set.
__global__ __launch_bounds__(kBinThreads) void fine_final_kernel(const unsigned long long* acc,
                                                                 int nb, int perw,
                                                                 const float* wscale, float* out) {
  const int k = blockIdx.x * kBinThreads + threadIdx.x;
  if (k >= nb) return;
  const unsigned* meta = reinterpret_cast<const unsigned*>(acc + nb);
  const int s = perw ? fine_shift(meta[0]) : kFineShift;
  double v = ldexp((double)(long long)acc[k], -s);
  if (wscale != nullptr) v *= (double)wscale[0];
  out[k] = meta[1] != 0u ? __uint_as_float(0x7fc00000u) : (float)v;
}

template <bool GMU, bool GSIG, bool GW>
__global__ __launch_bounds__(kBinThreads) void fine_bwd_kernel(FineArgs a, BinnedGrad o,
                                                               int direct) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fine_lds[];
  __shared__ float red[2 * (kBinThreads / kWave)];
  float* gl = reinterpret_cast<float*>(fine_lds);
  float* edge = gl + a.nb;
  const int nb = a.nb;
  for (int k = threadIdx.x; k < nb; k += kBinThreads) gl[k] = o.g[k];
  for (int k = threadIdx.x; k <= nb; k += kBinThreads) edge[k] = a.edge[k];
  __syncthreads();
  const bool red_sig = GSIG && a.sig_b, red_w = GW && a.w_b;
  float rs[2] = {0.0f, 0.0f};  // this thread's share of the broadcast gradients
  const int64_t nq = (a.n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < nq; q += stride) {
    const int64_t i0 = q * 4;
    const bool full = a.vec && i0 + 4 <= a.n;
    float m4[4], s4[4], w4[4], dm[4], ds[4], dc[4];
    load_group<4>(a.mu, i0, a.n, full, false, 0.0f, 0.0f, m4);
    load_group<4>(a.sigma, i0, a.n, full, a.sig_b != 0, 1.0f, 1.0f, s4);
    load_group<4>(a.w, i0, a.n, full, a.w_b != 0, 1.0f, 0.0f, w4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float m = m4[j], sg = s4[j];
      const float lo = m - kFineT * sg, hi = m + kFineT * sg;
      float A = 0.0f;  // sum_e h_e exp(-z_e^2/2)
      float B = 0.0f;  // sum_e h_e z_e exp(-z_e^2/2)
      float C = 0.0f;  // sum_k g_k dPhi_k
      const float inv = 1.0f / sg;
      if (i0 + j >= a.n) {
        // beyond N: weight 0, nothing stored
      } else if (!(hi >= lo)) {
        A = B = C = __uint_as_float(0x7fc00000u);
      } else {
        int k0, k1;
        fine_window(edge, nb, lo, hi, k0, k1);
        if (k0 <= k1) {
          float gp = k0 > 0 ? gl[k0 - 1] : 0.0f;  // g[e - 1]
          float b0 = 0.0f, f0 = 0.0f;
          for (int e = k0; e <= k1 + 1; ++e) {
            const float gc = e < nb ? gl[e] : 0.0f;
            const float z = (edge[e] - m) * inv;
            float gs;
            if constexpr (GW) {
              float b1, f1;
              edge_cdf(z, b1, f1, gs);
              if (e > k0) C = fmaf(gp, (b1 - b0) + (f1 - f0), C);
              b0 = b1;
              f0 = f1;
            } else {
              const float ws = z * kWScale;
              gs = fast_exp2(-ws * ws);
            }
            const float hg = (gp - gc) * gs;  // h_e = g_{e-1} - g_e (g_{-1} = g_{nb} = 0)
            if constexpr (GMU) A += hg;
            if constexpr (GSIG) B = fmaf(hg, z, B);
            gp = gc;
          }
        }
      }
      const float c = -kInvSqrt2PiB * w4[j] * inv;  // 0 beyond N (weight 0)
      dm[j] = c * A;
      ds[j] = c * B;
      dc[j] = C;
    }
    if constexpr (GMU) store_group<4>(o.dmu, i0, a.n, dm);
    if constexpr (GSIG) put_quad(red_sig, rs[0], o.dsigma, i0, a.n, ds);
    if constexpr (GW) put_quad(red_w, rs[1], o.dw, i0, a.n, dc);
  }
  finish_broadcast(rs, red, red_sig, red_w, o.dsigma, o.dw, o.slab, direct);
}

FineArgs make_fine_args(const torch::Tensor& mu, const torch::Tensor& sigma,
                        const c10::optional<torch::Tensor>& w, const torch::Tensor& edges) {
  FineArgs a;
  a.n = mu.numel();
  bool wide = true;
  int none = 0;
  a.mu = operand(mu, "mu", a.n, none, wide);
  a.sigma = operand(sigma, "sigma", a.n, a.sig_b, wide);
  check_dev(edges, "edges", at::kFloat);
  a.nb = (int)edges.numel() - 1;
  TORCH_CHECK(edges.numel() >= 2 && a.nb <= kFineMaxBins, "gaussian_binned_sum_fine: 1 <= nb <= ",
              kFineMaxBins, ", got ", edges.numel() - 1);
  TORCH_CHECK(a.n > 0 && a.n < (int64_t(1) << 31), "gaussian_binned_sum_fine: 0 < N < 2^31 required");
  a.edge = edges.data_ptr<float>();
  a.w = nullptr;
  a.w_b = 0;
  if (w.has_value() && w->defined()) a.w = operand(*w, "weights", a.n, a.w_b, wide);
  a.vec = wide;
  return a;
}

}  // namespace

// edges: the plan's float32 [nb + 1] device copy.  Returns the [nb] bin sums.
torch::Tensor binned_fine_forward(torch::Tensor mu, torch::Tensor sigma,
                                  c10::optional<torch::Tensor> w, torch::Tensor edges) {
  FineArgs a = make_fine_args(mu, sigma, w, edges);
  const bool perw = a.w != nullptr && !a.w_b;  // N == 1: the one weight is the object's own
  const float* wscale = a.w != nullptr && !perw ? a.w : nullptr;
  auto stream = at::hip::getCurrentHIPStream();
  auto acc = torch::zeros({(int64_t)a.nb + 1}, mu.options().dtype(at::kLong));
  auto out = torch::empty({(int64_t)a.nb}, mu.options());
  auto* accp = reinterpret_cast<unsigned long long*>(acc.data_ptr<int64_t>());
  const size_t lds = (size_t)a.nb * 8 + (size_t)(a.nb + 1) * sizeof(float);
  const int64_t need = blocks_for(a.n);
  if (perw) {
    const int64_t mblocks = std::min(need, chip_blocks<fine_maxabs_kernel>());
    hipLaunchKernelGGL(fine_maxabs_kernel, dim3(mblocks), dim3(kBinThreads), 0, stream, a.w, a.n,
                       aligned16(a.w) ? 1 : 0, accp, a.nb);
    const int64_t blocks =
        std::min(need, chip_blocks(reinterpret_cast<const void*>(fine_fwd_kernel<true>), lds));
    hipLaunchKernelGGL(fine_fwd_kernel<true>, dim3(blocks), dim3(kBinThreads), lds, stream, a, accp);
  } else {
    a.w = nullptr;
    a.w_b = 0;
    const int64_t blocks =
        std::min(need, chip_blocks(reinterpret_cast<const void*>(fine_fwd_kernel<false>), lds));
    hipLaunchKernelGGL(fine_fwd_kernel<false>, dim3(blocks), dim3(kBinThreads), lds, stream, a,
                       accp);
  }
  hipLaunchKernelGGL(fine_final_kernel, dim3((a.nb + kBinThreads - 1) / kBinThreads),
                     dim3(kBinThreads), 0, stream, accp, a.nb, perw ? 1 : 0, wscale,
                     out.data_ptr<float>());
  return out;
}

// Gradients of sum_k g[k] out[k] with respect to the requested operands; an operand that was
// not requested comes back undefined (None).  A broadcast operand gets the sum over objects.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> binned_fine_backward(
    torch::Tensor mu, torch::Tensor sigma, c10::optional<torch::Tensor> w, torch::Tensor edges,
    torch::Tensor g, bool need_mu, bool need_sigma, bool need_w) {
  FineArgs a = make_fine_args(mu, sigma, w, edges);
  check_dev(g, "grad_out", at::kFloat);
  TORCH_CHECK(g.numel() == a.nb, "grad_out must have nb elements");
  TORCH_CHECK(!need_w || a.w != nullptr, "weights gradient requested without weights");
  TORCH_CHECK(need_mu || need_sigma || need_w, "no gradient requested");
  BinnedGrad o = {};
  o.g = g.data_ptr<float>();
  auto dmu = alloc_grad(need_mu, a.n, mu, o.dmu);
  auto dsigma = alloc_grad(need_sigma, sigma.numel(), mu, o.dsigma);
  auto dw = alloc_grad(need_w, need_w ? w->numel() : 0, mu, o.dw);
  const auto r = reduce_sigma_w(a.sig_b ? o.dsigma : nullptr, a.w_b ? o.dw : nullptr);
  const size_t lds = (size_t)(2 * a.nb + 1) * sizeof(float);  // the cotangent and the edges
  auto stream = at::hip::getCurrentHIPStream();
  with_need3(need_mu, need_sigma, need_w, [&](auto M, auto S, auto W) {
    launch_slab_bwd<fine_bwd_kernel<decltype(M)::value, decltype(S)::value, decltype(W)::value>>(
        a, o, blocks_for(a.n), 2, r, mu, stream, lds);
  });
  return std::make_tuple(dmu, dsigma, dw);
}

}  // namespace mg
