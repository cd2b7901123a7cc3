// Forward-mode tangent of the Gaussian-binned sum (ops/binned.py, _GaussianBinnedSum.jvp).
// With z_e = (e_e - mu)/sigma, phi the normal pdf and tangents (tmu, tsigma, tw) of (mu, sigma,
// w), the tangent bin mass of object i is D_i[k] = E_i[k+1] - E_i[k] with the edge term
//   E_i[e] = -(1/sigma_i) phi(z_ie) (tmu_i + z_ie tsigma_i),
// and the tangent of the output is again a binned sum:
//   tout[k] = sum_i ( w_i D_i[k] + tw_i dPhi_i[k] ).
// A missing tangent is a zero; a broadcast sigma or w has a one-element tangent that is used
// for every object.
//
// The traversal is binned_fwd_kernel's (binned.hip): a grid-stride over quads of objects,
// 16-byte loads where every pointer is aligned and guarded scalar loads otherwise, NB per-thread
// bin accumulators, block_sum_n into one slab row per workgroup, then the fixed-order reduce of
// binned.hip (a single launch when one workgroup covers the input).  Nothing of length N is
// written.  The Gaussian is evaluated as in the backward (one v_exp per edge); Phi is evaluated
// only when tw is present (TW).  The kernel exists for a mu or sigma tangent only: with tw
// alone the tangent is the forward with tw as the weights, and the host calls binned_forward.
// No float atomics: results are bitwise reproducible for a fixed N and device.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <vector>

#include "binned_host.h"

namespace mg {

namespace {

struct BinnedTangent {
  const float* tmu;     // [n]; nullptr: zero
  const float* tsigma;  // [n], or [1] when sigma is broadcast; nullptr: zero
  const float* tw;      // [n], or [1] when w is broadcast; nullptr: zero (always, unless TW)
};

// Registers at NB = 32: the 32 accumulators, and per object of the quad m, 1/sigma, the two
// edge coefficients and the running edge term (20), with TW the weight tangent and the running
// base/frac of Phi (12 more); the edges are kernel arguments and stay in scalar registers.
// The compiler's count at NB = 32 is 71 VGPRs (88 with TW), no scratch: 7 (5) waves per SIMD.
template <int NB, bool TW>
__global__ __launch_bounds__(kBinThreads) void binned_jvp_kernel(BinnedArgs a, BinnedTangent t,
                                                                 float* slab, float* out,
                                                                 int direct) {
  __shared__ float red[NB * (kBinThreads / kWave)];
  float acc[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) acc[k] = 0.0f;
  const int64_t nq = (a.n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < nq; q += stride) {
    const int64_t i0 = q * 4;
    const bool full = a.vec && i0 + 4 <= a.n;  // a.vec covers the tangents too
    float m[4], inv[4], wt[4], tm[4], ts[4], tw[4];
    load_quad(a, q, m, inv, wt);
    // objects beyond N: weight 0 and tangents 0, so every term below vanishes
    load_group<4>(t.tmu, i0, a.n, full, false, 0.0f, 0.0f, tm);
    load_group<4>(t.tsigma, i0, a.n, full, a.sig_b, 0.0f, 0.0f, ts);
    if constexpr (TW) load_group<4>(t.tw, i0, a.n, full, a.w_b, 0.0f, 0.0f, tw);
    float ua[4], ub[4], u0[4], b0[4], f0[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // w E_e = (ua + ub z_e) exp(-z_e^2/2)
      const float s = -kInvSqrt2PiB * wt[j] * inv[j];
      ua[j] = s * tm[j];
      ub[j] = s * ts[j];
    }
#pragma unroll
    for (int e = 0; e <= NB; ++e) {
      if (e <= a.nb) {  // wave-uniform: padded bins cost nothing
        float d = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float z = (a.edge[e] - m[j]) * inv[j];
          float gs, b1, f1;
          if constexpr (TW) {
            edge_cdf(z, b1, f1, gs);
          } else {
            const float ws = z * kWScale;
            gs = fast_exp2(-ws * ws);
          }
          const float u = fmaf(ub[j], z, ua[j]) * gs;
          if (e > 0) {
            float dj = u - u0[j];
            if constexpr (TW) dj = fmaf(tw[j], (b1 - b0[j]) + (f1 - f0[j]), dj);
            d += dj;
          }
          u0[j] = u;
          if constexpr (TW) {
            b0[j] = b1;
            f0[j] = f1;
          }
        }
        if (e > 0) acc[e > 0 ? e - 1 : 0] += d;  // a constant index once unrolled
      }
    }
  }
  block_sum_n<NB>(acc, red);
  if (threadIdx.x == 0) {
    if (direct) {
#pragma unroll
      for (int k = 0; k < NB; ++k)
        if (k < a.nb) out[k] = acc[k];
    } else {
#pragma unroll
      for (int k = 0; k < NB; ++k) slab[(int64_t)blockIdx.x * NB + k] = acc[k];
    }
  }
}

template <int NB, bool TW>
void launch_jvp(const BinnedArgs& a, const BinnedTangent& t, torch::Tensor& out,
                hipStream_t stream) {
  launch_slab_fwd<binned_jvp_kernel<NB, TW>>(blocks_for(a.n), ReduceFwd{NB, NB, 1, NB, 1, a.nb},
                                             out.data_ptr<float>(), out, stream, a, t);
}

}  // namespace

// The tangent [nb] of binned_forward(mu, sigma, w, edges) along (tmu, tsigma, tw); an absent
// tangent is a zero, and at least one must be present.
torch::Tensor binned_jvp(torch::Tensor mu, torch::Tensor sigma, c10::optional<torch::Tensor> w,
                         std::vector<double> edges, c10::optional<torch::Tensor> tmu,
                         c10::optional<torch::Tensor> tsigma, c10::optional<torch::Tensor> tw) {
  BinnedArgs a = make_args(mu, sigma, w, edges);
  TORCH_CHECK(a.n > 0, "binned_jvp: empty input");
  BinnedTangent t;
  t.tmu = optional_operand(tmu, "the tangent of mu", a.n);
  t.tsigma = optional_operand(tsigma, "the tangent of sigma", sigma.numel());
  TORCH_CHECK(a.w != nullptr || !tw.has_value() || !tw->defined(),
              "binned_jvp: a weights tangent without weights");
  t.tw = optional_operand(tw, "the tangent of the weights", a.w != nullptr ? w->numel() : 0);
  TORCH_CHECK(t.tmu != nullptr || t.tsigma != nullptr || t.tw != nullptr, "no tangent given");
  if (t.tmu == nullptr && t.tsigma == nullptr)  // linear in w: the forward with tw as weights
    return binned_forward(mu, sigma, *tw, edges);
  a.vec = a.vec && (t.tmu == nullptr || aligned16(t.tmu)) &&
          (t.tsigma == nullptr || a.sig_b || aligned16(t.tsigma)) &&
          (t.tw == nullptr || a.w_b || aligned16(t.tw));
  auto out = torch::empty({a.nb}, mu.options());
  const int nbp = padded_bins(a.nb, "gaussian_binned_sum");
  auto stream = at::hip::getCurrentHIPStream();
  MG_DISPATCH_BINNED(nbp, {
    if (t.tw != nullptr) launch_jvp<NB, true>(a, t, out, stream);
    else launch_jvp<NB, false>(a, t, out, stream);
  });
  return out;
}

}  // namespace mg
