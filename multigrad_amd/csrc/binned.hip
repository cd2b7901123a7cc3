// Gaussian-binned sum for user-written models (ops/binned.py):
//   out[k] = sum_i w_i * (Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i))
// with per-object mu, sigma and weight tensors produced by arbitrary torch code.
//
// Forward : grid-stride over quads of objects (16-byte loads), per-thread fp32 bin
//           accumulators in registers, block_sum_n into one slab row per workgroup, then a
//           fixed-order reduction of the rows by a second one-workgroup kernel (a single
//           launch when one workgroup covers the input).
// Backward: the same traversal, recomputing from mu/sigma/w (no residuals); per-object
//           gradients are stored 16 bytes at a time, gradients of broadcast operands go
//           through the same block sum -> slab -> fixed-order reduce.
// No float atomics anywhere: results are bitwise reproducible for a fixed N and device.
// Phi is evaluated with normal_tail_parts_w<false> (common.h), the absolute-accuracy class
// of the float32 erf.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <tuple>
#include <vector>

#include "binned_host.h"

namespace mg {

namespace {

template <int NB>
__global__ __launch_bounds__(kBinThreads) void binned_fwd_kernel(BinnedArgs a, float* slab,
                                                                 float* out, int direct) {
  __shared__ float red[NB * (kBinThreads / kWave)];
  float acc[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) acc[k] = 0.0f;
  const int64_t nq = (a.n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < nq; q += stride) {
    float m[4], inv[4], wt[4], b0[4], f0[4];
    load_quad(a, q, m, inv, wt);
#pragma unroll
    for (int e = 0; e <= NB; ++e) {
      if (e <= a.nb) {  // wave-uniform: padded bins cost nothing
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float b1, f1, gs;
          edge_cdf((a.edge[e] - m[j]) * inv[j], b1, f1, gs);
          if (e > 0) {
            float& dst = acc[e > 0 ? e - 1 : 0];  // a constant index once unrolled
            dst = fmaf(wt[j], (b1 - b0[j]) + (f1 - f0[j]), dst);
          }
          b0[j] = b1;
          f0[j] = f1;
        }
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

template <int NB, bool GMU, bool GSIG, bool GW>
__global__ __launch_bounds__(kBinThreads) void binned_bwd_kernel(BinnedArgs a, BinnedGrad o,
                                                                 int direct) {
  __shared__ float red[2 * (kBinThreads / kWave)];
  // cotangent per bin and the edge weights h_e = g_{e-1} - g_e (g_{-1} = g_{nb} = 0)
  float g[NB], h[NB + 1];
#pragma unroll
  for (int k = 0; k < NB; ++k) g[k] = k < a.nb ? o.g[k] : 0.0f;
  h[0] = -g[0];
#pragma unroll
  for (int e = 1; e < NB; ++e) h[e] = g[e - 1] - g[e];
  h[NB] = g[NB - 1];
  const bool red_sig = GSIG && a.sig_b, red_w = GW && a.w_b;
  float rs[2] = {0.0f, 0.0f};  // this thread's share of the broadcast gradients
  const int64_t nq = (a.n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < nq; q += stride) {
    float m[4], inv[4], wt[4], b0[4], f0[4];
    float A[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sum_e h_e exp(-z_e^2/2)
    float B[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sum_e h_e z_e exp(-z_e^2/2)
    float C[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sum_k g_k dPhi_k
    load_quad(a, q, m, inv, wt);
#pragma unroll
    for (int e = 0; e <= NB; ++e) {
      if (e <= a.nb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float z = (a.edge[e] - m[j]) * inv[j];
          float gs;
          if constexpr (GW) {
            float b1, f1;
            edge_cdf(z, b1, f1, gs);
            if (e > 0) C[j] = fmaf(g[e > 0 ? e - 1 : 0], (b1 - b0[j]) + (f1 - f0[j]), C[j]);
            b0[j] = b1;
            f0[j] = f1;
          } else {
            const float ws = z * kWScale;
            gs = fast_exp2(-ws * ws);
          }
          const float hg = h[e] * gs;
          if constexpr (GMU) A[j] += hg;
          if constexpr (GSIG) B[j] = fmaf(hg, z, B[j]);
        }
      }
    }
    const int64_t i0 = q * 4;
    float dm[4], ds[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float c = -kInvSqrt2PiB * wt[j] * inv[j];  // 0 beyond N (weight 0)
      dm[j] = c * A[j];
      ds[j] = c * B[j];
      if (i0 + j >= a.n) C[j] = 0.0f;
    }
    if constexpr (GMU) store_group<4>(o.dmu, i0, a.n, dm);
    if constexpr (GSIG) put_quad(red_sig, rs[0], o.dsigma, i0, a.n, ds);
    if constexpr (GW) put_quad(red_w, rs[1], o.dw, i0, a.n, C);
  }
  finish_broadcast(rs, red, red_sig, red_w, o.dsigma, o.dw, o.slab, direct);
}

}  // namespace

torch::Tensor binned_forward(torch::Tensor mu, torch::Tensor sigma, c10::optional<torch::Tensor> w,
                             std::vector<double> edges) {
  BinnedArgs a = make_args(mu, sigma, w, edges);
  TORCH_CHECK(a.n > 0, "binned_forward: empty input");
  const int nbp = padded_bins(a.nb, "gaussian_binned_sum");
  auto out = torch::empty({a.nb}, mu.options());
  auto stream = at::hip::getCurrentHIPStream();
  MG_DISPATCH_BINNED(nbp, {
    launch_slab_fwd<binned_fwd_kernel<NB>>(blocks_for(a.n), ReduceFwd{NB, NB, 1, NB, 1, a.nb},
                                           out.data_ptr<float>(), mu, stream, a);
  });
  return out;
}

// Gradients of sum_k g_k out_k with respect to the requested operands; an operand that was
// not requested comes back undefined (None).  A broadcast operand gets the sum over objects.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> binned_backward(
    torch::Tensor mu, torch::Tensor sigma, c10::optional<torch::Tensor> w, std::vector<double> edges,
    torch::Tensor g, bool need_mu, bool need_sigma, bool need_w) {
  BinnedArgs a = make_args(mu, sigma, w, edges);
  TORCH_CHECK(a.n > 0, "binned_backward: empty input");
  check_dev(g, "grad_out", at::kFloat);
  TORCH_CHECK(g.numel() == a.nb, "grad_out must have nb elements");
  TORCH_CHECK(!need_w || a.w != nullptr, "weights gradient requested without weights");
  TORCH_CHECK(need_mu || need_sigma || need_w, "no gradient requested");
  const int nbp = padded_bins(a.nb, "gaussian_binned_sum");
  BinnedGrad o = {};
  o.g = g.data_ptr<float>();
  auto dmu = alloc_grad(need_mu, a.n, mu, o.dmu);
  auto dsigma = alloc_grad(need_sigma, sigma.numel(), mu, o.dsigma);
  auto dw = alloc_grad(need_w, need_w ? w->numel() : 0, mu, o.dw);
  const auto r = reduce_sigma_w(a.sig_b ? o.dsigma : nullptr, a.w_b ? o.dw : nullptr);
  auto stream = at::hip::getCurrentHIPStream();
  MG_DISPATCH_BINNED(nbp, {
    with_need3(need_mu, need_sigma, need_w, [&](auto M, auto S, auto W) {
      launch_slab_bwd<binned_bwd_kernel<NB, decltype(M)::value, decltype(S)::value,
                                        decltype(W)::value>>(a, o, blocks_for(a.n), 2, r, mu,
                                                             stream);
    });
  });
  return std::make_tuple(dmu, dsigma, dw);
}

}  // namespace mg
