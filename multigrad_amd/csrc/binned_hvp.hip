// Second backward of the Gaussian-binned sum (ops/binned.py, _GaussianBinnedSumBackward).
// The first backward maps (mu, sigma, w, g) to
//   dmu = -(w/sigma) M0,  dsigma = -(w/sigma) M1,  dw = sum_e h_e Phi(z_e),
// with z_e = (e_e - mu)/sigma, h_e = g_{e-1} - g_e (g_{-1} = g_nb = 0) and the moments
// M_n = sum_e h_e z_e^n phi(z_e).  Given cotangents a, b, c of (dmu, dsigma, dw) this file
// computes the gradients of sum_i (a_i dmu_i + b_i dsigma_i + c_i dw_i):
//   d/dmu    = (w/sigma^2) [-a M1 + b (M0 - M2)] - c M0/sigma
//   d/dsigma = (w/sigma^2) [ a (M0 - M2) + b (2 M1 - M3)] - c M1/sigma
//   d/dw     = -(a M0 + b M1)/sigma
//   d/dg_k   = T_{k+1} - T_k,  T_e = sum_i [-(w_i/sigma_i)(a_i + b_i z_ie) phi(z_ie) + c_i Phi(z_ie)]
// A missing cotangent is a zero; a broadcast sigma or w has a one-element cotangent that is
// used for every object, and its gradient is the sum over objects.
//
// One recomputing pass in the traversal of binned_bwd_kernel (binned.hip): a grid-stride over
// quads of objects, 16-byte loads and stores, guarded scalar accesses for a misaligned view
// and the last N % 4 objects, no residuals.  The gradient of g is accumulated per bin (the
// difference of the edge term between consecutive edges, the Phi part from the base/frac
// split of edge_cdf as in the forward), so its slab has a power-of-two column count <= 32:
// block_sum_n -> slab row -> the fixed-order reduce of binned.hip.  Gradients of broadcast
// operands go through the two-column slab of the first backward.  No float atomics: results
// are bitwise reproducible for a fixed N and device.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <tuple>
#include <vector>

#include "binned_host.h"

namespace mg {

namespace {

struct Binned2 {
  const float* g;  // [nb] cotangent of the forward
  const float* a;  // [n] cotangent of dmu; nullptr: zero
  const float* b;  // [n], or [1] when sigma is broadcast: cotangent of dsigma; nullptr: zero
  const float* c;  // [n], or [1] when w is broadcast: cotangent of dw; nullptr: zero
  float* gmu;      // [n]; nullptr: not wanted
  float* gsigma;   // [n], or [1] when sigma is broadcast; nullptr: not wanted
  float* gw;       // [n], or [1] when w is broadcast; nullptr: not wanted
  float* gg;       // [nb]; nullptr: not wanted
  float* slab_b;   // [blocks, 2] partial sums of the broadcast gradients (col 0 sigma, col 1 w)
  float* slab_g;   // [blocks, NB] partial sums of the gradient of g
};

// The moments and the gradients of mu, sigma and w are always formed (autograd asks for this
// pass only when one of them requires grad); which of the three is stored is a wave-uniform
// test on its pointer.
// GG : the gradient of g is wanted (per-bin accumulators).
// CDF: GG with a cotangent c, the only case that evaluates Phi; otherwise one v_exp per edge.
template <int NB, bool GG, bool CDF>
__global__ __launch_bounds__(kBinThreads) void binned_bwd2_kernel(BinnedArgs a, Binned2 o,
                                                                  int direct) {
  static_assert(GG || !CDF, "Phi only feeds the gradient of g");
  __shared__ float red[(GG ? NB : 2) * (kBinThreads / kWave)];
  // the edge weights h_e = g_{e-1} - g_e (g_{-1} = g_{nb} = 0)
  float g[NB], h[NB + 1];
#pragma unroll
  for (int k = 0; k < NB; ++k) g[k] = k < a.nb ? o.g[k] : 0.0f;
  h[0] = -g[0];
#pragma unroll
  for (int e = 1; e < NB; ++e) h[e] = g[e - 1] - g[e];
  h[NB] = g[NB - 1];
  const bool red_sig = o.gsigma != nullptr && a.sig_b;
  const bool red_w = o.gw != nullptr && a.w_b;
  float rs[2] = {0.0f, 0.0f};  // this thread's share of the broadcast gradients
  float acc[NB];               // this thread's share of the gradient of g, per bin
#pragma unroll
  for (int k = 0; k < NB; ++k) acc[k] = 0.0f;
  const int64_t nq = (a.n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < nq; q += stride) {
    const int64_t i0 = q * 4;
    const bool full = a.vec && i0 + 4 <= a.n;  // a.vec covers the cotangents too
    float m[4], inv[4], wt[4], ca[4], cb[4], cc[4];
    load_quad(a, q, m, inv, wt);
    // objects beyond N: weight 0 and cotangents 0, so every term below vanishes
    load_group<4>(o.a, i0, a.n, full, false, 0.0f, 0.0f, ca);
    load_group<4>(o.b, i0, a.n, full, a.sig_b, 0.0f, 0.0f, cb);
    load_group<4>(o.c, i0, a.n, full, a.w_b, 0.0f, 0.0f, cc);
    float M0[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sum_e h_e z_e^n exp(-z_e^2/2), n = 0..3
    float M1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float M2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float M3[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float ua[4], ub[4], u0[4], b0[4], f0[4];
    if constexpr (GG) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // edge term u_e = (ua + ub z_e) exp(-z_e^2/2)
        const float s = -kInvSqrt2PiB * wt[j] * inv[j];
        ua[j] = s * ca[j];
        ub[j] = s * cb[j];
      }
    }
#pragma unroll
    for (int e = 0; e <= NB; ++e) {
      if (e <= a.nb) {  // wave-uniform: padded bins cost nothing
        float d = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float z = (a.edge[e] - m[j]) * inv[j];
          float gs, b1, f1;
          if constexpr (CDF) {
            edge_cdf(z, b1, f1, gs);
          } else {
            const float ws = z * kWScale;
            gs = fast_exp2(-ws * ws);
          }
          const float t0 = h[e] * gs, t1 = t0 * z, t2 = t1 * z;
          M0[j] += t0;
          M1[j] += t1;
          M2[j] += t2;
          M3[j] = fmaf(t2, z, M3[j]);
          if constexpr (GG) {
            const float u = fmaf(ub[j], z, ua[j]) * gs;
            if (e > 0) {
              float dj = u - u0[j];
              if constexpr (CDF) dj = fmaf(cc[j], (b1 - b0[j]) + (f1 - f0[j]), dj);
              d += dj;
            }
            u0[j] = u;
            if constexpr (CDF) {
              b0[j] = b1;
              f0[j] = f1;
            }
          }
        }
        if constexpr (GG)
          if (e > 0) acc[e > 0 ? e - 1 : 0] += d;  // a constant index once unrolled
      }
    }
    float gm[4], gs[4], gw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float r = kInvSqrt2PiB * inv[j];  // phi's normalisation and one 1/sigma
      const float wr = wt[j] * inv[j] * r;    // 0 beyond N (weight 0)
      const float cr = cc[j] * r;
      const float d02 = M0[j] - M2[j];
      gm[j] = wr * (cb[j] * d02 - ca[j] * M1[j]) - cr * M0[j];
      gs[j] = wr * (ca[j] * d02 + cb[j] * (2.0f * M1[j] - M3[j])) - cr * M1[j];
      gw[j] = -r * (ca[j] * M0[j] + cb[j] * M1[j]);
    }
    if (o.gmu != nullptr) store_group<4>(o.gmu, i0, a.n, gm);
    if (o.gsigma != nullptr) put_quad(red_sig, rs[0], o.gsigma, i0, a.n, gs);
    if (o.gw != nullptr) put_quad(red_w, rs[1], o.gw, i0, a.n, gw);
  }
  finish_broadcast(rs, red, red_sig, red_w, o.gsigma, o.gw, o.slab_b, direct);
  if constexpr (GG) {
    __syncthreads();  // `red` may still be read by thread 0 of the sum above
    block_sum_n<NB>(acc, red);
    if (threadIdx.x == 0) {
      if (direct) {
#pragma unroll
        for (int k = 0; k < NB; ++k)
          if (k < a.nb) o.gg[k] = acc[k];
      } else {
#pragma unroll
        for (int k = 0; k < NB; ++k) o.slab_g[(int64_t)blockIdx.x * NB + k] = acc[k];
      }
    }
  }
}

template <auto Kernel, int NB, bool GG>
void launch_bwd2(const BinnedArgs& a, Binned2& o, const torch::Tensor& like, bool red_b,
                 hipStream_t stream) {
  const int64_t blocks = std::min(blocks_for(a.n), chip_blocks<Kernel>());
  const bool two = blocks > 1;
  torch::Tensor slab_b, slab_g;
  if (two && red_b) {
    slab_b = torch::empty({blocks, 2}, like.options());
    o.slab_b = slab_b.data_ptr<float>();
  }
  if (two && GG) {
    slab_g = torch::empty({blocks, (int64_t)NB}, like.options());
    o.slab_g = slab_g.data_ptr<float>();
  }
  hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(kBinThreads), 0, stream, a, o, two ? 0 : 1);
  if (two && red_b)
    launch_reduce_bwd(o.slab_b, blocks, 2,
                      reduce_sigma_w(a.sig_b ? o.gsigma : nullptr, a.w_b ? o.gw : nullptr), stream);
  if (two && GG)
    launch_reduce_fwd(o.slab_g, blocks, ReduceFwd{NB, NB, 1, NB, 1, a.nb}, o.gg, stream);
}

}  // namespace

// Gradients of sum_i (a_i dmu_i + b_i dsigma_i + c_i dw_i), where (dmu, dsigma, dw) is what
// binned_backward returns for the cotangent g, with respect to the requested ones of (mu,
// sigma, w, g); one that was not requested comes back undefined (None).  An absent cotangent
// is a zero.  A broadcast operand gets the sum over objects.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> binned_backward2(
    torch::Tensor mu, torch::Tensor sigma, c10::optional<torch::Tensor> w, std::vector<double> edges,
    torch::Tensor g, c10::optional<torch::Tensor> ca, c10::optional<torch::Tensor> cb,
    c10::optional<torch::Tensor> cc, bool need_mu, bool need_sigma, bool need_w, bool need_g) {
  BinnedArgs a = make_args(mu, sigma, w, edges);
  TORCH_CHECK(a.n > 0, "binned_backward2: empty input");
  check_dev(g, "grad_out", at::kFloat);
  TORCH_CHECK(g.numel() == a.nb, "grad_out must have nb elements");
  TORCH_CHECK(!need_w || a.w != nullptr, "weights gradient requested without weights");
  TORCH_CHECK(need_mu || need_sigma || need_w || need_g, "no gradient requested");
  Binned2 o = {};
  o.g = g.data_ptr<float>();
  o.a = optional_operand(ca, "the cotangent of dmu", a.n);
  o.b = optional_operand(cb, "the cotangent of dsigma", sigma.numel());
  o.c = optional_operand(cc, "the cotangent of dw", a.w != nullptr ? w->numel() : 0);
  TORCH_CHECK(o.a != nullptr || o.b != nullptr || o.c != nullptr, "no cotangent given");
  a.vec = a.vec && (o.a == nullptr || aligned16(o.a)) &&
          (o.b == nullptr || a.sig_b || aligned16(o.b)) &&
          (o.c == nullptr || a.w_b || aligned16(o.c));
  auto gmu = alloc_grad(need_mu, a.n, mu, o.gmu);
  auto gsigma = alloc_grad(need_sigma, sigma.numel(), mu, o.gsigma);
  auto gw = alloc_grad(need_w, need_w ? w->numel() : 0, mu, o.gw);
  auto gg = alloc_grad(need_g, a.nb, mu, o.gg);
  const bool cdf = need_g && o.c != nullptr;
  const bool red_b = (need_sigma && a.sig_b) || (need_w && a.w_b);
  const int nbp = padded_bins(a.nb, "gaussian_binned_sum");
  auto stream = at::hip::getCurrentHIPStream();
  MG_DISPATCH_BINNED(nbp, {
    with_bool(need_g, [&](auto G) {
      with_bool(cdf, [&](auto C) {
        constexpr bool kG = decltype(G)::value, kC = decltype(C)::value;
        if constexpr (kG || !kC)
          launch_bwd2<binned_bwd2_kernel<NB, kG, kC>, NB, kG>(a, o, mu, red_b, stream);
      });
    });
  });
  return std::make_tuple(gmu, gsigma, gw, gg);
}

}  // namespace mg
