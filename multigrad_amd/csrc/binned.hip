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

struct BinnedGrad {
  const float* g;  // [nb] cotangent
  float* dmu;      // [n]
  float* dsigma;   // [n], or [1] when sigma is broadcast
  float* dw;       // [n], or [1] when w is broadcast
  float* slab;     // [blocks, 2] partial sums of the broadcast gradients (col 0 sigma, col 1 w)
};

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

// Fixed-order sum of slab rows [rows, ncols] (ncols a power of two <= 32) by one workgroup
// (slab_column_sum).  Columns [0, na) go to out_a, column na to out_b (either may be null:
// the column is dropped).
__global__ __launch_bounds__(kRedThreads) void binned_reduce_kernel(const float* slab, int64_t rows,
                                                                    int ncols, float* out_a, int na,
                                                                    float* out_b) {
  __shared__ float part[kRedThreads];
  float t;
  if (slab_column_sum(slab, rows, ncols, 0, ncols, part, t)) {
    const int k = threadIdx.x;
    if (k < na) {
      if (out_a) out_a[k] = t;
    } else if (k == na && out_b) {
      out_b[0] = t;
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
    const bool full = i0 + 4 <= a.n;
    float dm[4], ds[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float c = -kInvSqrt2PiB * wt[j] * inv[j];  // 0 beyond N (weight 0)
      dm[j] = c * A[j];
      ds[j] = c * B[j];
      if (i0 + j >= a.n) C[j] = 0.0f;
    }
    if constexpr (GMU) {
      if (full) {
        *reinterpret_cast<float4*>(o.dmu + i0) = make_float4(dm[0], dm[1], dm[2], dm[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i0 + j < a.n) o.dmu[i0 + j] = dm[j];
      }
    }
    if constexpr (GSIG) {
      if (red_sig) {
        rs[0] += (ds[0] + ds[1]) + (ds[2] + ds[3]);
      } else if (full) {
        *reinterpret_cast<float4*>(o.dsigma + i0) = make_float4(ds[0], ds[1], ds[2], ds[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i0 + j < a.n) o.dsigma[i0 + j] = ds[j];
      }
    }
    if constexpr (GW) {
      if (red_w) {
        rs[1] += (C[0] + C[1]) + (C[2] + C[3]);
      } else if (full) {
        *reinterpret_cast<float4*>(o.dw + i0) = make_float4(C[0], C[1], C[2], C[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i0 + j < a.n) o.dw[i0 + j] = C[j];
      }
    }
  }
  if (red_sig || red_w) {  // uniform over the grid
    block_sum_n<2>(rs, red);
    if (threadIdx.x == 0) {
      if (direct) {
        if (red_sig) o.dsigma[0] = rs[0];
        if (red_w) o.dw[0] = rs[1];
      } else {
        o.slab[(int64_t)blockIdx.x * 2 + 0] = rs[0];
        o.slab[(int64_t)blockIdx.x * 2 + 1] = rs[1];
      }
    }
  }
}

template <auto Kernel>
void launch_bwd(const BinnedArgs& a, BinnedGrad& o, const torch::Tensor& like, bool red_sig,
                bool red_w, hipStream_t stream) {
  const int64_t need = ((a.n + 3) / 4 + kBinThreads - 1) / kBinThreads;
  const int64_t blocks = std::min(need, chip_blocks<Kernel>());
  const bool two = (red_sig || red_w) && blocks > 1;
  torch::Tensor slab;
  if (two) {
    slab = torch::empty({blocks, 2}, like.options());
    o.slab = slab.data_ptr<float>();
  }
  hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(kBinThreads), 0, stream, a, o, blocks == 1 ? 1 : 0);
  if (two)
    hipLaunchKernelGGL(binned_reduce_kernel, dim3(1), dim3(kRedThreads), 0, stream,
                       (const float*)o.slab, blocks, 2, red_sig ? o.dsigma : nullptr, 1,
                       red_w ? o.dw : nullptr);
}

}  // namespace

void launch_binned_reduce(const float* slab, int64_t rows, int ncols, float* out_a, int na,
                          float* out_b, hipStream_t stream) {
  hipLaunchKernelGGL(binned_reduce_kernel, dim3(1), dim3(kRedThreads), 0, stream, slab, rows, ncols,
                     out_a, na, out_b);
}

torch::Tensor binned_forward(torch::Tensor mu, torch::Tensor sigma, c10::optional<torch::Tensor> w,
                             std::vector<double> edges) {
  BinnedArgs a = make_args(mu, sigma, w, edges);
  TORCH_CHECK(a.n > 0, "binned_forward: empty input");
  const int nbp = binned_padded(a.nb);
  auto out = torch::empty({a.nb}, mu.options());
  auto stream = at::hip::getCurrentHIPStream();
  const int64_t need = ((a.n + 3) / 4 + kBinThreads - 1) / kBinThreads;
  MG_DISPATCH_BINNED(nbp, {
    const int64_t blocks = std::min(need, chip_blocks<binned_fwd_kernel<NB>>());
    if (blocks == 1) {
      hipLaunchKernelGGL(binned_fwd_kernel<NB>, dim3(1), dim3(kBinThreads), 0, stream, a,
                         (float*)nullptr, out.data_ptr<float>(), 1);
    } else {
      auto slab = torch::empty({blocks, (int64_t)NB}, mu.options());
      hipLaunchKernelGGL(binned_fwd_kernel<NB>, dim3(blocks), dim3(kBinThreads), 0, stream, a,
                         slab.data_ptr<float>(), (float*)nullptr, 0);
      hipLaunchKernelGGL(binned_reduce_kernel, dim3(1), dim3(kRedThreads), 0, stream,
                         (const float*)slab.data_ptr<float>(), blocks, NB, out.data_ptr<float>(),
                         a.nb, (float*)nullptr);
    }
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
  const int nbp = binned_padded(a.nb);
  torch::Tensor dmu, dsigma, dw;
  BinnedGrad o;
  o.g = g.data_ptr<float>();
  o.dmu = o.dsigma = o.dw = o.slab = nullptr;
  if (need_mu) {
    dmu = torch::empty({a.n}, mu.options());
    o.dmu = dmu.data_ptr<float>();
  }
  if (need_sigma) {
    dsigma = torch::empty({sigma.numel()}, mu.options());
    o.dsigma = dsigma.data_ptr<float>();
  }
  if (need_w) {
    dw = torch::empty({w->numel()}, mu.options());
    o.dw = dw.data_ptr<float>();
  }
  const bool red_sig = need_sigma && a.sig_b, red_w = need_w && a.w_b;
  auto stream = at::hip::getCurrentHIPStream();
  MG_DISPATCH_BINNED(nbp, {
    with_bool(need_mu, [&](auto M) {
      with_bool(need_sigma, [&](auto S) {
        with_bool(need_w, [&](auto W) {
          constexpr bool kM = decltype(M)::value, kS = decltype(S)::value, kW = decltype(W)::value;
          if constexpr (kM || kS || kW)
            launch_bwd<binned_bwd_kernel<NB, kM, kS, kW>>(a, o, mu, red_sig, red_w, stream);
        });
      });
    });
  });
  return std::make_tuple(dmu, dsigma, dw);
}

}  // namespace mg
