// Multi-channel Gaussian-binned sum for user-written models (ops/binned_multi.py):
//   out[c][k] = sum_i w_{c,i} * (Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i))
// for C weight channels over the same per-object bin masses.  The edge CDFs (one v_rcp + one
// v_exp each, the dominant cost of binned.hip) are evaluated once per object; each channel
// adds one FMA per bin.
//
// Channels are processed in blocks of up to kChanBlock = 4 (one launch per block: C <= 4 is a
// single pass, C <= 8 two).  The traversal is that of binned.hip: a grid-stride over quads
// of objects, 16-byte loads when every operand of the pass is aligned, guarded scalar loads
// for misaligned views and the last N % 4 objects.
// Forward : per-thread accumulators acc[c][k] in registers, block_sum_n into one slab row
//           [CB * NB] per workgroup, then a fixed-order column reduce (one workgroup per
//           channel); a single launch when one workgroup covers the input.
// Backward: one recomputing pass per channel block, no residuals.  The cotangent rows and the
//           edge weights h_c[e] = g[c][e-1] - g[c][e] are staged once per workgroup in LDS as
//           [edge][channel] quads (one broadcast 16-byte read per edge).  Per object and edge
//           H = sum_c w_c h_c[e] is formed in registers, so dmu / dsigma are the channel sums
//           and are stored once; a later pass adds into what the earlier one stored (load,
//           add, store by the same launch order: fixed).  Whether a channel's dw is stored is
//           a wave-uniform test on its pointer.  Gradients of broadcast operands (sigma and up
//           to four weights) go block sum -> [blocks, 8] slab -> fixed-order reduce.
// No float atomics anywhere: results are bitwise reproducible for a fixed N, C, shape and
// device.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <vector>

#include "binned_host.h"

namespace mg {

namespace {

constexpr int kChanBlock = 4;   // channels per pass
constexpr int kMaxChannels = 8;
constexpr int kRedCols = 8;     // backward slab row: sigma, four weights, three unused

struct MultiArgs {
  const float* mu;
  const float* sigma;
  const float* w[kChanBlock];  // nullptr: every weight of the channel is 1
  int64_t n;
  int nb;     // real bins (<= the padded template count)
  int nc;     // real channels of this pass (<= the template block)
  int sig_b;  // sigma has one element
  int w_b;    // bit c: w[c] has one element
  int vec;    // every per-object input pointer of the pass is 16-byte aligned
  float edge[kMaxBins + 1];
};

struct MultiGrad {
  const float* g;          // [nc, nb] cotangent rows of this pass
  float* dmu;              // [n]
  float* dsigma;           // [n], or [1] when sigma is broadcast
  float* dw[kChanBlock];   // [n] or [1] per channel; nullptr: not wanted
  float* slab;             // [blocks, kRedCols] partial sums of the broadcast gradients
  int accum;               // an earlier pass stored dmu / dsigma: add into them
};

// Mean and 1/sigma of the four objects of a quad; objects beyond N get mean 0, sigma 1.
__device__ __forceinline__ void load_mean_width(const MultiArgs& a, int64_t i0, bool full,
                                                float (&m)[4], float (&inv)[4]) {
  float s[4];
  load_group<4>(a.mu, i0, a.n, full, false, 0.0f, 0.0f, m);
  load_group<4>(a.sigma, i0, a.n, full, a.sig_b, 1.0f, 1.0f, s);
#pragma unroll
  for (int j = 0; j < 4; ++j) inv[j] = 1.0f / s[j];
}

template <int NB, int CB>
__global__ __launch_bounds__(kBinThreads) void binned_multi_fwd_kernel(MultiArgs a, float* slab,
                                                                       float* out, int direct) {
  __shared__ float red[CB * NB * (kBinThreads / kWave)];
  float acc[CB * NB];
#pragma unroll
  for (int k = 0; k < CB * NB; ++k) acc[k] = 0.0f;
  const int64_t nq = (a.n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < nq; q += stride) {
    const int64_t i0 = q * 4;
    const bool full = a.vec && i0 + 4 <= a.n;  // one branch for all operands
    float m[4], inv[4], wt[CB][4], b0[4], f0[4];
    load_mean_width(a, i0, full, m, inv);
#pragma unroll
    for (int c = 0; c < CB; ++c)
      if (c < a.nc)  // wave-uniform: padded channels cost nothing; objects beyond N weigh 0
        load_group<4>(a.w[c], i0, a.n, full, (a.w_b >> c) & 1, 1.0f, 0.0f, wt[c]);
#pragma unroll
    for (int e = 0; e <= NB; ++e) {
      if (e <= a.nb) {  // wave-uniform: padded bins cost nothing
        float d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float b1, f1, gs;
          edge_cdf((a.edge[e] - m[j]) * inv[j], b1, f1, gs);
          if (e > 0) d[j] = (b1 - b0[j]) + (f1 - f0[j]);
          b0[j] = b1;
          f0[j] = f1;
        }
        if (e > 0) {
#pragma unroll
          for (int c = 0; c < CB; ++c) {
            if (c < a.nc) {
              float& dst = acc[c * NB + (e > 0 ? e - 1 : 0)];  // a constant index once unrolled
#pragma unroll
              for (int j = 0; j < 4; ++j) dst = fmaf(wt[c][j], d[j], dst);
            }
          }
        }
      }
    }
  }
  block_sum_n<CB * NB>(acc, red);
  if (threadIdx.x == 0) {
    if (direct) {
#pragma unroll
      for (int c = 0; c < CB; ++c)
#pragma unroll
        for (int k = 0; k < NB; ++k)
          if (c < a.nc && k < a.nb) out[c * a.nb + k] = acc[c * NB + k];
    } else {
#pragma unroll
      for (int k = 0; k < CB * NB; ++k) slab[(int64_t)blockIdx.x * (CB * NB) + k] = acc[k];
    }
  }
}

// V results added to / stored over p[i0 .. i0+V) (p is a fresh allocation, hence aligned).
__device__ __forceinline__ void put_group(float* p, int64_t i0, int64_t n, bool add,
                                          float (&v)[4]) {
  if (add) {
    float old[4];
    load_group<4>(p, i0, n, i0 + 4 <= n, false, 0.0f, 0.0f, old);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = old[j] + v[j];
  }
  store_group<4>(p, i0, n, v);
}

// GW: some channel of the pass wants its weight gradient (the CDF is evaluated; otherwise
// only the Gaussian).
template <int NB, int CB, bool GMU, bool GSIG, bool GW>
__global__ __launch_bounds__(kBinThreads) void binned_multi_bwd_kernel(MultiArgs a, MultiGrad o,
                                                                       int direct) {
  static_assert(CB == 2 || CB == 4, "channel quads / pairs in LDS");
  // cotangent per bin and the edge weights h_e = g_{e-1} - g_e (g_{-1} = g_{nb} = 0), per
  // edge one group of CB channels (zero for padded bins and channels)
  __shared__ __attribute__((aligned(16))) float gl[NB * CB];
  __shared__ __attribute__((aligned(16))) float hl[(NB + 1) * CB];
  __shared__ float red[(1 + CB) * (kBinThreads / kWave)];
  for (int t = threadIdx.x; t < (NB + 1) * CB; t += kBinThreads) {
    const int e = t / CB, c = t % CB;
    const bool ch = c < a.nc;
    const float lo = ch && e > 0 && e <= a.nb ? o.g[c * a.nb + e - 1] : 0.0f;
    const float hi = ch && e < a.nb ? o.g[c * a.nb + e] : 0.0f;
    hl[t] = lo - hi;
    if (e < NB) gl[t] = hi;
  }
  __syncthreads();
  const bool red_sig = GSIG && a.sig_b;
  bool red_w = false;  // some broadcast weight wants its gradient (the host's test for the slab)
  if constexpr (GW) {
#pragma unroll
    for (int c = 0; c < CB; ++c) red_w = red_w || (((a.w_b >> c) & 1) && o.dw[c] != nullptr);
  }
  float rs[1 + CB];  // this thread's share of the broadcast gradients
#pragma unroll
  for (int k = 0; k <= CB; ++k) rs[k] = 0.0f;
  const int64_t nq = (a.n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < nq; q += stride) {
    const int64_t i0 = q * 4;
    const bool full = a.vec && i0 + 4 <= a.n;
    float m[4], inv[4], wt[CB][4], b0[4], f0[4];
    float A[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sum_e H_e exp(-z_e^2/2), H_e = sum_c w_c h_c[e]
    float B[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sum_e H_e z_e exp(-z_e^2/2)
    float Cw[CB][4];                        // sum_k g_c[k] dPhi_k
    load_mean_width(a, i0, full, m, inv);
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      if (c < a.nc) load_group<4>(a.w[c], i0, a.n, full, (a.w_b >> c) & 1, 1.0f, 0.0f, wt[c]);
#pragma unroll
      for (int j = 0; j < 4; ++j) Cw[c][j] = 0.0f;
    }
#pragma unroll
    for (int e = 0; e <= NB; ++e) {
      if (e <= a.nb) {
        // One broadcast LDS read per table and edge (a uniform address).  The reads are
        // volatile so that they stay here: hoisted out of the object loop, the tables would
        // occupy 2 * CB * NB registers per thread.
        using Group = float __attribute__((ext_vector_type(CB)));
        Group hv = {}, gv = {};
        if constexpr (GMU || GSIG) hv = *reinterpret_cast<const volatile Group*>(hl + e * CB);
        if constexpr (GW)
          if (e > 0) gv = *reinterpret_cast<const volatile Group*>(gl + (e > 0 ? e - 1 : 0) * CB);
        float hc[CB], gc[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) {
          hc[c] = hv[c];
          gc[c] = gv[c];
        }
        float z[4], gs[4], d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          z[j] = (a.edge[e] - m[j]) * inv[j];
          if constexpr (GW) {
            float b1, f1;
            edge_cdf(z[j], b1, f1, gs[j]);
            if (e > 0) d[j] = (b1 - b0[j]) + (f1 - f0[j]);
            b0[j] = b1;
            f0[j] = f1;
          } else {
            const float ws = z[j] * kWScale;
            gs[j] = fast_exp2(-ws * ws);
          }
        }
        float H[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < CB; ++c) {
          if (c < a.nc) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if constexpr (GW)
                if (e > 0) Cw[c][j] = fmaf(gc[c], d[j], Cw[c][j]);
              if constexpr (GMU || GSIG) H[j] = fmaf(wt[c][j], hc[c], H[j]);
            }
          }
        }
        if constexpr (GMU || GSIG) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float hg = H[j] * gs[j];
            if constexpr (GMU) A[j] += hg;
            if constexpr (GSIG) B[j] = fmaf(hg, z[j], B[j]);
          }
        }
      }
    }
    float dm[4], ds[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float s = -kInvSqrt2PiB * inv[j];  // the weights are inside H: 0 beyond N
      dm[j] = s * A[j];
      ds[j] = s * B[j];
    }
    if constexpr (GMU) put_group(o.dmu, i0, a.n, o.accum, dm);
    if constexpr (GSIG) {
      if (red_sig) rs[0] += (ds[0] + ds[1]) + (ds[2] + ds[3]);
      else put_group(o.dsigma, i0, a.n, o.accum, ds);
    }
    if constexpr (GW) {
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        if (o.dw[c] != nullptr) {  // wave-uniform
          if ((a.w_b >> c) & 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (i0 + j >= a.n) Cw[c][j] = 0.0f;
            rs[1 + c] += (Cw[c][0] + Cw[c][1]) + (Cw[c][2] + Cw[c][3]);
          } else {
            store_group<4>(o.dw[c], i0, a.n, Cw[c]);
          }
        }
      }
    }
  }
  if (red_sig || red_w) {  // uniform over the grid
    block_sum_n<1 + CB>(rs, red);
    if (threadIdx.x == 0) {
      if (direct) {
        if (red_sig) o.dsigma[0] = o.accum ? o.dsigma[0] + rs[0] : rs[0];
#pragma unroll
        for (int c = 0; c < CB; ++c)
          if (GW && ((a.w_b >> c) & 1) && o.dw[c] != nullptr) o.dw[c][0] = rs[1 + c];
      } else {
        float* row = o.slab + (int64_t)blockIdx.x * kRedCols;
#pragma unroll
        for (int k = 0; k < kRedCols; ++k) row[k] = k <= CB ? rs[k <= CB ? k : 0] : 0.0f;
      }
    }
  }
}

constexpr const char* kOpMulti = "gaussian_binned_sum_multi";

#define MG_DISPATCH_MULTI(NBP, NC, ...)                                         \
  switch ((NBP) * 2 + ((NC) > 2 ? 1 : 0)) {                                     \
    case 8: { constexpr int NB = 4, CB = 2; __VA_ARGS__; break; }               \
    case 9: { constexpr int NB = 4, CB = 4; __VA_ARGS__; break; }               \
    case 16: { constexpr int NB = 8, CB = 2; __VA_ARGS__; break; }              \
    case 17: { constexpr int NB = 8, CB = 4; __VA_ARGS__; break; }              \
    case 32: { constexpr int NB = 16, CB = 2; __VA_ARGS__; break; }             \
    case 33: { constexpr int NB = 16, CB = 4; __VA_ARGS__; break; }             \
    case 64: { constexpr int NB = 32, CB = 2; __VA_ARGS__; break; }             \
    default: { constexpr int NB = 32, CB = 4; __VA_ARGS__; break; }             \
  }

using Weights = std::vector<c10::optional<torch::Tensor>>;

// The operands shared by every pass (vec: mu and sigma are wide); with_channels adds a pass's
// weights.
MultiArgs make_multi_args(const torch::Tensor& mu, const torch::Tensor& sigma,
                          const Weights& w, const std::vector<double>& edges) {
  const int64_t C = (int64_t)w.size();
  MultiArgs a;
  a.n = mu.numel();
  a.nb = (int)edges.size() - 1;
  bool wide = true;
  int none = 0;
  a.mu = operand(mu, "mu", a.n, none, wide);
  a.sigma = operand(sigma, "sigma", a.n, a.sig_b, wide);
  a.vec = wide;
  TORCH_CHECK(C >= 1 && C <= kMaxChannels, kOpMulti, ": 1 <= C <= ", kMaxChannels,
              " weight channels, got ", C);
  padded_bins(a.nb, kOpMulti);
  set_edges(edges, a.nb, a.edge, kOpMulti);
  for (const auto& t : w) {
    if (t.has_value() && t->defined()) {
      check_dev(*t, "weights", at::kFloat);
      operand(*t, "every weights entry", a.n, none, wide);
    }
  }
  return a;
}

// The arguments of the pass over channels [c0, c0 + nc) of `w` (checked by make_multi_args).
MultiArgs with_channels(MultiArgs a, const Weights& w, int c0, int nc) {
  a.nc = nc;
  a.w_b = 0;
  bool wide = a.vec;
  for (int c = 0; c < kChanBlock; ++c) {
    a.w[c] = nullptr;
    if (c >= nc) continue;
    const auto& t = w[c0 + c];
    if (!t.has_value() || !t->defined()) continue;
    int b = 0;
    a.w[c] = operand(*t, "every weights entry", a.n, b, wide);
    a.w_b |= b << c;
  }
  a.vec = wide;
  return a;
}

}  // namespace

// out[C, nb]; weights[c] undefined / None stands for the constant 1.
torch::Tensor binned_multi_forward(torch::Tensor mu, torch::Tensor sigma, Weights weights,
                                   std::vector<double> edges) {
  const MultiArgs base = make_multi_args(mu, sigma, weights, edges);
  TORCH_CHECK(base.n > 0, "binned_multi_forward: empty input");
  const int C = (int)weights.size();
  const int nb = base.nb, nbp = padded_bins(nb, kOpMulti);
  auto out = torch::empty({(int64_t)C, (int64_t)nb}, mu.options());
  auto stream = at::hip::getCurrentHIPStream();
  for (int c0 = 0; c0 < C; c0 += kChanBlock) {
    const int nc = std::min(kChanBlock, C - c0);
    const MultiArgs a = with_channels(base, weights, c0, nc);
    MG_DISPATCH_MULTI(nbp, nc, {
      launch_slab_fwd<binned_multi_fwd_kernel<NB, CB>>(
          blocks_for(a.n), ReduceFwd{CB * NB, NB, nc, NB, nc, nb},
          out.data_ptr<float>() + (int64_t)c0 * nb, mu, stream, a);
    });
  }
  return out;
}

// Gradients of sum_ck g[c][k] out[c][k] in the order (mu, sigma, weights[0], ...,
// weights[C-1]); an operand that was not requested comes back undefined (None).  A broadcast
// operand gets the sum over objects.
std::vector<torch::Tensor> binned_multi_backward(torch::Tensor mu, torch::Tensor sigma,
                                                 Weights weights, std::vector<double> edges,
                                                 torch::Tensor g, bool need_mu, bool need_sigma,
                                                 std::vector<bool> need_w) {
  const MultiArgs base = make_multi_args(mu, sigma, weights, edges);
  TORCH_CHECK(base.n > 0, "binned_multi_backward: empty input");
  const int C = (int)weights.size();
  const int nb = base.nb;
  check_dev(g, "grad_out", at::kFloat);
  TORCH_CHECK(g.numel() == (int64_t)C * nb, "grad_out must have C * nb elements");
  TORCH_CHECK((int)need_w.size() == C, "need_w: one flag per channel");
  bool any_w = false;
  for (int c = 0; c < C; ++c) {
    const bool has = weights[c].has_value() && weights[c]->defined();
    TORCH_CHECK(!need_w[c] || has, "weights gradient requested for a channel without weights");
    any_w = any_w || need_w[c];
  }
  TORCH_CHECK(need_mu || need_sigma || any_w, "no gradient requested");
  const int nbp = padded_bins(nb, kOpMulti);
  std::vector<torch::Tensor> grads(2 + C);
  std::vector<float*> ptr(2 + C);
  grads[0] = alloc_grad(need_mu, base.n, mu, ptr[0]);
  grads[1] = alloc_grad(need_sigma, sigma.numel(), mu, ptr[1]);
  for (int c = 0; c < C; ++c)
    grads[2 + c] = alloc_grad(need_w[c], need_w[c] ? weights[c]->numel() : 0, mu, ptr[2 + c]);
  auto stream = at::hip::getCurrentHIPStream();
  for (int c0 = 0; c0 < C; c0 += kChanBlock) {
    const int nc = std::min(kChanBlock, C - c0);
    const MultiArgs a = with_channels(base, weights, c0, nc);
    MultiGrad o;
    o.g = g.data_ptr<float>() + (int64_t)c0 * nb;
    o.dmu = ptr[0];
    o.dsigma = ptr[1];
    o.slab = nullptr;
    o.accum = c0 > 0;  // with mu or sigma wanted, every earlier pass ran and stored
    // the [blocks, kRedCols] slab: sigma (added to an earlier pass's), four weights, unused
    ReduceBwd r = {};
    r.add0 = o.accum;
    r.out[0] = a.sig_b ? o.dsigma : nullptr;
    bool pass_w = false;
    for (int c = 0; c < kChanBlock; ++c) {
      o.dw[c] = c < nc ? ptr[2 + c0 + c] : nullptr;
      pass_w = pass_w || o.dw[c] != nullptr;
      r.out[1 + c] = (a.w_b >> c) & 1 ? o.dw[c] : nullptr;
    }
    if (!need_mu && !need_sigma && !pass_w) continue;
    MG_DISPATCH_MULTI(nbp, nc, {
      with_need3(need_mu, need_sigma, pass_w, [&](auto M, auto S, auto W) {
        launch_slab_bwd<binned_multi_bwd_kernel<NB, CB, decltype(M)::value, decltype(S)::value,
                                                decltype(W)::value>>(a, o, blocks_for(a.n),
                                                                     kRedCols, r, mu, stream);
      });
    });
  }
  return grads;
}

}  // namespace mg
