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

#include "binned_common.h"
#include "smf_host.h"

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

// Fixed-order sum of the forward slab [rows, ld]: workgroup c sums the nbp columns of channel
// c (slab_column_sum) and writes its real bins to out[c][0..nb).
__global__ __launch_bounds__(kRedThreads) void binned_multi_reduce_fwd_kernel(
    const float* slab, int64_t rows, int ld, int nbp, int nb, float* out) {
  __shared__ float part[kRedThreads];
  float t;
  if (slab_column_sum(slab, rows, ld, blockIdx.x * nbp, nbp, part, t)) {
    const int k = threadIdx.x;
    if (k < nb) out[blockIdx.x * nb + k] = t;
  }
}

// The [blocks, kRedCols] slab of broadcast gradients: column k goes to out[k] (null: dropped);
// with `add0`, column 0 (sigma) is added to what an earlier pass left there.
struct MultiRed {
  float* out[kRedCols];
  int add0;
};

__global__ __launch_bounds__(kRedThreads) void binned_multi_reduce_bwd_kernel(const float* slab,
                                                                              int64_t rows,
                                                                              MultiRed r) {
  __shared__ float part[kRedThreads];
  float t;
  if (slab_column_sum(slab, rows, kRedCols, 0, kRedCols, part, t)) {
#pragma unroll
    for (int k = 0; k < kRedCols; ++k) {
      if ((int)threadIdx.x == k && r.out[k] != nullptr)
        r.out[k][0] = k == 0 && r.add0 ? r.out[k][0] + t : t;
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

int multi_padded(int nb) {
  TORCH_CHECK(nb >= 1 && nb <= kMaxBins, "gaussian_binned_sum_multi: 1 <= nb <= ", kMaxBins,
              ", got ", nb);
  return nb <= 4 ? 4 : nb <= 8 ? 8 : nb <= 16 ? 16 : 32;
}

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

// Workgroups that fill the chip once (occupancy x CU count of the device), per kernel.
template <auto Kernel>
int64_t chip_blocks_multi() {
  static int64_t cap = resident_blocks(reinterpret_cast<const void*>(Kernel), kBinThreads);
  return cap;
}

using Weights = std::vector<c10::optional<torch::Tensor>>;

// The operands shared by every pass; the channels are filled in by set_channels.
MultiArgs make_multi_args(const torch::Tensor& mu, const torch::Tensor& sigma,
                          const Weights& w, const std::vector<double>& edges) {
  check_dev(mu, "mu", at::kFloat);
  check_dev(sigma, "sigma", at::kFloat);
  const int64_t C = (int64_t)w.size();
  TORCH_CHECK(C >= 1 && C <= kMaxChannels, "gaussian_binned_sum_multi: 1 <= C <= ", kMaxChannels,
              " weight channels, got ", C);
  MultiArgs a;
  a.n = mu.numel();
  a.nb = (int)edges.size() - 1;
  multi_padded(a.nb);
  for (int e = 1; e <= a.nb; ++e)
    TORCH_CHECK(edges[e] > edges[e - 1],
                "gaussian_binned_sum_multi: edges must be strictly increasing");
  for (int e = 0; e <= kMaxBins; ++e) a.edge[e] = (float)edges[std::min(e, a.nb)];
  TORCH_CHECK(sigma.numel() == a.n || sigma.numel() == 1, "sigma must have N elements or one");
  a.mu = mu.data_ptr<float>();
  a.sigma = sigma.data_ptr<float>();
  a.sig_b = sigma.numel() == 1 && a.n != 1;
  for (const auto& t : w) {
    if (t.has_value() && t->defined()) {
      check_dev(*t, "weights", at::kFloat);
      TORCH_CHECK(t->numel() == a.n || t->numel() == 1,
                  "every weights entry must have N elements or one");
    }
  }
  return a;
}

// Channels [c0, c0 + nc) of `w` into the pass arguments.
void set_channels(MultiArgs& a, const Weights& w, int c0, int nc) {
  a.nc = nc;
  a.w_b = 0;
  bool vec = aligned_to(a.mu, 16) && (a.sig_b || aligned_to(a.sigma, 16));
  for (int c = 0; c < kChanBlock; ++c) {
    a.w[c] = nullptr;
    if (c >= nc) continue;
    const auto& t = w[c0 + c];
    if (!t.has_value() || !t->defined()) continue;
    a.w[c] = t->data_ptr<float>();
    if (t->numel() == 1 && a.n != 1) a.w_b |= 1 << c;
    else vec = vec && aligned_to(a.w[c], 16);
  }
  a.vec = vec;
}

template <auto Kernel>
void launch_multi_bwd(const MultiArgs& a, MultiGrad& o, const torch::Tensor& like, bool red_sig,
                      hipStream_t stream) {
  const int64_t need = ((a.n + 3) / 4 + kBinThreads - 1) / kBinThreads;
  const int64_t blocks = std::min(need, chip_blocks_multi<Kernel>());
  MultiRed r;
  r.add0 = o.accum;
  bool any = red_sig;
  r.out[0] = red_sig ? o.dsigma : nullptr;
  for (int k = 1; k < kRedCols; ++k) {
    const int c = k - 1;
    r.out[k] = c < kChanBlock && ((a.w_b >> c) & 1) ? o.dw[c] : nullptr;
    any = any || r.out[k] != nullptr;
  }
  const bool two = any && blocks > 1;
  torch::Tensor slab;
  if (two) {
    slab = torch::empty({blocks, (int64_t)kRedCols}, like.options());
    o.slab = slab.data_ptr<float>();
  }
  hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(kBinThreads), 0, stream, a, o, blocks == 1 ? 1 : 0);
  if (two)
    hipLaunchKernelGGL(binned_multi_reduce_bwd_kernel, dim3(1), dim3(kRedThreads), 0, stream,
                       (const float*)o.slab, blocks, r);
}

}  // namespace

// out[C, nb]; weights[c] undefined / None stands for the constant 1.
torch::Tensor binned_multi_forward(torch::Tensor mu, torch::Tensor sigma, Weights weights,
                                   std::vector<double> edges) {
  MultiArgs a = make_multi_args(mu, sigma, weights, edges);
  TORCH_CHECK(a.n > 0, "binned_multi_forward: empty input");
  const int C = (int)weights.size();
  const int nbp = multi_padded(a.nb);
  auto out = torch::empty({(int64_t)C, (int64_t)a.nb}, mu.options());
  auto stream = at::hip::getCurrentHIPStream();
  const int64_t need = ((a.n + 3) / 4 + kBinThreads - 1) / kBinThreads;
  for (int c0 = 0; c0 < C; c0 += kChanBlock) {
    const int nc = std::min(kChanBlock, C - c0);
    set_channels(a, weights, c0, nc);
    float* dst = out.data_ptr<float>() + (int64_t)c0 * a.nb;
    MG_DISPATCH_MULTI(nbp, nc, {
      const int64_t blocks =
          std::min(need, chip_blocks_multi<binned_multi_fwd_kernel<NB, CB>>());
      if (blocks == 1) {
        hipLaunchKernelGGL((binned_multi_fwd_kernel<NB, CB>), dim3(1), dim3(kBinThreads), 0,
                           stream, a, (float*)nullptr, dst, 1);
      } else {
        auto slab = torch::empty({blocks, (int64_t)(CB * NB)}, mu.options());
        hipLaunchKernelGGL((binned_multi_fwd_kernel<NB, CB>), dim3(blocks), dim3(kBinThreads), 0,
                           stream, a, slab.data_ptr<float>(), (float*)nullptr, 0);
        hipLaunchKernelGGL(binned_multi_reduce_fwd_kernel, dim3(nc), dim3(kRedThreads), 0, stream,
                           (const float*)slab.data_ptr<float>(), blocks, CB * NB, NB, a.nb, dst);
      }
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
  MultiArgs a = make_multi_args(mu, sigma, weights, edges);
  TORCH_CHECK(a.n > 0, "binned_multi_backward: empty input");
  const int C = (int)weights.size();
  check_dev(g, "grad_out", at::kFloat);
  TORCH_CHECK(g.numel() == (int64_t)C * a.nb, "grad_out must have C * nb elements");
  TORCH_CHECK((int)need_w.size() == C, "need_w: one flag per channel");
  bool any_w = false;
  for (int c = 0; c < C; ++c) {
    const bool has = weights[c].has_value() && weights[c]->defined();
    TORCH_CHECK(!need_w[c] || has, "weights gradient requested for a channel without weights");
    any_w = any_w || need_w[c];
  }
  TORCH_CHECK(need_mu || need_sigma || any_w, "no gradient requested");
  const int nbp = multi_padded(a.nb);
  std::vector<torch::Tensor> grads(2 + C);
  if (need_mu) grads[0] = torch::empty({a.n}, mu.options());
  if (need_sigma) grads[1] = torch::empty({sigma.numel()}, mu.options());
  for (int c = 0; c < C; ++c)
    if (need_w[c]) grads[2 + c] = torch::empty({weights[c]->numel()}, mu.options());
  auto stream = at::hip::getCurrentHIPStream();
  for (int c0 = 0; c0 < C; c0 += kChanBlock) {
    const int nc = std::min(kChanBlock, C - c0);
    set_channels(a, weights, c0, nc);
    MultiGrad o;
    o.g = g.data_ptr<float>() + (int64_t)c0 * a.nb;
    o.dmu = need_mu ? grads[0].data_ptr<float>() : nullptr;
    o.dsigma = need_sigma ? grads[1].data_ptr<float>() : nullptr;
    o.slab = nullptr;
    o.accum = c0 > 0;  // with mu or sigma wanted, every earlier pass ran and stored
    bool pass_w = false;
    for (int c = 0; c < kChanBlock; ++c) {
      o.dw[c] = c < nc && need_w[c0 + c] ? grads[2 + c0 + c].data_ptr<float>() : nullptr;
      pass_w = pass_w || o.dw[c] != nullptr;
    }
    if (!need_mu && !need_sigma && !pass_w) continue;
    const bool red_sig = need_sigma && a.sig_b;
    MG_DISPATCH_MULTI(nbp, nc, {
      with_bool(need_mu, [&](auto M) {
        with_bool(need_sigma, [&](auto S) {
          with_bool(pass_w, [&](auto W) {
            constexpr bool kM = decltype(M)::value, kS = decltype(S)::value, kW = decltype(W)::value;
            if constexpr (kM || kS || kW)
              launch_multi_bwd<binned_multi_bwd_kernel<NB, CB, kM, kS, kW>>(a, o, mu, red_sig,
                                                                            stream);
          });
        });
      });
    });
  }
  return grads;
}

}  // namespace mg
