// Vector kernels of the Gaussian parameter prior (optim/prior.py; beyond the reference, which
// has neither a prior nor a sampler): pen(x) = 1/2 sum w (x - m)^2 with a mean m and an
// inverse variance w per parameter, each of n elements or both of one (broadcast).
//
//   gaussian_prior_grad  : out = g + c w (x - m)  (out may be g);
//                          optionally pen = 1/2 sum w (x - m)^2
//   hmc_leapfrog_prior   : hmc.hip's leapfrog with the prior's force taken from the position
//                          it reads:  s = p - a g;  p = s - ap w (q - m);
//                          if b != 0: q += b inv_mass p (the new p);  optionally
//                          ke = 1/2 sum p^2 inv_mass and pen = 1/2 sum w (q_in - m)^2
//
// Both are one streaming pass built as hmc.hip's: chunks of 4 elements, chunk j to the same
// thread of the same grid on the float4 and on the guarded-scalar path (chunk_sweep.h), one
// grid cap per kernel family, explicit fmaf for the fp32 updates, and energies whose
// products and sums are formed in double from the fp32 values (the difference x - m of a
// penalty too) in a fixed order -- lane, wave shuffles, LDS, one slab row per workgroup and
// energy, then one one-workgroup `prior_reduce_kernel` for both energies: no float atomics,
// bitwise equal on both load paths and from run to run.  With w = 0 the leapfrog's vectors
// and kinetic energy are those of hmc_leapfrog_kernel: fmaf(-0, d, s) = s, and the slab sums
// run in the same order on the same grid while both grids are below their caps.  Against the
// flat leapfrog the pass reads 8 more bytes per element for a per-element prior (and q in
// the closing half step, which the flat kernel skips), none for a broadcast one.
//
// gfx950 (hipcc -O3), VGPRs per instantiation; no scratch, 32 bytes of LDS, 8 waves per SIMD
// in every one (the occupancy of hmc.hip's kernels, so the same grid cap):
//   hmc_leapfrog_prior_kernel <VEC, BCAST (inv_mass), PB (prior)>
//     <1,0,0> 46  <1,0,1> 42  <1,1,0> 46  <1,1,1> 42
//     <0,0,0> 46  <0,0,1> 40  <0,1,0> 44  <0,1,1> 40
//   gaussian_prior_grad_kernel <VEC, PB>  <1,0> 30  <1,1> 26  <0,0> 29  <0,1> 25
//   prior_reduce_kernel 20 (64 bytes of LDS)
#include "chunk_sweep.h"

#include <ATen/hip/HIPContext.h>

namespace mg {

template <bool VEC, bool PB>
__device__ __forceinline__ void load_prior(const float* __restrict__ mean,
                                           const float* __restrict__ inv_var, float m0, float w0,
                                           int64_t off, int cnt, float (&mv)[4], float (&wv)[4]) {
  if constexpr (PB) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      mv[e] = m0;
      wv[e] = w0;
    }
  } else {
    load_chunk<VEC>(mean, off, cnt, mv);
    load_chunk<VEC>(inv_var, off, cnt, wv);
  }
}

// acc += w (x - m)^2 over the chunk's cnt elements, in double from the fp32 values
__device__ __forceinline__ double penalty_chunk(const float (&xv)[4], const float (&mv)[4],
                                                const float (&wv)[4], int cnt, double acc) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < cnt) {
      const double d = (double)xv[e] - (double)mv[e];
      acc = fma(d * d, (double)wv[e], acc);
    }
  return acc;
}

// g and out carry no __restrict__: out may be g (every chunk is read before it is written,
// by the one thread that owns it).
template <bool VEC, bool PB>
__global__ __launch_bounds__(kHmcThreads) void gaussian_prior_grad_kernel(
    const float* __restrict__ x, const float* g, const float* __restrict__ mean,
    const float* __restrict__ inv_var, float c, float* out, int64_t n,
    double* __restrict__ partial) {
  const int64_t chunks = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * kHmcThreads;
  const float m0 = PB ? mean[0] : 0.0f;
  const float w0 = PB ? inv_var[0] : 0.0f;
  double acc = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * kHmcThreads + threadIdx.x; j < chunks; j += stride) {
    const int64_t off = j << 2;
    const int cnt = (int)min((int64_t)4, n - off);
    float xv[4], gv[4], mv[4], wv[4];
    load_chunk<VEC>(x, off, cnt, xv);
    load_chunk<VEC>(g, off, cnt, gv);
    load_prior<VEC, PB>(mean, inv_var, m0, w0, off, cnt, mv, wv);
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[e] = fmaf(c * wv[e], xv[e] - mv[e], gv[e]);
    store_chunk<VEC>(out, off, cnt, gv);
    if (partial != nullptr) acc = penalty_chunk(xv, mv, wv, cnt, acc);
  }
  if (partial != nullptr) slab_row(acc, partial);
}

template <bool VEC, bool BCAST, bool PB>
__global__ __launch_bounds__(kHmcThreads) void hmc_leapfrog_prior_kernel(
    float* __restrict__ q, float* __restrict__ p, const float* __restrict__ g,
    const float* __restrict__ inv_mass, float a, float b, const float* __restrict__ mean,
    const float* __restrict__ inv_var, float ap, int64_t n, double* __restrict__ ke_partial,
    double* __restrict__ pen_partial) {
  const int64_t chunks = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * kHmcThreads;
  const float mb = BCAST ? inv_mass[0] : 0.0f;
  const float m0 = PB ? mean[0] : 0.0f;
  const float w0 = PB ? inv_var[0] : 0.0f;
  double acc = 0.0, pacc = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * kHmcThreads + threadIdx.x; j < chunks; j += stride) {
    const int64_t off = j << 2;
    const int cnt = (int)min((int64_t)4, n - off);
    float pv[4], gv[4], imv[4], qv[4], mv[4], wv[4];
    load_chunk<VEC>(p, off, cnt, pv);
    load_chunk<VEC>(g, off, cnt, gv);
    load_chunk<VEC>(q, off, cnt, qv);
    if constexpr (BCAST) {
#pragma unroll
      for (int e = 0; e < 4; ++e) imv[e] = mb;
    } else {
      load_chunk<VEC>(inv_mass, off, cnt, imv);
    }
    load_prior<VEC, PB>(mean, inv_var, m0, w0, off, cnt, mv, wv);
    if (pen_partial != nullptr) pacc = penalty_chunk(qv, mv, wv, cnt, pacc);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      pv[e] = fmaf(-(ap * wv[e]), qv[e] - mv[e], fmaf(-a, gv[e], pv[e]));
    store_chunk<VEC>(p, off, cnt, pv);
    if (b != 0.0f) {
#pragma unroll
      for (int e = 0; e < 4; ++e) qv[e] = fmaf(b * imv[e], pv[e], qv[e]);
      store_chunk<VEC>(q, off, cnt, qv);
    }
    if (ke_partial != nullptr) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) acc = fma((double)pv[e] * (double)pv[e], (double)imv[e], acc);
    }
  }
  // the two slab rows go through the one LDS array of slab_row
  if (ke_partial != nullptr) slab_row(acc, ke_partial);
  if (ke_partial != nullptr && pen_partial != nullptr) __syncthreads();
  if (pen_partial != nullptr) slab_row(pacc, pen_partial);
}

// out_k[0] = 1/2 sum of the rows of slab k, for each slab given: each thread a fixed strided
// subset, then the fixed shuffle/LDS tree, as hmc_reduce_kernel (one workgroup).
__global__ __launch_bounds__(kHmcThreads) void prior_reduce_kernel(
    const double* __restrict__ ke_partial, double* __restrict__ ke_out,
    const double* __restrict__ pen_partial, double* __restrict__ pen_out, int nblk) {
  if (ke_partial != nullptr) {
    const double s = slab_entry_sum<kHmcThreads>(nblk, [&](int b) { return ke_partial[b]; });
    if (threadIdx.x == 0) ke_out[0] = 0.5 * s;
  }
  if (ke_partial != nullptr && pen_partial != nullptr) __syncthreads();
  if (pen_partial != nullptr) {
    const double s = slab_entry_sum<kHmcThreads>(nblk, [&](int b) { return pen_partial[b]; });
    if (threadIdx.x == 0) pen_out[0] = 0.5 * s;
  }
}

// mean and inv_var: both n elements, or both 1 (broadcast)
static bool check_prior(const torch::Tensor& mean, const torch::Tensor& inv_var, int64_t n) {
  for (const torch::Tensor* t : {&mean, &inv_var})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() &&
                (t->numel() == n || t->numel() == 1), "mean, inv_var: fp32 device, n elements or 1");
  TORCH_CHECK(mean.numel() == inv_var.numel(), "mean and inv_var must have the same length");
  return mean.numel() == 1 && n != 1;
}

// An energy's output and its slab (row `slot` of the workspace), or nullptr without one.
static double* energy_slab(const c10::optional<torch::Tensor>& e_out,
                           const c10::optional<torch::Tensor>& ws, int slot, double** out) {
  *out = nullptr;
  if (!has(e_out)) return nullptr;
  TORCH_CHECK(has(ws), "an energy output needs the workspace");
  TORCH_CHECK(e_out->is_cuda() && e_out->scalar_type() == at::kDouble && e_out->numel() >= 1 &&
              ws->is_cuda() && ws->scalar_type() == at::kDouble && ws->is_contiguous() &&
              ws->numel() >= 2 * kHmcMaxBlocks,
              "energy output: fp64 device; workspace: prior_workspace() fp64");
  *out = e_out->data_ptr<double>();
  return ws->data_ptr<double>() + (int64_t)slot * kHmcMaxBlocks;
}

int64_t prior_workspace() { return 2 * kHmcMaxBlocks; }

void gaussian_prior_grad(torch::Tensor x, torch::Tensor g, torch::Tensor mean,
                         torch::Tensor inv_var, double c, torch::Tensor out,
                         c10::optional<torch::Tensor> pen_out, c10::optional<torch::Tensor> ws) {
  const int64_t n = x.numel();
  check_vec(x, n, "x");
  check_vec(g, n, "g");
  check_vec(out, n, "out");
  const bool pb = check_prior(mean, inv_var, n);
  double* pout = nullptr;
  double* partial = energy_slab(pen_out, ws, 1, &pout);
  if (n == 0) {
    if (pout != nullptr) pen_out->zero_();
    return;
  }
  const float* xp = x.data_ptr<float>();
  const float* gp = g.data_ptr<float>();
  const float* mp = mean.data_ptr<float>();
  const float* wp = inv_var.data_ptr<float>();
  float* op = out.data_ptr<float>();
  TORCH_CHECK(op != xp && op != mp && op != wp, "out must not be x, mean or inv_var");
  const bool vec = aligned16(xp) && aligned16(gp) && aligned16(op) &&
                   (pb || (aligned16(mp) && aligned16(wp)));
  static GridCap cap;
  const int blocks = hmc_grid(n, cap, gaussian_prior_grad_kernel<true, false>,
                              gaussian_prior_grad_kernel<true, true>,
                              gaussian_prior_grad_kernel<false, false>,
                              gaussian_prior_grad_kernel<false, true>);
  auto stream = at::hip::getCurrentHIPStream();
  const float cf = (float)c;
  auto go = [&](auto k) {
    hipLaunchKernelGGL(k, dim3(blocks), dim3(kHmcThreads), 0, stream, xp, gp, mp, wp, cf, op, n,
                       partial);
  };
  if (vec) {
    if (pb) go(gaussian_prior_grad_kernel<true, true>);
    else go(gaussian_prior_grad_kernel<true, false>);
  } else {
    if (pb) go(gaussian_prior_grad_kernel<false, true>);
    else go(gaussian_prior_grad_kernel<false, false>);
  }
  if (partial != nullptr)
    hipLaunchKernelGGL(prior_reduce_kernel, dim3(1), dim3(kHmcThreads), 0, stream,
                       (const double*)nullptr, (double*)nullptr, (const double*)partial, pout,
                       blocks);
}

void hmc_leapfrog_prior(torch::Tensor q, torch::Tensor p, torch::Tensor g, torch::Tensor inv_mass,
                        double a, double b, torch::Tensor mean, torch::Tensor inv_var, double ap,
                        c10::optional<torch::Tensor> ke_out, c10::optional<torch::Tensor> pen_out,
                        c10::optional<torch::Tensor> ws) {
  const int64_t n = q.numel();
  check_vec(q, n, "q");
  check_vec(p, n, "p");
  check_vec(g, n, "g");
  TORCH_CHECK(inv_mass.is_cuda() && inv_mass.scalar_type() == at::kFloat &&
              inv_mass.is_contiguous() && (inv_mass.numel() == n || inv_mass.numel() == 1),
              "inv_mass: fp32 device, n elements or 1");
  const bool bcast = inv_mass.numel() == 1 && n != 1;
  const bool pb = check_prior(mean, inv_var, n);
  double *kout = nullptr, *pout = nullptr;
  double* kpart = energy_slab(ke_out, ws, 0, &kout);
  double* ppart = energy_slab(pen_out, ws, 1, &pout);
  if (n == 0) {
    if (kout != nullptr) ke_out->zero_();
    if (pout != nullptr) pen_out->zero_();
    return;
  }
  float* qp = q.data_ptr<float>();
  float* pp = p.data_ptr<float>();
  const float* gp = g.data_ptr<float>();
  const float* imp = inv_mass.data_ptr<float>();
  const float* mp = mean.data_ptr<float>();
  const float* wp = inv_var.data_ptr<float>();
  TORCH_CHECK(qp != pp && qp != gp && pp != gp, "q, p and g must be distinct vectors");
  for (const float* r : {imp, mp, wp})
    TORCH_CHECK(r != qp && r != pp, "inv_mass, mean and inv_var must not be q or p");
  const bool vec = aligned16(qp) && aligned16(pp) && aligned16(gp) &&
                   (bcast || aligned16(imp)) && (pb || (aligned16(mp) && aligned16(wp)));
  static GridCap cap;
  const int blocks = hmc_grid(
      n, cap, hmc_leapfrog_prior_kernel<true, false, false>,
      hmc_leapfrog_prior_kernel<true, false, true>, hmc_leapfrog_prior_kernel<true, true, false>,
      hmc_leapfrog_prior_kernel<true, true, true>, hmc_leapfrog_prior_kernel<false, false, false>,
      hmc_leapfrog_prior_kernel<false, false, true>, hmc_leapfrog_prior_kernel<false, true, false>,
      hmc_leapfrog_prior_kernel<false, true, true>);
  auto stream = at::hip::getCurrentHIPStream();
  const float af = (float)a, bf = (float)b, apf = (float)ap;
  auto go = [&](auto k) {
    hipLaunchKernelGGL(k, dim3(blocks), dim3(kHmcThreads), 0, stream, qp, pp, gp, imp, af, bf, mp,
                       wp, apf, n, kpart, ppart);
  };
  auto pick = [&](auto v, auto bc) {
    if (pb) go(hmc_leapfrog_prior_kernel<decltype(v)::value, decltype(bc)::value, true>);
    else go(hmc_leapfrog_prior_kernel<decltype(v)::value, decltype(bc)::value, false>);
  };
  if (vec) {
    if (bcast) pick(std::true_type{}, std::true_type{});
    else pick(std::true_type{}, std::false_type{});
  } else {
    if (bcast) pick(std::false_type{}, std::true_type{});
    else pick(std::false_type{}, std::false_type{});
  }
  if (kpart != nullptr || ppart != nullptr)
    hipLaunchKernelGGL(prior_reduce_kernel, dim3(1), dim3(kHmcThreads), 0, stream,
                       (const double*)kpart, kout, (const double*)ppart, pout, blocks);
}

}  // namespace mg
