// Vector kernels of the device HMC sampler (optim/hmc.py; beyond the reference, which has
// no sampler).  A trajectory of L leapfrog steps is L + 1 launches of `hmc_leapfrog`
// around the L model evaluations: (eps/2, eps), L - 1 times (eps, eps), (eps/2, 0, ke).
//
//   hmc_leapfrog : p -= a g;  if b != 0: q += b inv_mass p (the new p);
//                  optionally ke = 1/2 sum p^2 inv_mass
//   hmc_momentum : p = z / sqrt(inv_mass);  ke = 1/2 sum z^2
//   hmc_commit   : Welford update of (mean, m2) with the host's count, the tracked
//                  parameters and a copy of q into a sample row -- one pass over q
//
// Vectors are fp32, energies fp64: the accept decision needs dH to far better than 1 while
// the kinetic energy is about n / 2 = 5e6 at 1e7 parameters, so every product and sum of an
// energy is formed in double from the fp32 values.  Reduction order is fixed (lane, wave
// shuffles, LDS, one slab row per workgroup, then `hmc_reduce_kernel`, as multi_dot in
// lbfgs.hip): no float atomics.  Every kernel walks the vector in chunks of 4 elements,
// chunk j to the same thread of the same grid whether the chunk is read as one float4 (all
// pointers 16-byte aligned) or as guarded scalars (any other view, and the last partial
// chunk), and the grid is the same for both, so the energies are bitwise equal on both
// load paths and from run to run for a fixed n and device.  The elementwise updates are
// written with explicit fmaf, the same on both paths.  The chunk load and store, the slab row
// and the grid are chunk_sweep.h's (shared with prior.hip); the final sum is sweep_device.h's
// slab entry sum and the cap over a kernel family sweep_host.h's.
//
// gfx950 (hipcc -O3), VGPRs per instantiation <VEC, BCAST>; no scratch, 8 waves per SIMD:
//   hmc_leapfrog_kernel  <1,0> 30  <1,1> 30  <0,0> 30  <0,1> 30
//   hmc_momentum_kernel  <1,0> 25  <1,1> 22  <0,0> 25  <0,1> 21
//   hmc_commit_kernel    <1> 33    <0> 30      hmc_reduce_kernel 18
#include "chunk_sweep.h"

#include <ATen/hip/HIPContext.h>

namespace mg {

template <bool VEC, bool BCAST>
__global__ __launch_bounds__(kHmcThreads) void hmc_leapfrog_kernel(
    float* __restrict__ q, float* __restrict__ p, const float* __restrict__ g,
    const float* __restrict__ inv_mass, float a, float b, int64_t n,
    double* __restrict__ partial) {
  const int64_t chunks = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * kHmcThreads;
  const float mb = BCAST ? inv_mass[0] : 0.0f;
  double acc = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * kHmcThreads + threadIdx.x; j < chunks; j += stride) {
    const int64_t off = j << 2;
    const int cnt = (int)min((int64_t)4, n - off);
    float pv[4], gv[4], mv[4], qv[4];
    load_chunk<VEC>(p, off, cnt, pv);
    load_chunk<VEC>(g, off, cnt, gv);
    if constexpr (BCAST) {
#pragma unroll
      for (int e = 0; e < 4; ++e) mv[e] = mb;
    } else {
      load_chunk<VEC>(inv_mass, off, cnt, mv);
    }
    if (b != 0.0f) load_chunk<VEC>(q, off, cnt, qv);
#pragma unroll
    for (int e = 0; e < 4; ++e) pv[e] = fmaf(-a, gv[e], pv[e]);
    store_chunk<VEC>(p, off, cnt, pv);
    if (b != 0.0f) {
#pragma unroll
      for (int e = 0; e < 4; ++e) qv[e] = fmaf(b * mv[e], pv[e], qv[e]);
      store_chunk<VEC>(q, off, cnt, qv);
    }
    if (partial != nullptr) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) acc = fma((double)pv[e] * (double)pv[e], (double)mv[e], acc);
    }
  }
  if (partial != nullptr) slab_row(acc, partial);
}

template <bool VEC, bool BCAST>
__global__ __launch_bounds__(kHmcThreads) void hmc_momentum_kernel(
    const float* __restrict__ z, const float* __restrict__ inv_mass, float* __restrict__ p,
    int64_t n, double* __restrict__ partial) {
  const int64_t chunks = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * kHmcThreads;
  const float mb = BCAST ? inv_mass[0] : 1.0f;
  double acc = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * kHmcThreads + threadIdx.x; j < chunks; j += stride) {
    const int64_t off = j << 2;
    const int cnt = (int)min((int64_t)4, n - off);
    float zv[4], mv[4], pv[4];
    load_chunk<VEC>(z, off, cnt, zv);
    if constexpr (BCAST) {
#pragma unroll
      for (int e = 0; e < 4; ++e) mv[e] = mb;
    } else {
      load_chunk<VEC>(inv_mass, off, cnt, mv);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) pv[e] = zv[e] / sqrtf(mv[e]);  // lanes past cnt are not stored
    store_chunk<VEC>(p, off, cnt, pv);
    if (partial != nullptr) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) acc = fma((double)zv[e], (double)zv[e], acc);
    }
  }
  if (partial != nullptr) slab_row(acc, partial);
}

// out[0] = 1/2 sum of the slab rows: each thread a fixed strided subset, then the fixed
// shuffle/LDS tree (one workgroup).
__global__ __launch_bounds__(kHmcThreads) void hmc_reduce_kernel(
    const double* __restrict__ partial, int nblk, double* __restrict__ out) {
  const double s = slab_entry_sum<kHmcThreads>(nblk, [&](int b) { return partial[b]; });
  if (threadIdx.x == 0) out[0] = 0.5 * s;
}

// Welford with the count that includes this vector (rc = 1 / count):
//   d = q - mean;  mean += d rc;  m2 += d (q - mean).
template <bool VEC>
__global__ __launch_bounds__(kHmcThreads) void hmc_commit_kernel(
    const float* __restrict__ q, int64_t n, float rc, float* __restrict__ mean,
    float* __restrict__ m2, const int64_t* __restrict__ track_idx, int64_t ntrack,
    float* __restrict__ track_row, float* __restrict__ sample_row) {
  const int64_t chunks = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * kHmcThreads;
  const int64_t tid = (int64_t)blockIdx.x * kHmcThreads + threadIdx.x;
  if (mean != nullptr || sample_row != nullptr) {
    for (int64_t j = tid; j < chunks; j += stride) {
      const int64_t off = j << 2;
      const int cnt = (int)min((int64_t)4, n - off);
      float qv[4];
      load_chunk<VEC>(q, off, cnt, qv);
      if (mean != nullptr) {
        float av[4], sv[4];
        load_chunk<VEC>(mean, off, cnt, av);
        load_chunk<VEC>(m2, off, cnt, sv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = qv[e] - av[e];
          av[e] = fmaf(d, rc, av[e]);
          sv[e] = fmaf(d, qv[e] - av[e], sv[e]);
        }
        store_chunk<VEC>(mean, off, cnt, av);
        store_chunk<VEC>(m2, off, cnt, sv);
      }
      if (sample_row != nullptr) store_chunk<VEC>(sample_row, off, cnt, qv);
    }
  }
  for (int64_t j = tid; j < ntrack; j += stride) {
    const int64_t i = track_idx[j];
    if (i >= 0 && i < n) track_row[j] = q[i];  // an index outside q is never read
  }
}

// inv_mass: n elements, or 1 (broadcast)
static bool check_mass(const torch::Tensor& m, int64_t n) {
  TORCH_CHECK(m.is_cuda() && m.scalar_type() == at::kFloat && m.is_contiguous() &&
              (m.numel() == n || m.numel() == 1), "inv_mass: fp32 device, n elements or 1");
  return m.numel() == 1 && n != 1;
}

static double* energy_ptrs(const c10::optional<torch::Tensor>& ke_out,
                           const c10::optional<torch::Tensor>& ws, double** out) {
  *out = nullptr;
  if (!ke_out.has_value() || !ke_out->defined()) return nullptr;
  TORCH_CHECK(ws.has_value() && ws->defined(), "ke_out needs the workspace");
  TORCH_CHECK(ke_out->is_cuda() && ke_out->scalar_type() == at::kDouble && ke_out->numel() >= 1 &&
              ws->is_cuda() && ws->scalar_type() == at::kDouble && ws->is_contiguous() &&
              ws->numel() >= kHmcMaxBlocks, "ke_out: fp64 device; workspace: hmc_workspace() fp64");
  *out = ke_out->data_ptr<double>();
  return ws->data_ptr<double>();
}

int64_t hmc_workspace() { return kHmcMaxBlocks; }

void hmc_leapfrog(torch::Tensor q, torch::Tensor p, torch::Tensor g, torch::Tensor inv_mass,
                  double a, double b, c10::optional<torch::Tensor> ke_out,
                  c10::optional<torch::Tensor> ws) {
  const int64_t n = q.numel();
  check_vec(q, n, "q");
  check_vec(p, n, "p");
  check_vec(g, n, "g");
  const bool bcast = check_mass(inv_mass, n);
  double* out = nullptr;
  double* partial = energy_ptrs(ke_out, ws, &out);
  if (n == 0) {
    if (out != nullptr) ke_out->zero_();
    return;
  }
  float* qp = q.data_ptr<float>();
  float* pp = p.data_ptr<float>();
  const float* gp = g.data_ptr<float>();
  const float* mp = inv_mass.data_ptr<float>();
  TORCH_CHECK(qp != pp && qp != gp && pp != gp, "q, p and g must be distinct vectors");
  const bool vec = aligned16(qp) && aligned16(pp) && aligned16(gp) &&
                   (bcast || aligned16(mp));
  static GridCap cap;
  const int blocks = hmc_grid(n, cap, hmc_leapfrog_kernel<true, false>,
                              hmc_leapfrog_kernel<true, true>, hmc_leapfrog_kernel<false, false>,
                              hmc_leapfrog_kernel<false, true>);
  auto stream = at::hip::getCurrentHIPStream();
  const float af = (float)a, bf = (float)b;
  auto go = [&](auto k) {
    hipLaunchKernelGGL(k, dim3(blocks), dim3(kHmcThreads), 0, stream, qp, pp, gp, mp, af, bf, n,
                       partial);
  };
  if (vec) {
    if (bcast) go(hmc_leapfrog_kernel<true, true>); else go(hmc_leapfrog_kernel<true, false>);
  } else {
    if (bcast) go(hmc_leapfrog_kernel<false, true>); else go(hmc_leapfrog_kernel<false, false>);
  }
  if (partial != nullptr)
    hipLaunchKernelGGL(hmc_reduce_kernel, dim3(1), dim3(kHmcThreads), 0, stream, partial, blocks,
                       out);
}

void hmc_momentum(torch::Tensor z, torch::Tensor inv_mass, torch::Tensor p,
                  c10::optional<torch::Tensor> ke_out, c10::optional<torch::Tensor> ws) {
  const int64_t n = z.numel();
  check_vec(z, n, "z");
  check_vec(p, n, "p");
  const bool bcast = check_mass(inv_mass, n);
  double* out = nullptr;
  double* partial = energy_ptrs(ke_out, ws, &out);
  if (n == 0) {
    if (out != nullptr) ke_out->zero_();
    return;
  }
  const float* zp = z.data_ptr<float>();
  float* pp = p.data_ptr<float>();
  const float* mp = inv_mass.data_ptr<float>();
  TORCH_CHECK(zp != pp, "z and p must be distinct vectors");
  const bool vec = aligned16(zp) && aligned16(pp) && (bcast || aligned16(mp));
  static GridCap cap;
  const int blocks = hmc_grid(n, cap, hmc_momentum_kernel<true, false>,
                              hmc_momentum_kernel<true, true>, hmc_momentum_kernel<false, false>,
                              hmc_momentum_kernel<false, true>);
  auto stream = at::hip::getCurrentHIPStream();
  auto go = [&](auto k) {
    hipLaunchKernelGGL(k, dim3(blocks), dim3(kHmcThreads), 0, stream, zp, mp, pp, n, partial);
  };
  if (vec) {
    if (bcast) go(hmc_momentum_kernel<true, true>); else go(hmc_momentum_kernel<true, false>);
  } else {
    if (bcast) go(hmc_momentum_kernel<false, true>); else go(hmc_momentum_kernel<false, false>);
  }
  if (partial != nullptr)
    hipLaunchKernelGGL(hmc_reduce_kernel, dim3(1), dim3(kHmcThreads), 0, stream, partial, blocks,
                       out);
}

void hmc_commit(torch::Tensor q, int64_t count, c10::optional<torch::Tensor> mean,
                c10::optional<torch::Tensor> m2, c10::optional<torch::Tensor> track_idx,
                c10::optional<torch::Tensor> track_row, c10::optional<torch::Tensor> sample_row) {
  const int64_t n = q.numel();
  check_vec(q, n, "q");
  const float* qp = q.data_ptr<float>();
  bool vec = aligned16(qp);
  float *ap = nullptr, *sp = nullptr, *tp = nullptr, *rp = nullptr;
  const int64_t* ip = nullptr;
  int64_t ntrack = 0;
  if (has(mean)) {
    TORCH_CHECK(has(m2) && count >= 1, "mean needs m2 and a count >= 1");
    check_vec(*mean, n, "mean");
    check_vec(*m2, n, "m2");
    ap = mean->data_ptr<float>();
    sp = m2->data_ptr<float>();
    TORCH_CHECK(ap != sp && ap != qp && sp != qp, "q, mean and m2 must be distinct vectors");
    vec = vec && aligned16(ap) && aligned16(sp);
  }
  if (has(track_idx)) {
    TORCH_CHECK(has(track_row), "track_idx needs track_row");
    ntrack = track_idx->numel();
    TORCH_CHECK(track_idx->is_cuda() && track_idx->scalar_type() == at::kLong &&
                track_idx->is_contiguous(), "track_idx: contiguous int64 device vector");
    check_vec(*track_row, ntrack, "track_row");
    ip = track_idx->data_ptr<int64_t>();
    tp = track_row->data_ptr<float>();
  }
  if (has(sample_row)) {
    check_vec(*sample_row, n, "sample_row");
    rp = sample_row->data_ptr<float>();
    TORCH_CHECK(rp != qp, "sample_row must not be q");
    vec = vec && aligned16(rp);
  }
  const bool pass = (ap != nullptr || rp != nullptr) && n > 0;
  if (!pass && ntrack == 0) return;
  static GridCap cap;
  auto grid = [&](int64_t len) {
    return hmc_grid(len, cap, hmc_commit_kernel<true>, hmc_commit_kernel<false>);
  };
  const int blocks = std::max(pass ? grid(n) : 1, grid(4 * ntrack));
  const float rc = (float)(1.0 / (double)std::max<int64_t>(count, 1));
  auto stream = at::hip::getCurrentHIPStream();
  if (vec)
    hipLaunchKernelGGL(hmc_commit_kernel<true>, dim3(blocks), dim3(kHmcThreads), 0, stream, qp, n,
                       rc, ap, sp, ip, ntrack, tp, rp);
  else
    hipLaunchKernelGGL(hmc_commit_kernel<false>, dim3(blocks), dim3(kHmcThreads), 0, stream, qp,
                       n, rc, ap, sp, ip, ntrack, tp, rp);
}

}  // namespace mg
