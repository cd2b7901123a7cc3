// One-pass sumstat Jacobian of the population SMF over the lanes layout's residuals.
//
// The residual forward (smf_lanes.hip) leaves, per population slot, the per-edge sums
// G_e = sum_i exp2(-w_ie^2) and W_e = sum_i exp2(-w_ie^2) w_ie, and the residual VJP
// contracts them with the edge weights h of ONE cotangent.  Every row of the Jacobian
// J[k] = dS_k / dtheta is that VJP for the unit cotangent e_k, whose edge weights are
// h_k = -scale_k / sqrt(2 pi), h_{k+1} = +scale_k / sqrt(2 pi) (smf_edge_weights), so
//
//     A_k = (scale_k / sqrt(2 pi)) (G_{k+1} - G_k),   B_k = (scale_k / sqrt(2 pi)) (W_{k+1} - W_k)
//
// and J[k][c] = pop_grad(theta_c, A_k, B_k): all nb rows are linear in the same 2 (NB + 1)
// residuals.  This kernel reads the residuals once and writes the nb rows, where nb
// launches of smf_vjp_lanes_kernel read them nb times.  Same persistent, XCD-sliced walk
// over the 64-slot groups with the next group's residuals in flight.  Split populations
// write their nb (A_k, B_k) pairs to partials [nparts, nb]; smf_jac_finalize_kernel sums a
// population's parts in a fixed order and applies pop_grad (the shape of
// smf_vjp_finalize_kernel).
#include "smf_device.h"
#include "smf_host.h"

namespace mg {

struct JacCoef {
  float c[kMaxBins];  // scale_k / sqrt(2 pi), zero for the padded bins
};

template <int NB, bool LOGSIG>
__global__ __launch_bounds__(kThreads) void smf_jac_lanes_kernel(
    const int32_t* __restrict__ slot_pop, const int32_t* __restrict__ slot_part,
    const float2* __restrict__ theta, const float* __restrict__ resid, int64_t s0, int64_t s1,
    JacCoef coef, int nb, float2* __restrict__ jac, int64_t ldj, float2* __restrict__ partials) {
  constexpr int R = 2 * (NB + 1);
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t g0 = s0 / kWave, g1 = s1 / kWave;
  const int xcd = blockIdx.x % kXcds;
  const int64_t nbx = gridDim.x / kXcds;  // host launches a multiple of kXcds blocks
  const int64_t ngx = (g1 - g0 + kXcds - 1) / kXcds;
  const int64_t ga = g0 + xcd * ngx, gb = min(g1, ga + ngx);
  const int64_t nw = nbx * (kThreads / kWave);
  int64_t g = ga + (int64_t)(blockIdx.x / kXcds) * (kThreads / kWave) + (threadIdx.x >> 6);
  float r[R];
  int c = -1, part = -1;
  if (g < gb) {
#pragma unroll
    for (int e = 0; e < R; ++e) r[e] = resid[(g * R + e) * kWave + lane];
    c = slot_pop[g * kWave + lane];
    part = slot_part[g * kWave + lane];
  }
  while (g < gb) {
    float A[NB], B[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      A[k] = coef.c[k] * (r[k + 1] - r[k]);
      B[k] = coef.c[k] * (r[NB + 2 + k] - r[NB + 1 + k]);
    }
    const int cc = c, pp = part;
    const int64_t gn = g + nw;
    if (gn < gb) {
#pragma unroll
      for (int e = 0; e < R; ++e) r[e] = resid[(gn * R + e) * kWave + lane];
      c = slot_pop[gn * kWave + lane];
      part = slot_part[gn * kWave + lane];
    }
    if (cc >= 0) {
      if (pp >= 0) {
#pragma unroll
        for (int k = 0; k < NB; ++k)
          if (k < nb) partials[(int64_t)pp * nb + k] = make_float2(A[k], B[k]);
      } else {
        const float2 th = theta[cc];
#pragma unroll
        for (int k = 0; k < NB; ++k)
          if (k < nb) jac[(int64_t)k * ldj + cc] = pop_grad<LOGSIG>(th, A[k], B[k]);
      }
    }
    g = gn;
  }
}

// grid (split populations, nb): giant [G, 3] = {pop, part_begin, part_end}.
template <bool LOGSIG>
__global__ __launch_bounds__(kThreads) void smf_jac_finalize_kernel(
    const int32_t* __restrict__ giant, const float2* __restrict__ partials, int nb,
    const float2* __restrict__ theta, float2* __restrict__ jac, int64_t ldj) {
  const int c = giant[3 * blockIdx.x], p0 = giant[3 * blockIdx.x + 1], p1 = giant[3 * blockIdx.x + 2];
  const int k = blockIdx.y;
  double v[2] = {0.0, 0.0};
  for (int s = p0 + threadIdx.x; s < p1; s += kThreads) {
    const float2 p = partials[(int64_t)s * nb + k];
    v[0] += p.x; v[1] += p.y;
  }
  __shared__ double scratch[2 * (kThreads / kWave)];
  block_sum_n<2>(v, scratch);
  if (threadIdx.x == 0)
    jac[(int64_t)k * ldj + c] = pop_grad<LOGSIG>(theta[c], (float)v[0], (float)v[1]);
}

// Jacobian rows over slots [s0, s1) into jac [nb, theta.numel()] (the columns of these
// slots' populations only), plus the finalize of the split populations in giant [G, 3].
// partials: float32 [>= 2 nb nparts] where nparts bounds every part index of the slots.
void smf_jacobian_lanes(torch::Tensor slot_pop, torch::Tensor slot_part, torch::Tensor theta,
                        torch::Tensor resid, int64_t s0, int64_t s1, std::vector<double> scale,
                        bool log_sigma, torch::Tensor jac, torch::Tensor partials, int64_t nparts,
                        torch::Tensor giant) {
  check_dev(slot_pop, "slot_pop", at::kInt);
  check_dev(slot_part, "slot_part", at::kInt);
  check_dev(theta, "theta", at::kFloat);
  check_dev(resid, "resid", at::kFloat);
  check_dev(jac, "jac", at::kFloat);
  const int nb = (int)scale.size();
  const int nbp = padded_bins(nb);
  TORCH_CHECK(nb >= 1, "need at least one bin");
  TORCH_CHECK(theta.numel() % 2 == 0 && jac.dim() == 2 && jac.size(0) == nb &&
                  jac.size(1) == theta.numel(), "jac must be [nb, theta.numel()]");
  const int64_t ns = slot_pop.numel();
  TORCH_CHECK(slot_part.numel() == ns && resid.dim() == 3 && resid.size(0) * kWave == ns &&
                  resid.size(1) == 2 * (nbp + 1) && resid.size(2) == kWave, "inconsistent residuals");
  TORCH_CHECK(s0 >= 0 && s1 <= ns && s0 <= s1, "bad slot range");
  TORCH_CHECK(s0 % kWave == 0 && s1 % kWave == 0, "slot ranges must be group aligned");
  const int64_t ng = giant.numel() / 3;
  float2* pa = nullptr;
  if (nparts > 0) {
    check_dev(partials, "partials", at::kFloat);
    TORCH_CHECK(partials.numel() >= 2 * (int64_t)nb * nparts, "partials too small");
    pa = reinterpret_cast<float2*>(partials.data_ptr<float>());
  }
  TORCH_CHECK(ng == 0 || pa != nullptr, "partials buffer required for split populations");
  JacCoef coef;
  for (int k = 0; k < kMaxBins; ++k)
    coef.c[k] = k < nb ? (float)(scale[k] / std::sqrt(2.0 * M_PI)) : 0.0f;
  auto stream = at::hip::getCurrentHIPStream();
  const float2* tp = reinterpret_cast<const float2*>(theta.data_ptr<float>());
  float2* jp = reinterpret_cast<float2*>(jac.data_ptr<float>());
  const int64_t ldj = theta.numel() / 2;
  if (s1 > s0) {
    static int64_t caps[kMaxBins + 1] = {0};  // per padded bin count (register use differs)
    int64_t& cap = caps[nbp];
    if (cap == 0)
      MG_DISPATCH_NB(nbp, {
        cap = resident_blocks((const void*)smf_jac_lanes_kernel<NB, true>, kThreads);
      });
    const int64_t want = (s1 - s0 + kThreads - 1) / kThreads;
    const int64_t nblk = std::max<int64_t>(kXcds, std::min(cap, want) / kXcds * kXcds);
    MG_DISPATCH_NB(nbp, {
      with_bool(log_sigma, [&](auto LS) {
        hipLaunchKernelGGL((smf_jac_lanes_kernel<NB, decltype(LS)::value>), dim3(nblk),
                           dim3(kThreads), 0, stream, slot_pop.data_ptr<int32_t>(),
                           slot_part.data_ptr<int32_t>(), tp, resid.data_ptr<float>(), s0, s1, coef,
                           nb, jp, ldj, pa);
      });
    });
  }
  if (ng > 0) {
    check_dev(giant, "giant", at::kInt);
    with_bool(log_sigma, [&](auto LS) {
      hipLaunchKernelGGL((smf_jac_finalize_kernel<decltype(LS)::value>), dim3(ng, nb), dim3(kThreads),
                         0, stream, giant.data_ptr<int32_t>(), pa, nb, tp, jp, ldj);
    });
  }
}

}  // namespace mg
