// Two-axis Gaussian-binned sum for user-written models (ops/binned2d.py):
//   out[j][k] = sum_i w_i * Px_i[j] * Py_i[k]
//   Px_i[j]   = Phi((ex[j+1] - mux_i)/sigx_i) - Phi((ex[j] - mux_i)/sigx_i)   (Py likewise)
// with per-object means, widths and weights produced by arbitrary torch code.
//
// Forward : the product [nbx x T] . [T x nby] over tiles of T = 256 objects.  Phase A: thread t
//           evaluates the edge CDFs of object t of the tile and writes w*Px[.] and Py[.] as one
//           row of LDS (row stride NBX + NBY + 2 floats: twice an odd number, so the 4-byte
//           writes of a wave are at most two-way conflicted, which costs nothing, and every
//           row is 8-byte aligned).  Phase B: thread (slice, cell tile) owns a 4x4 register
//           tile of cells and sweeps the rows slice, slice + NSL, ... with 8-byte LDS reads
//           (all lanes of a cell-tile column read the same address: broadcast), accumulating
//           into fresh registers per tile of objects; the tile partial is then added to the
//           workgroup's running total.  At the end the NSL slices are folded in LDS in a fixed
//           order, the workgroup total goes to one slab row [blocks, NBX*NBY], and a
//           fixed-order reduction over column groups sums the rows (a single launch when one
//           workgroup covers the input).
// Backward: per-object parallel (V = 4 objects per thread, 2 when NBY = 32), recomputing from
//           the inputs (no residuals).  G is staged once per workgroup in LDS (<= 4 KiB).  One
//           sweep over the rows of G forms u_j = sum_k G[j][k] Py[k] (complete after row j) and
//           v[k] += G[j][k] Px[j]; Px[j], the x-edge Gaussians and hx_j = u_{j-1} - u_j are
//           produced and consumed inside the sweep, so only Py and v live in registers.  The
//           y-edge sweep then recomputes its Gaussians (one v_exp each).  Gradients of
//           broadcast operands go block sum -> [blocks, 4] slab -> fixed-order reduce.
// No float atomics anywhere: results are bitwise reproducible for a fixed N, shape and device.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <tuple>
#include <vector>

#include "binned_host.h"

namespace mg {

namespace {

constexpr int kTile = kBinThreads;  // objects per forward tile: one per thread in phase A

struct Binned2dArgs {
  const float* mux;
  const float* sigx;
  const float* muy;
  const float* sigy;
  const float* w;  // nullptr: every weight is 1
  int64_t n;
  int nbx, nby;    // real bins (<= the padded template counts)
  int sigx_b;      // sigma_x has one element
  int sigy_b;
  int w_b;
  int wide;        // every per-object input pointer is 16-byte aligned
  float ex[kMaxBins + 1];
  float ey[kMaxBins + 1];
};

struct Binned2dGrad {
  const float* g;  // [nbx, nby] cotangent
  float* dmux;     // [n]
  float* dsigx;    // [n], or [1] when sigma_x is broadcast
  float* dmuy;
  float* dsigy;
  float* dw;
  float* slab;     // [blocks, 4] partial sums of the broadcast gradients (sigx, sigy, w, unused)
  int need_x;      // mu_x or sigma_x wanted
  int need_y;
};

// The CDF differences of one object over the edges e[0..nb] into dst[0..nb), scaled by `scale`;
// dst[nb..nbp) = 0.
__device__ __forceinline__ void write_axis(const float* e, int nb, int nbp, float m, float inv,
                                           float scale, float* dst) {
  float b0, f0, gs;
  edge_cdf((e[0] - m) * inv, b0, f0, gs);
#pragma unroll 4
  for (int k = 1; k <= nb; ++k) {
    float b1, f1;
    edge_cdf((e[k] - m) * inv, b1, f1, gs);
    dst[k - 1] = scale * ((b1 - b0) + (f1 - f0));
    b0 = b1;
    f0 = f1;
  }
  for (int k = nb; k < nbp; ++k) dst[k] = 0.0f;
}

template <int NBX, int NBY>
struct Fwd2d {
  static constexpr int kStride = NBX + NBY + 2;           // floats per LDS row
  static constexpr int kCellTiles = (NBX / 4) * (NBY / 4);
  static constexpr int kSlices = kBinThreads / kCellTiles;  // object slices of phase B
  static constexpr int kFold = kBinThreads * 16;            // floats of the final fold
  static constexpr int kLds = kTile * kStride > kFold ? kTile * kStride : kFold;
};

template <int NBX, int NBY>
__global__ __launch_bounds__(kBinThreads) void binned2d_fwd_kernel(Binned2dArgs a, float* slab,
                                                                   float* out, int direct) {
  using F = Fwd2d<NBX, NBY>;
  constexpr int S = F::kStride, NSL = F::kSlices, NCT = F::kCellTiles;
  __shared__ __attribute__((aligned(16))) float lds[F::kLds];
  const int tid = threadIdx.x;
  const int ct = tid % NCT, sl = tid / NCT;
  const int j0 = (ct / (NBY / 4)) * 4, k0 = (ct % (NBY / 4)) * 4;
  float tot[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) tot[p][q] = 0.0f;
  const int64_t ntiles = (a.n + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    {  // phase A: this thread's object -> one LDS row (objects beyond N: weight 0)
      const int64_t i = tile * kTile + tid;
      const bool ok = i < a.n;
      const float mx = ok ? a.mux[i] : 0.0f;
      const float my = ok ? a.muy[i] : 0.0f;
      const float sx = ok ? a.sigx[a.sigx_b ? 0 : i] : 1.0f;
      const float sy = ok ? a.sigy[a.sigy_b ? 0 : i] : 1.0f;
      const float wt = !ok ? 0.0f : a.w == nullptr ? 1.0f : a.w[a.w_b ? 0 : i];
      float* row = lds + tid * S;
      write_axis(a.ex, a.nbx, NBX, mx, 1.0f / sx, wt, row);
      write_axis(a.ey, a.nby, NBY, my, 1.0f / sy, 1.0f, row + NBX);
    }
    __syncthreads();
    {  // phase B: 4x4 cells x the objects of this slice, fresh accumulators per tile
      float acc[4][4];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0f;
      const float* px = lds + j0;
      const float* py = lds + NBX + k0;
#pragma unroll 4
      for (int t = sl; t < kTile; t += NSL) {
        const float2 xa = *reinterpret_cast<const float2*>(px + t * S);
        const float2 xb = *reinterpret_cast<const float2*>(px + t * S + 2);
        const float2 ya = *reinterpret_cast<const float2*>(py + t * S);
        const float2 yb = *reinterpret_cast<const float2*>(py + t * S + 2);
        const float x[4] = {xa.x, xa.y, xb.x, xb.y};
        const float y[4] = {ya.x, ya.y, yb.x, yb.y};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[p][q] = fmaf(x[p], y[q], acc[p][q]);
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) tot[p][q] += acc[p][q];
    }
    __syncthreads();
  }
  // fold the slices: lds[(sl * NCT + ct) * 16 + p * 4 + q], then cell c sums over sl in four
  // interleaved chains (fixed order)
#pragma unroll
  for (int p = 0; p < 4; ++p)
    *reinterpret_cast<float4*>(lds + tid * 16 + p * 4) =
        make_float4(tot[p][0], tot[p][1], tot[p][2], tot[p][3]);
  __syncthreads();
  for (int c = tid; c < NBX * NBY; c += kBinThreads) {
    const int j = c / NBY, k = c % NBY;
    const int cell = ((j / 4) * (NBY / 4) + k / 4) * 16 + (j % 4) * 4 + (k % 4);
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
    for (int r = 0; r < NSL; r += 4) {  // NSL is a multiple of 4 (at most 64 cell tiles)
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] += lds[(r + u) * NCT * 16 + cell];
    }
    const float total = (s[0] + s[1]) + (s[2] + s[3]);
    if (direct) {
      if (j < a.nbx && k < a.nby) out[j * a.nby + k] = total;
    } else {
      slab[(int64_t)blockIdx.x * (NBX * NBY) + c] = total;
    }
  }
}

template <int NBY, int V>
__global__ __launch_bounds__(kBinThreads) void binned2d_bwd_kernel(Binned2dArgs a, Binned2dGrad o,
                                                                   int direct) {
  __shared__ __attribute__((aligned(16))) float G[kMaxBins * NBY];  // [nbx][NBY], zero padded
  __shared__ float red[3 * (kBinThreads / kWave)];
  for (int c = threadIdx.x; c < a.nbx * NBY; c += kBinThreads) {
    const int j = c / NBY, k = c % NBY;
    G[c] = k < a.nby ? o.g[j * a.nby + k] : 0.0f;
  }
  __syncthreads();
  const bool red_sx = o.dsigx != nullptr && a.sigx_b;
  const bool red_sy = o.dsigy != nullptr && a.sigy_b;
  const bool red_w = o.dw != nullptr && a.w_b;
  float rs[3] = {0.0f, 0.0f, 0.0f};  // this thread's share of the broadcast gradients
  const int64_t ng = (a.n + V - 1) / V;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < ng; q += stride) {
    const int64_t i0 = q * V;
    float mx[V], my[V], sx[V], sy[V], wt[V], ix[V], iy[V];
    const bool full = a.wide && i0 + V <= a.n;  // one branch for the five operands
    load_group<V>(a.mux, i0, a.n, full, false, 0.0f, 0.0f, mx);
    load_group<V>(a.muy, i0, a.n, full, false, 0.0f, 0.0f, my);
    load_group<V>(a.sigx, i0, a.n, full, a.sigx_b, 1.0f, 1.0f, sx);
    load_group<V>(a.sigy, i0, a.n, full, a.sigy_b, 1.0f, 1.0f, sy);
    load_group<V>(a.w, i0, a.n, full, a.w_b, 1.0f, 0.0f, wt);
    // Py (unweighted), and v = G^T Px accumulated over the rows of G
    float Py[V][NBY], v[V][NBY];
    float b0[V], f0[V];
#pragma unroll
    for (int e = 0; e <= NBY; ++e) {
      if (e <= a.nby) {  // wave-uniform: padded bins cost nothing
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if (e == 0) {
            ix[j] = 1.0f / sx[j];
            iy[j] = 1.0f / sy[j];
          }
          float b1, f1, gs;
          edge_cdf((a.ey[e] - my[j]) * iy[j], b1, f1, gs);
          if (e > 0) Py[j][e > 0 ? e - 1 : 0] = (b1 - b0[j]) + (f1 - f0[j]);
          b0[j] = b1;
          f0[j] = f1;
        }
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) Py[j][e - 1] = 0.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
      for (int k = 0; k < NBY; ++k) v[j][k] = 0.0f;
    // the sweep over rows of G: x edge r + 1 closes bin r
    float Ax[V], Bx[V], C[V], up[V], gp[V], zp[V];  // previous u, Gaussian and z (edge r)
#pragma unroll
    for (int j = 0; j < V; ++j) {
      zp[j] = (a.ex[0] - mx[j]) * ix[j];
      edge_cdf(zp[j], b0[j], f0[j], gp[j]);
      Ax[j] = Bx[j] = C[j] = up[j] = 0.0f;
    }
    for (int r = 0; r < a.nbx; ++r) {
      const float er = a.ex[r + 1];
      float Px[V], u[V], z1[V], g1[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float b1, f1;
        z1[j] = (er - mx[j]) * ix[j];
        edge_cdf(z1[j], b1, f1, g1[j]);
        Px[j] = (b1 - b0[j]) + (f1 - f0[j]);
        b0[j] = b1;
        f0[j] = f1;
        u[j] = 0.0f;
      }
      const float* grow = G + r * NBY;
#pragma unroll
      for (int k4 = 0; k4 < NBY; k4 += 4) {
        if (k4 < a.nby) {
          const float4 gv = *reinterpret_cast<const float4*>(grow + k4);  // broadcast read
          const float gk[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) {
              u[j] = fmaf(gk[k], Py[j][k4 + k], u[j]);
              v[j][k4 + k] = fmaf(gk[k], Px[j], v[j][k4 + k]);
            }
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        C[j] = fmaf(Px[j], u[j], C[j]);
        if (o.need_x) {  // edge r carries hx_r = u_{r-1} - u_r
          const float hg = (up[j] - u[j]) * gp[j];
          Ax[j] += hg;
          Bx[j] = fmaf(hg, zp[j], Bx[j]);
        }
        up[j] = u[j];
        gp[j] = g1[j];
        zp[j] = z1[j];
      }
    }
    float dmx[V], dsx[V], dmy[V], dsy[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float hg = up[j] * gp[j];  // the last edge: hx_nbx = u_{nbx-1}
      Ax[j] += hg;
      Bx[j] = fmaf(hg, zp[j], Bx[j]);
      const float c = -kInvSqrt2PiB * wt[j] * ix[j];  // 0 beyond N (weight 0)
      dmx[j] = c * Ax[j];
      dsx[j] = c * Bx[j];
      if (i0 + j >= a.n) C[j] = 0.0f;
    }
    if (o.need_y) {  // the y-edge sweep, Gaussians recomputed
      float Ay[V], By[V];
#pragma unroll
      for (int j = 0; j < V; ++j) Ay[j] = By[j] = 0.0f;
#pragma unroll
      for (int e = 0; e <= NBY; ++e) {
        if (e <= a.nby) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float z = (a.ey[e] - my[j]) * iy[j];
            const float ws = z * kWScale;
            const float lo = e > 0 ? v[j][e > 0 ? e - 1 : 0] : 0.0f;
            const float hi = e < NBY ? v[j][e < NBY ? e : 0] : 0.0f;  // 0 for padded bins
            const float hg = (lo - hi) * fast_exp2(-ws * ws);
            Ay[j] += hg;
            By[j] = fmaf(hg, z, By[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float c = -kInvSqrt2PiB * wt[j] * iy[j];
        dmy[j] = c * Ay[j];
        dsy[j] = c * By[j];
      }
    }
    if (o.dmux) store_group<V>(o.dmux, i0, a.n, dmx);
    if (o.dmuy) store_group<V>(o.dmuy, i0, a.n, dmy);
    if (o.dsigx) {
      if (red_sx) {
#pragma unroll
        for (int j = 0; j < V; ++j) rs[0] += dsx[j];
      } else {
        store_group<V>(o.dsigx, i0, a.n, dsx);
      }
    }
    if (o.dsigy) {
      if (red_sy) {
#pragma unroll
        for (int j = 0; j < V; ++j) rs[1] += dsy[j];
      } else {
        store_group<V>(o.dsigy, i0, a.n, dsy);
      }
    }
    if (o.dw) {
      if (red_w) {
#pragma unroll
        for (int j = 0; j < V; ++j) rs[2] += C[j];
      } else {
        store_group<V>(o.dw, i0, a.n, C);
      }
    }
  }
  if (red_sx || red_sy || red_w) {  // uniform over the grid
    block_sum_n<3>(rs, red);
    if (threadIdx.x == 0) {
      if (direct) {
        if (red_sx) o.dsigx[0] = rs[0];
        if (red_sy) o.dsigy[0] = rs[1];
        if (red_w) o.dw[0] = rs[2];
      } else {
        *reinterpret_cast<float4*>(o.slab + (int64_t)blockIdx.x * 4) =
            make_float4(rs[0], rs[1], rs[2], 0.0f);
      }
    }
  }
}

constexpr const char* kOp2d = "gaussian_binned_sum_2d";

Binned2dArgs make_args2d(const torch::Tensor& mux, const torch::Tensor& sigx,
                         const torch::Tensor& muy, const torch::Tensor& sigy,
                         const c10::optional<torch::Tensor>& w, const std::vector<double>& ex,
                         const std::vector<double>& ey) {
  Binned2dArgs a;
  a.n = mux.numel();
  a.nbx = (int)ex.size() - 1;
  a.nby = (int)ey.size() - 1;
  padded_bins(a.nbx, kOp2d, "x");
  padded_bins(a.nby, kOp2d, "y");
  set_edges(ex, a.nbx, a.ex, kOp2d);
  set_edges(ey, a.nby, a.ey, kOp2d);
  bool wide = true;
  int none = 0;
  a.mux = operand(mux, "mu_x", a.n, none, wide);
  TORCH_CHECK(muy.numel() == a.n, "mu_y must have N elements");
  a.muy = operand(muy, "mu_y", a.n, none, wide);
  a.sigx = operand(sigx, "sigma_x", a.n, a.sigx_b, wide);
  a.sigy = operand(sigy, "sigma_y", a.n, a.sigy_b, wide);
  a.w = nullptr;
  a.w_b = 0;
  if (w.has_value() && w->defined()) a.w = operand(*w, "weights", a.n, a.w_b, wide);
  a.wide = wide;
  return a;
}

}  // namespace

torch::Tensor binned2d_forward(torch::Tensor mux, torch::Tensor sigx, torch::Tensor muy,
                               torch::Tensor sigy, c10::optional<torch::Tensor> w,
                               std::vector<double> ex, std::vector<double> ey) {
  Binned2dArgs a = make_args2d(mux, sigx, muy, sigy, w, ex, ey);
  TORCH_CHECK(a.n > 0, "binned2d_forward: empty input");
  const int nbxp = padded_bins(a.nbx, kOp2d, "x"), nbyp = padded_bins(a.nby, kOp2d, "y");
  auto out = torch::empty({a.nbx, a.nby}, mux.options());
  auto stream = at::hip::getCurrentHIPStream();
  const int64_t tiles = (a.n + kTile - 1) / kTile;
  MG_DISPATCH_PAD(nbxp, NBX, MG_DISPATCH_PAD(nbyp, NBY, {
    constexpr int kCells = NBX * NBY, kGroup = kCells < 32 ? kCells : 32;
    launch_slab_fwd<binned2d_fwd_kernel<NBX, NBY>>(
        tiles, ReduceFwd{kCells, kGroup, kCells / kGroup, NBY, a.nbx, a.nby},
        out.data_ptr<float>(), mux, stream, a);
  }));
  return out;
}

// Gradients of sum_jk g_jk out_jk with respect to the requested operands, in the order
// (mu_x, sigma_x, mu_y, sigma_y, weights); an operand that was not requested comes back
// undefined (None).  A broadcast operand gets the sum over objects.
std::vector<torch::Tensor> binned2d_backward(torch::Tensor mux, torch::Tensor sigx,
                                             torch::Tensor muy, torch::Tensor sigy,
                                             c10::optional<torch::Tensor> w, std::vector<double> ex,
                                             std::vector<double> ey, torch::Tensor g,
                                             std::vector<bool> need) {
  Binned2dArgs a = make_args2d(mux, sigx, muy, sigy, w, ex, ey);
  TORCH_CHECK(a.n > 0, "binned2d_backward: empty input");
  check_dev(g, "grad_out", at::kFloat);
  TORCH_CHECK(g.numel() == (int64_t)a.nbx * a.nby, "grad_out must have nbx * nby elements");
  TORCH_CHECK(need.size() == 5, "need: five flags");
  TORCH_CHECK(!need[4] || a.w != nullptr, "weights gradient requested without weights");
  TORCH_CHECK(need[0] || need[1] || need[2] || need[3] || need[4], "no gradient requested");
  const int nbyp = padded_bins(a.nby, kOp2d, "y");
  std::vector<torch::Tensor> grads(5);
  const int64_t sizes[5] = {a.n, sigx.numel(), a.n, sigy.numel(), a.w ? w->numel() : 0};
  float* ptr[5];
  for (int i = 0; i < 5; ++i) grads[i] = alloc_grad(need[i], sizes[i], mux, ptr[i]);
  Binned2dGrad o;
  o.g = g.data_ptr<float>();
  o.dmux = ptr[0];
  o.dsigx = ptr[1];
  o.dmuy = ptr[2];
  o.dsigy = ptr[3];
  o.dw = ptr[4];
  o.slab = nullptr;
  o.need_x = need[0] || need[1];
  o.need_y = need[2] || need[3];
  ReduceBwd r = {};  // the [blocks, 4] slab: sigma_x, sigma_y, w, unused
  r.out[0] = a.sigx_b ? o.dsigx : nullptr;
  r.out[1] = a.sigy_b ? o.dsigy : nullptr;
  r.out[2] = a.w_b ? o.dw : nullptr;
  auto stream = at::hip::getCurrentHIPStream();
  MG_DISPATCH_PAD(nbyp, NBY, {
    constexpr int V = NBY == 32 ? 2 : 4;
    launch_slab_bwd<binned2d_bwd_kernel<NBY, V>>(a, o, blocks_for(a.n, V), 4, r, mux, stream);
  });
  return grads;
}

}  // namespace mg
