// One pass of the box-constrained dual Gauss-Newton solve over a short, wide Jacobian
// (optim/gauss_newton_box.py).  For J [K, n] float32, coefficients a [K] float64, the scaling
// d [n] > 0, the damping lam and the step box lo <= 0 <= hi [n] (+-inf allowed), per column p
//
//   t = sum_k a[k] J[k, p],   sigma = -t / (lam d[p]),   delta = clip(sigma, lo[p], hi[p]),
//   free = lo[p] < sigma < hi[p],
//
// and the sums over the columns
//
//   v[k]    = sum_p J[k, p] delta_p                      (K values)
//   W[k, l] = sum_p J[k, p] (free_p / (lam d_p)) J[l, p]  (K x K, symmetric)
//   s       = sum_p (t_p delta_p + lam d_p delta_p^2 / 2)
//   nfree   = sum_p free_p
//
// returned as one float64 block [v, W, s, nfree] (K + K*K + 2 values); delta, rounded to
// float32, is written only when the caller passes a buffer.
//
// Structure as gram.hip: J is streamed once, every thread keeps the K + K (K + 1) / 2 + 2
// float64 accumulators in registers, operands are converted to float64 before the first
// multiply and the sums use the unrounded delta (so the equation the host solves is exactly
// piecewise linear in a), and the per-thread sums are reduced in a fixed order: wave
// shuffles, LDS, one slab row per workgroup, and a final per-entry reduce kernel that also
// mirrors the lower triangle of W.  No atomics: bitwise reproducible for a fixed n and
// device.  The reciprocal 1 / (lam d) is taken once per column and serves sigma and W.
// The group loads, the slab-row store, the slab entry sum and the triangle decode are
// sweep_device.h's; the cap, the grid and the row-tile dispatch are sweep_host.h's.
//
// Loads are 16 bytes wide when every pointer, the row stride and n allow it (the last n % 4
// columns by guarded scalar loads); otherwise every load is a guarded scalar load.
#include "sweep_device.h"
#include "sweep_host.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace mg {

constexpr int kBoxThreads = 256;
constexpr int kBoxMaxBlocks = 1024;  // slab rows
constexpr int kBoxMaxRows = 10;      // largest instantiation: T = 16 spills to scratch

// Accumulator layout of one thread (and of a slab row): v[T], the upper triangle of W row by
// row, s, nfree.
template <int T>
struct BoxAcc {
  static constexpr int kTri = T * (T + 1) / 2;
  static constexpr int kEntries = T + kTri + 2;
};

// One column group: G = 4 columns (one float4 per row) or 1 column.
template <int T, int G>
__device__ __forceinline__ void box_dual_accumulate(const float (&x)[T][G], const double (&a)[T],
                                                    const float (&dv)[G], const float (&lov)[G],
                                                    const float (&hiv)[G], double lam,
                                                    double (&acc)[BoxAcc<T>::kEntries],
                                                    float (&dout)[G]) {
#pragma unroll
  for (int q = 0; q < G; ++q) {
    double xd[T];
#pragma unroll
    for (int k = 0; k < T; ++k) xd[k] = (double)x[k][q];
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < T; ++k) t = fma(a[k], xd[k], t);
    const double ld = lam * (double)dv[q];
    const double r = 1.0 / ld;
    const double sigma = -t * r;
    const double lo = (double)lov[q], hi = (double)hiv[q];
    const bool free = sigma > lo && sigma < hi;
    const double delta = fmin(fmax(sigma, lo), hi);
    const double w = free ? r : 0.0;
#pragma unroll
    for (int k = 0; k < T; ++k) acc[k] = fma(xd[k], delta, acc[k]);
    int e = T;
#pragma unroll
    for (int k = 0; k < T; ++k) {
      const double xw = xd[k] * w;
#pragma unroll
      for (int l = k; l < T; ++l) {
        acc[e] = fma(xw, xd[l], acc[e]);
        ++e;
      }
    }
    acc[e] = fma(delta, fma(0.5 * ld, delta, t), acc[e]);
    acc[e + 1] += free ? 1.0 : 0.0;
    dout[q] = (float)delta;
  }
}

// Column group j of the sweep: loads, sums and the delta store.
template <int T, int G>
__device__ __forceinline__ void box_dual_group(int64_t j, const float* (&row)[T],
                                               const double (&a)[T], const float* d,
                                               const float* lo, const float* hi, double lam,
                                               float* delta_out,
                                               double (&acc)[BoxAcc<T>::kEntries]) {
  float x[T][G], dv[G], lov[G], hiv[G], dout[G];
  load_group<G>(d, j, dv);
  load_group<G>(lo, j, lov);
  load_group<G>(hi, j, hiv);
  load_group_rows<T, G>(row, j, x);
  box_dual_accumulate<T, G>(x, a, dv, lov, hiv, lam, acc, dout);
  if (delta_out) {
    if constexpr (G == 4)
      reinterpret_cast<float4*>(delta_out)[j] = make_float4(dout[0], dout[1], dout[2], dout[3]);
    else
      delta_out[j] = dout[0];
  }
}

// grid.x: column slices (grid-stride).  Row indices past K are clamped to the last row with
// a zero coefficient (their sums are never read).
template <int T, bool VEC>
__global__ __launch_bounds__(kBoxThreads) void box_dual_kernel(
    const float* __restrict__ J, int64_t ld, int K, const double* __restrict__ coef,
    const float* __restrict__ d, double lam, const float* __restrict__ lo,
    const float* __restrict__ hi, int64_t n, float* __restrict__ delta_out,
    double* __restrict__ slab) {
  constexpr int NE = BoxAcc<T>::kEntries;
  const float* row[T];
  double a[T];
#pragma unroll
  for (int k = 0; k < T; ++k) {
    row[k] = J + (int64_t)min(k, K - 1) * ld;
    a[k] = k < K ? coef[k] : 0.0;
  }
  double acc[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) acc[e] = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * kBoxThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBoxThreads;
  // float4 groups first, then single columns; the loops stay here: inside a helper they
  // cost box_dual_kernel<1, true> 20 VGPRs
  int64_t j0 = 0;
  if constexpr (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t j = tid; j < n4; j += stride)
      box_dual_group<T, 4>(j, row, a, d, lo, hi, lam, delta_out, acc);
    j0 = n4 << 2;
  }
  for (int64_t j = j0 + tid; j < n; j += stride)
    box_dual_group<T, 1>(j, row, a, d, lo, hi, lam, delta_out, acc);
  double* out = slab + (int64_t)blockIdx.x * NE;
  slab_row_store<kBoxThreads>(out, acc);
}

// One workgroup per slab entry e: the fixed-order sum over the bx slab rows, written to its
// place in the [v, W, s, nfree] block (W mirrored).
__global__ __launch_bounds__(kBoxThreads) void box_dual_reduce_kernel(
    const double* __restrict__ slab, int bx, int ne, int T, int K, double* __restrict__ out) {
  const int e = blockIdx.x;
  const int tri = T * (T + 1) / 2;
  int64_t at = -1, mirror = -1;  // uniform per workgroup
  if (e < T) {
    if (e < K) at = e;
  } else if (e < T + tri) {
    int k, l;
    triangle_index(e - T, T, k, l);
    if (l < K) {
      at = K + (int64_t)k * K + l;
      mirror = K + (int64_t)l * K + k;
    }
  } else {
    at = K + (int64_t)K * K + (e - T - tri);
  }
  if (at < 0) return;
  const double s =
      slab_entry_sum<kBoxThreads>(bx, [&](int r) { return slab[(int64_t)r * ne + e]; });
  if (threadIdx.x == 0) {
    out[at] = s;
    if (mirror >= 0) out[mirror] = s;
  }
}

template <int T>
static void launch_box_dual(const float* J, int64_t ld, int K, const double* coef, const float* d,
                            double lam, const float* lo, const float* hi, int64_t n, bool vec,
                            float* delta_out, double* out, const torch::Tensor& like,
                            hipStream_t stream) {
  constexpr int NE = BoxAcc<T>::kEntries;
  auto kv = box_dual_kernel<T, true>;
  auto ks = box_dual_kernel<T, false>;
  static GridCap cap;  // of the 16-byte-load instantiation: one grid for both load paths
  const int64_t bx = chunk_grid(sweep_chunks(n, vec), kBoxThreads,
                                resident_cap(cap, kBoxMaxBlocks, kBoxThreads, kv));
  auto slab = torch::empty({bx * NE}, like.options().dtype(at::kDouble));
  double* sp = slab.data_ptr<double>();
  hipLaunchKernelGGL(vec ? kv : ks, dim3((unsigned)bx), dim3(kBoxThreads), 0, stream, J, ld, K,
                     coef, d, lam, lo, hi, n, delta_out, sp);
  hipLaunchKernelGGL(box_dual_reduce_kernel, dim3(NE), dim3(kBoxThreads), 0, stream, sp, (int)bx,
                     NE, T, K, out);
}

// Whether a launch takes the 16-byte-load kernel: every pointer 16-byte aligned, rows a
// multiple of 4 floats apart and at least one float4 of columns.
static bool box_vector_loads(const float* J, int K, int64_t ld, const float* d, const float* lo,
                             const float* hi, const float* delta_out, int64_t n) {
  return aligned16(J) && (K == 1 || ld % 4 == 0) && aligned16(d) && aligned16(lo) &&
         aligned16(hi) && (!delta_out || aligned16(delta_out)) && n >= 4;
}

// The same decision for the tensors of a call (tests and benchmarks record the path with it).
bool box_dual_vector_loads(torch::Tensor J, torch::Tensor d, torch::Tensor lo, torch::Tensor hi,
                           c10::optional<torch::Tensor> delta_out) {
  TORCH_CHECK(J.dim() == 2 && J.scalar_type() == at::kFloat && d.scalar_type() == at::kFloat &&
                  lo.scalar_type() == at::kFloat && hi.scalar_type() == at::kFloat,
              "float32 tensors, J 2-d");
  const int64_t rows = J.size(0), n = J.size(1);
  const float* dp = nullptr;
  if (delta_out.has_value() && delta_out->defined()) {
    TORCH_CHECK(delta_out->scalar_type() == at::kFloat, "float32 delta_out");
    dp = delta_out->data_ptr<float>();
  }
  return box_vector_loads(J.data_ptr<float>(), (int)rows, rows > 1 ? J.stride(0) : n,
                          d.data_ptr<float>(), lo.data_ptr<float>(), hi.data_ptr<float>(), dp, n);
}

// J: [K, n] float32 with unit column stride, 1 <= K <= 10; coef: [K] float64; d, lo, hi: [n]
// float32, contiguous; delta_out: [n] float32, contiguous, or none.  Returns the float64 block
// [v (K), W (K*K), s, nfree] on J's device.  Current stream, no host synchronisation.
torch::Tensor box_dual_pass(torch::Tensor J, torch::Tensor coef, torch::Tensor d, double lam,
                            torch::Tensor lo, torch::Tensor hi,
                            c10::optional<torch::Tensor> delta_out) {
  TORCH_CHECK(J.is_cuda() && J.scalar_type() == at::kFloat, "J must be a float32 device tensor");
  TORCH_CHECK(J.dim() == 2 && (J.size(1) <= 1 || J.stride(1) == 1), "J must be row-major 2-d");
  const int64_t rows = J.size(0), n = J.size(1);
  TORCH_CHECK(rows >= 1 && rows <= kBoxMaxRows, "box_dual_pass takes 1..10 rows of J");
  TORCH_CHECK(coef.is_cuda() && coef.scalar_type() == at::kDouble && coef.is_contiguous() &&
                  coef.numel() == rows && coef.get_device() == J.get_device(),
              "coef must be a contiguous float64 [K] tensor on J's device");
  auto vec_ok = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.dim() == 1 &&
           t.numel() == n && t.get_device() == J.get_device();
  };
  TORCH_CHECK(vec_ok(d) && vec_ok(lo) && vec_ok(hi),
              "d, lo and hi must be contiguous float32 [n] tensors on J's device");
  float* dp = nullptr;
  if (delta_out.has_value() && delta_out->defined()) {
    TORCH_CHECK(vec_ok(*delta_out), "delta_out must be a contiguous float32 [n] tensor on J's device");
    dp = delta_out->data_ptr<float>();
  }
  const int K = (int)rows;
  auto out = torch::empty({rows + rows * rows + 2}, J.options().dtype(at::kDouble));
  if (n == 0) return out.zero_();
  auto stream = at::hip::getCurrentHIPStream();
  const float* jp = J.data_ptr<float>();
  const int64_t ld = rows > 1 ? J.stride(0) : n;
  const float *dd = d.data_ptr<float>(), *lp = lo.data_ptr<float>(), *hp = hi.data_ptr<float>();
  const bool vec = box_vector_loads(jp, K, ld, dd, lp, hp, dp, n);
  const double* cp = coef.data_ptr<double>();
  double* op = out.data_ptr<double>();
  dispatch_row_tile<kBoxMaxRows>(K, [&](auto tile) {
    launch_box_dual<decltype(tile)::value>(jp, ld, K, cp, dd, lam, lp, hp, n, vec, dp, op, J, stream);
  });
  return out;
}

}  // namespace mg
