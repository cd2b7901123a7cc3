// Weighted Gram matrix of a short, wide matrix: out[k, l] = sum_p J[k, p] w[p] J[l, p]
// for J [K, n] float32 (K <= 256, n up to 1e8), float64 result.
//
// The dual (K x K) Gauss-Newton solve (optim/gauss_newton.py) needs W1 = J diag(1/d) J^T
// once per Jacobian.  torch's composite (J * w) @ J.T writes and re-reads a scaled copy of J
// and, in float32, loses the low bits the K x K Cholesky factorisation depends on; in
// float64 it converts the whole of J first.  Here J is streamed ONCE (K <= 16): every thread
// keeps the K (K + 1) / 2 float64 accumulators of the upper triangle in registers, converts
// its operands to float64 BEFORE any multiply (the product of two float32 is then exact,
// and the third factor enters by one fused multiply-add), and the per-thread sums are
// reduced in a fixed order: wave shuffles, LDS, one slab row per workgroup, and a final
// per-entry reduce kernel that also mirrors the lower triangle.  No atomics: the result is
// bitwise reproducible for a fixed n and device.  The reduce kernel's sum and the triangle
// decode are sweep_device.h's, the cap, the grid and the row-tile dispatch sweep_host.h's; the
// main kernel's loads and slab-row store are written out here (see the note in the kernel).
//
// K > 16 is tiled over pairs of 8-row blocks (grid.y, block pairs bi <= bj with a full
// 8 x 8 tile each), so J is re-read once per row block: (K / 8 + 1) / 2 passes per row.
//
// Loads are 16 bytes wide when the pointers, the row stride and n allow it (the last
// n % 4 columns by guarded scalar loads); otherwise every load is a guarded scalar load.
#include "sweep_device.h"
#include "sweep_host.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace mg {

constexpr int kGramThreads = 256;
constexpr int kGramMaxBlocks = 1024;  // slab rows of the single-tile kernels
constexpr int kGramTile = 8;          // row block of the tiled (K > 16) kernels
constexpr int kGramTiledBlocks = 4096;  // workgroups (slab rows) of a tiled launch
constexpr int kGramMaxRows = 256;

// Entries a tile keeps: the upper triangle of a T x T diagonal tile, or all of an
// off-diagonal one.
template <int T, bool FULL>
struct GramTile {
  static constexpr int kEntries = FULL ? T * T : T * (T + 1) / 2;
};

// One column group: G = 4 columns (one float4 per row) or 1 column.
template <int T, bool FULL, int G>
__device__ __forceinline__ void gram_accumulate(const float (&xi)[T][G], const float (&xj)[T][G],
                                                const float (&wv)[G],
                                                double (&acc)[GramTile<T, FULL>::kEntries]) {
#pragma unroll
  for (int q = 0; q < G; ++q) {
    const double wd = (double)wv[q];
    double dj[T];
#pragma unroll
    for (int b = 0; b < T; ++b) dj[b] = (double)xj[b][q];
    int e = 0;
#pragma unroll
    for (int a = 0; a < T; ++a) {
      const double t = (double)xi[a][q] * wd;  // exact: two 24-bit significands
#pragma unroll
      for (int b = FULL ? 0 : a; b < T; ++b) {
        acc[e] = fma(t, dj[b], acc[e]);
        ++e;
      }
    }
  }
}

// grid.x: column slices (grid-stride); grid.y: tile pairs (bi <= bj) of the nrb row blocks
// (FULL) or 1.  Row indices past K are clamped to the last row (their sums are never read).
template <int T, bool FULL, bool VEC>
__global__ __launch_bounds__(kGramThreads) void weighted_gram_kernel(
    const float* __restrict__ J, int64_t ld, int K, int nrb, const float* __restrict__ w,
    int64_t n, double* __restrict__ slab) {
  constexpr int NE = GramTile<T, FULL>::kEntries;
  int bi = 0, bj = 0;
  if constexpr (FULL) triangle_index(blockIdx.y, nrb, bi, bj);
  const float* ri[T];
  const float* rj[T];
#pragma unroll
  for (int a = 0; a < T; ++a) {
    ri[a] = J + (int64_t)min(bi * T + a, K - 1) * ld;
    rj[a] = J + (int64_t)min(bj * T + a, K - 1) * ld;
  }
  double acc[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) acc[e] = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * kGramThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kGramThreads;
  // The sweep and the slab-row store are written out (box_dual.hip uses sweep_device.h for
  // both): at T = 16 this kernel sits at the register limit, and any other spelling of them
  // changes its allocation.
  int64_t j0 = 0;
  if constexpr (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t j = tid; j < n4; j += stride) {
      float xi[T][4], xj[T][4], wv[4] = {1.0f, 1.0f, 1.0f, 1.0f};
      if (w) {
        const float4 v = reinterpret_cast<const float4*>(w)[j];
        wv[0] = v.x; wv[1] = v.y; wv[2] = v.z; wv[3] = v.w;
      }
#pragma unroll
      for (int a = 0; a < T; ++a) {
        const float4 v = reinterpret_cast<const float4*>(ri[a])[j];
        xi[a][0] = v.x; xi[a][1] = v.y; xi[a][2] = v.z; xi[a][3] = v.w;
      }
      if constexpr (FULL) {
#pragma unroll
        for (int a = 0; a < T; ++a) {
          const float4 v = reinterpret_cast<const float4*>(rj[a])[j];
          xj[a][0] = v.x; xj[a][1] = v.y; xj[a][2] = v.z; xj[a][3] = v.w;
        }
        gram_accumulate<T, FULL, 4>(xi, xj, wv, acc);
      } else {
        gram_accumulate<T, FULL, 4>(xi, xi, wv, acc);
      }
    }
    j0 = n4 << 2;
  }
  for (int64_t j = j0 + tid; j < n; j += stride) {
    float xi[T][1], xj[T][1], wv[1];
    wv[0] = w ? w[j] : 1.0f;
#pragma unroll
    for (int a = 0; a < T; ++a) xi[a][0] = ri[a][j];
    if constexpr (FULL) {
#pragma unroll
      for (int a = 0; a < T; ++a) xj[a][0] = rj[a][j];
      gram_accumulate<T, FULL, 1>(xi, xj, wv, acc);
    } else {
      gram_accumulate<T, FULL, 1>(xi, xi, wv, acc);
    }
  }
  double* out = slab + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * NE;
  __shared__ double scratch[8 * (kGramThreads / kWave)];
#pragma unroll
  for (int e0 = 0; e0 < NE; e0 += 8) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = e0 + q < NE ? acc[e0 + q] : 0.0;
    block_sum_n<8>(v, scratch);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (e0 + q < NE) out[e0 + q] = v[q];
    }
    __syncthreads();
  }
}

// One workgroup per slab entry (pair, e): the fixed-order sum over the bx slab rows, written
// to out[k, l] and mirrored to out[l, k].
__global__ __launch_bounds__(kGramThreads) void weighted_gram_reduce_kernel(
    const double* __restrict__ slab, int bx, int npairs, int ne, int T, int full, int nrb, int K,
    double* __restrict__ out) {
  const int pair = blockIdx.x / ne, e = blockIdx.x % ne;
  int bi = 0, bj = 0, a = 0, b = 0;
  if (full) {
    triangle_index(pair, nrb, bi, bj);
    a = e / T;
    b = e % T;
  } else {
    triangle_index(e, T, a, b);
  }
  const int k = bi * T + a, l = bj * T + b;
  if (k >= K || l >= K || k > l) return;  // uniform per workgroup
  const double s = slab_entry_sum<kGramThreads>(
      bx, [&](int r) { return slab[((int64_t)r * npairs + pair) * ne + e]; });
  if (threadIdx.x == 0) {
    out[(int64_t)k * K + l] = s;
    out[(int64_t)l * K + k] = s;
  }
}

template <int T, bool FULL>
static void launch_gram(const float* J, int64_t ld, int K, const float* w, int64_t n, bool vec,
                        double* out, const torch::Tensor& like, hipStream_t stream) {
  constexpr int NE = GramTile<T, FULL>::kEntries;
  auto kv = weighted_gram_kernel<T, FULL, true>;
  auto ks = weighted_gram_kernel<T, FULL, false>;
  static GridCap cap;  // of the 16-byte-load instantiation: one grid for both load paths
  const int nrb = FULL ? (K + T - 1) / T : 1;
  const int npairs = nrb * (nrb + 1) / 2;
  int64_t bx = chunk_grid(sweep_chunks(n, vec), kGramThreads,
                          resident_cap(cap, kGramMaxBlocks, kGramThreads, kv));
  if (FULL) bx = std::max<int64_t>(1, std::min<int64_t>(bx, kGramTiledBlocks / npairs));
  auto slab = torch::empty({bx * npairs * NE}, like.options().dtype(at::kDouble));
  double* sp = slab.data_ptr<double>();
  dim3 grid((unsigned)bx, (unsigned)npairs);
  hipLaunchKernelGGL(vec ? kv : ks, grid, dim3(kGramThreads), 0, stream, J, ld, K, nrb, w, n, sp);
  hipLaunchKernelGGL(weighted_gram_reduce_kernel, dim3(npairs * NE), dim3(kGramThreads), 0, stream,
                     sp, (int)bx, npairs, NE, T, FULL ? 1 : 0, nrb, K, out);
}

// J: [>= nrows, n] float32 with unit column stride; w: [n] float32 or none; returns
// [nrows, nrows] float64 on J's device.  Current stream, no host synchronisation.
torch::Tensor weighted_gram(torch::Tensor J, c10::optional<torch::Tensor> w, int64_t nrows) {
  TORCH_CHECK(J.is_cuda() && J.scalar_type() == at::kFloat, "J must be a float32 device tensor");
  TORCH_CHECK(J.dim() == 2 && (J.size(1) <= 1 || J.stride(1) == 1), "J must be row-major 2-d");
  TORCH_CHECK(nrows >= 1 && nrows <= kGramMaxRows && nrows <= J.size(0), "1 <= nrows <= 256 rows of J");
  const int64_t n = J.size(1);
  const float* wp = nullptr;
  if (w.has_value() && w->defined()) {
    TORCH_CHECK(w->is_cuda() && w->scalar_type() == at::kFloat && w->is_contiguous() &&
                    w->numel() == n && w->get_device() == J.get_device(),
                "w must be a contiguous float32 [n] tensor on J's device");
    wp = w->data_ptr<float>();
  }
  const int K = (int)nrows;
  auto out = torch::empty({nrows, nrows}, J.options().dtype(at::kDouble));
  if (n == 0) return out.zero_();
  auto stream = at::hip::getCurrentHIPStream();
  const float* jp = J.data_ptr<float>();
  const int64_t ld = J.size(0) > 1 ? J.stride(0) : n;
  const bool vec = aligned16(jp) && (K == 1 || ld % 4 == 0) && (!wp || aligned16(wp)) && n >= 4;
  double* op = out.data_ptr<double>();
  if (K <= 16)
    dispatch_row_tile<16>(K, [&](auto tile) {
      launch_gram<decltype(tile)::value, false>(jp, ld, K, wp, n, vec, op, J, stream);
    });
  else
    launch_gram<kGramTile, true>(jp, ld, K, wp, n, vec, op, J, stream);
  return out;
}

}  // namespace mg
