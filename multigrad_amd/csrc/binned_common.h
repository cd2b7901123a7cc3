// Device helpers shared by the Gaussian-binned-sum ops (binned.hip, binned_hvp.hip,
// binned_jvp.hip, binned2d.hip, binned_multi.hip, binned_group.hip, binned_fine.hip,
// binned_reduce.hip): the edge CDF, guarded vector loads and stores of per-object operands, the
// fixed-order slab column sum, the operands of the one-axis op, and the gradient outputs and
// epilogue of the object-parallel backward kernels.
#pragma once
#include "common.h"
#include "smf_device.h"

namespace mg {

constexpr int kBinThreads = 256;
constexpr int kRedThreads = 1024;
constexpr float kInvSqrt2PiB = 0x1.988454p-2f;  // 1/sqrt(2 pi)

inline bool aligned_to(const void* p, uintptr_t bytes) {
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}

// Phi(z) = base + frac with base in {0, 1} and |frac| = Q(|z|) <= 1/2: the difference of two
// edges on the same side of the mean is then formed from the small parts alone.  ws = z*kWScale.
__device__ __forceinline__ void edge_cdf(float z, float& base, float& frac, float& gauss) {
  float p;
  normal_tail_parts_w<false>(z * kWScale, p, gauss);
  const float q = p * gauss;
  const bool up = z >= 0.0f;
  base = up ? 1.0f : 0.0f;
  frac = up ? -q : q;
}

// V (2 or 4) consecutive elements p[i0 .. i0+V) of a per-object operand, read in groups: a
// full group of an aligned operand takes one 4*V-byte load (wide_load); a misaligned view
// and the last n % V elements take guarded scalar loads (guarded_load, never past the end;
// an element beyond n gives `fill`, a broadcast operand reads p[0]).
template <int V>
__device__ __forceinline__ void wide_load(const float* p, int64_t i0, float (&v)[V]) {
  static_assert(V == 2 || V == 4, "wide_load: 8- or 16-byte groups");
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + i0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    const float2 t = *reinterpret_cast<const float2*>(p + i0);
    v[0] = t.x; v[1] = t.y;
  }
}

template <int V>
__device__ __forceinline__ void guarded_load(const float* p, int64_t i0, int64_t n, bool bcast,
                                             float fill, float (&v)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j) v[j] = i0 + j < n ? p[bcast ? 0 : i0 + j] : fill;
}

template <int V>
__device__ __forceinline__ void splat(float x, float (&v)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j) v[j] = x;
}

// One operand of a group: `full` is "the group is whole and every operand is aligned"
// (the caller's single branch); a null pointer stands for the constant `fill_null`.
template <int V>
__device__ __forceinline__ void load_group(const float* p, int64_t i0, int64_t n, bool full,
                                           bool bcast, float fill_null, float fill_end,
                                           float (&v)[V]) {
  if (full) {
    if (p == nullptr) splat(fill_null, v);
    else if (bcast) splat(p[0], v);
    else wide_load<V>(p, i0, v);
  } else if (p == nullptr) {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = i0 + j < n ? fill_null : fill_end;
  } else {
    guarded_load<V>(p, i0, n, bcast, fill_end, v);
  }
}

// V consecutive results to p[i0 .. i0+V): one 4*V-byte store for a full group (p is a fresh
// allocation, hence aligned), guarded scalar stores for the last n % V elements.
template <int V>
__device__ __forceinline__ void store_group(float* p, int64_t i0, int64_t n, const float (&v)[V]) {
  static_assert(V == 2 || V == 4, "store_group: 8- or 16-byte groups");
  if (i0 + V <= n) {
    if constexpr (V == 4)
      *reinterpret_cast<float4*>(p + i0) = make_float4(v[0], v[1], v[2], v[3]);
    else
      *reinterpret_cast<float2*>(p + i0) = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (i0 + j < n) p[i0 + j] = v[j];
  }
}

// Fixed-order sum of `ncols` columns (a power of two <= 32) starting at column col0 of the
// slab rows [rows, ld], by one workgroup of kRedThreads threads: thread t owns column
// t % ncols and the rows t / ncols, + groups, ... (four independent partial sums, so four
// loads are in flight); the groups are then folded by a tree in LDS (part: kRedThreads
// floats).  The order depends only on (rows, ncols).  Threads [0, ncols) return true with the
// total of column col0 + threadIdx.x.
__device__ __forceinline__ bool slab_column_sum(const float* slab, int64_t rows, int64_t ld,
                                                int col0, int ncols, float* part, float& total) {
  const int k = threadIdx.x % ncols;
  const int64_t groups = kRedThreads / ncols;
  const float* col = slab + col0 + k;
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
  int64_t r = threadIdx.x / ncols;
  for (; r + 3 * groups < rows; r += 4 * groups) {
    s0 += col[r * ld];
    s1 += col[(r + groups) * ld];
    s2 += col[(r + 2 * groups) * ld];
    s3 += col[(r + 3 * groups) * ld];
  }
  for (; r < rows; r += groups) s0 += col[r * ld];
  part[threadIdx.x] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  for (int half = kRedThreads / 2; half >= ncols; half >>= 1) {
    if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
    __syncthreads();
  }
  total = part[threadIdx.x];
  return (int)threadIdx.x < ncols;
}

// The operands of the one-axis op (binned.hip, binned_hvp.hip).
struct BinnedArgs {
  const float* mu;
  const float* sigma;
  const float* w;  // nullptr: every weight is 1
  int64_t n;
  int nb;     // real bins (<= the padded template count)
  int sig_b;  // sigma has one element
  int w_b;    // w has one element
  int vec;    // every input pointer is 16-byte aligned
  float edge[kMaxBins + 1];
};

// Four consecutive objects of quad q: mean, 1/sigma and weight.  A full quad of aligned
// inputs is read with one 16-byte load per operand; a misaligned view and the last N % 4
// objects take guarded scalar loads (never past the end).  Objects beyond N get weight 0.
__device__ __forceinline__ void load_quad(const BinnedArgs& a, int64_t q, float (&m)[4],
                                          float (&inv)[4], float (&wt)[4]) {
  const int64_t i0 = q * 4;
  float s[4];
  if (a.vec && i0 + 4 <= a.n) {
    wide_load<4>(a.mu, i0, m);
    if (a.sig_b) splat(a.sigma[0], s);
    else wide_load<4>(a.sigma, i0, s);
    if (a.w == nullptr) splat(1.0f, wt);
    else if (a.w_b) splat(a.w[0], wt);
    else wide_load<4>(a.w, i0, wt);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = i0 + j;
      const bool ok = i < a.n;
      m[j] = ok ? a.mu[i] : 0.0f;
      s[j] = ok ? a.sigma[a.sig_b ? 0 : i] : 1.0f;
      wt[j] = !ok ? 0.0f : a.w == nullptr ? 1.0f : a.w[a.w_b ? 0 : i];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) inv[j] = 1.0f / s[j];
}

// The cotangent and the gradient outputs of an object-parallel backward over quads of objects
// (binned.hip, binned_group.hip, binned_fine.hip).
struct BinnedGrad {
  const float* g;  // the cotangent: [nb], or [G, nb] per group
  float* dmu;      // [n]
  float* dsigma;   // [n], or [1] when sigma is broadcast
  float* dw;       // [n], or [1] when w is broadcast
  float* slab;     // [blocks, 2] partial sums of the broadcast gradients (col 0 sigma, col 1 w)
};

// The gradient v of one operand for the quad at i0: a broadcast operand (`reduce`) adds the
// quad's sum to this thread's share, a per-object one stores the quad to dst.
__device__ __forceinline__ void put_quad(bool reduce, float& share, float* dst, int64_t i0,
                                         int64_t n, const float (&v)[4]) {
  if (reduce) share += (v[0] + v[1]) + (v[2] + v[3]);
  else store_group<4>(dst, i0, n, v);
}

// The end of such a kernel: the threads' shares rs of the broadcast gradients (0 sigma, 1 w)
// are summed over the workgroup (red: 2 floats per wave) and go to the outputs when one
// workgroup covers the input (`direct`), else to the workgroup's slab row.  red_sig / red_w
// are uniform over the grid.
__device__ __forceinline__ void finish_broadcast(float (&rs)[2], float* red, bool red_sig,
                                                 bool red_w, float* dsigma, float* dw, float* slab,
                                                 int direct) {
  if (!red_sig && !red_w) return;
  block_sum_n<2>(rs, red);
  if (threadIdx.x == 0) {
    if (direct) {
      if (red_sig) dsigma[0] = rs[0];
      if (red_w) dw[0] = rs[1];
    } else {
      slab[(int64_t)blockIdx.x * 2 + 0] = rs[0];
      slab[(int64_t)blockIdx.x * 2 + 1] = rs[1];
    }
  }
}

}  // namespace mg
