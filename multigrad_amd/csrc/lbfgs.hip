// Vector kernels for the device L-BFGS (SPMD, optionally sharded across ranks).
//
// Reference: multigrad/bfgs.py drives scipy's compiled L-BFGS-B on the root rank with
// two pickled broadcasts per function evaluation.  The device L-BFGS keeps the history
// (S, Y) on the GPU -- sharded 1/W per rank for 1e7-1e8 parameters -- and needs, per
// iteration, the 2m x 3 dot products [S; Y] . [s_new, y_new, g] (new row/column of
// S^T Y and Y^T Y plus S^T g, Y^T g for the compact inverse-Hessian product).  They are
// computed in ONE pass over the history by `multi_dot` (fp32 per-lane accumulation,
// fp64 fixed-order block and slab reductions: deterministic), and all-reduced across
// ranks as one device all-reduce (optim/_reduce.py: the wide one-shot peer-memory kernel,
// else RCCL).  The search direction d = -(gamma g + sum_i c_i H_i)
// is one fused pass (`lincomb`).  The slab-row store and the slab entry sum of `multi_dot` are
// sweep_device.h's; every launch takes its resident-workgroup cap and grid from sweep_host.h.
#include "sweep_device.h"
#include "sweep_host.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <vector>

namespace mg {

constexpr int kDotThreads = 256;
constexpr int kDotWaves = kDotThreads / kWave;
constexpr int kMaxCols = 4;    // right-hand vectors
constexpr int kDotMaxBlocks = 2048;

struct RowPtrs {
  const float* p[kMaxCols];
};

// SPLIT (>= 4 rows): the 4 waves of a workgroup take the same float4 chunks of the NC
// right-hand vectors and RPW rows each (wave w: rows r0 + w RPW ..), so a chunk of the
// vectors comes from HBM once and reaches the other waves from the caches, while each row
// is read once; about 60 VGPRs at 6 rows x 3 vectors (8 waves per SIMD).  (Round 4 had
// thread-private groups of 8 rows in separate workgroups, which re-read the vectors from
// HBM for every group: 4.0 TB/s at 23 rows x 3 vectors x 1e7.)
// Not SPLIT (1-3 rows): every thread takes all RPW rows of its own chunks.
// Row indices past nrows are clamped to the last row (their sums are never read), so the
// loads of a chunk carry no branches and are all in flight before the FMAs.  fp32 partial
// sums per lane, then fp64 reductions in a fixed order (wave shuffles, LDS, the per-output
// reduce kernel): deterministic.
template <int NC, int RPW, bool SPLIT, bool VEC>
__global__ __launch_bounds__(kDotThreads) void multi_dot_kernel(
    const float* __restrict__ A, int64_t lda, int nrows, RowPtrs B, int64_t n,
    double* __restrict__ partial) {
  constexpr int RB = SPLIT ? kDotWaves * RPW : RPW;  // rows per workgroup
  constexpr int TPB = SPLIT ? kWave : kDotThreads;    // threads per chunk set
  const int wid = threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  const int r0 = blockIdx.y * RB + (SPLIT ? wid * RPW : 0);
  const float* rows[RPW];
#pragma unroll
  for (int i = 0; i < RPW; ++i) rows[i] = A + (int64_t)min(r0 + i, nrows - 1) * lda;
  float acc[RPW][NC];
#pragma unroll
  for (int i = 0; i < RPW; ++i)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[i][c] = 0.0f;
  const int64_t tid = (int64_t)blockIdx.x * TPB + (SPLIT ? lane : (int)threadIdx.x);
  const int64_t stride = (int64_t)gridDim.x * TPB;
  int64_t j0 = 0;
  if constexpr (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t j = tid; j < n4; j += stride) {
      float4 b[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) b[c] = reinterpret_cast<const float4*>(B.p[c])[j];
      float4 a[RPW];
#pragma unroll
      for (int i = 0; i < RPW; ++i) a[i] = reinterpret_cast<const float4*>(rows[i])[j];
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          float t = acc[i][c];
          t = fmaf(a[i].x, b[c].x, t);
          t = fmaf(a[i].y, b[c].y, t);
          t = fmaf(a[i].z, b[c].z, t);
          t = fmaf(a[i].w, b[c].w, t);
          acc[i][c] = t;
        }
      }
    }
    j0 = n4 << 2;
  }
  for (int64_t j = j0 + tid; j < n; j += stride) {
    float b[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) b[c] = B.p[c][j];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const float a = rows[i][j];
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[i][c] = fmaf(a, b[c], acc[i][c]);
    }
  }
  constexpr int K = RPW * NC;
  double* out = partial + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * RB * NC;
  if constexpr (SPLIT) {
    // each wave owns its rows: wave reductions, lane 0 writes
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double v = wave_sum((double)acc[k / NC][k % NC]);
      if (lane == 0) out[wid * K + k] = v;
    }
  } else {
    slab_row_store<kDotThreads>(out, acc);
  }
}

// out[r, c] = sum over the column blocks of the partials: one workgroup per output, each
// thread a fixed strided subset, then the fixed shuffle/LDS tree -> deterministic.  (One
// thread per output walking all 1024 partials took 193 us per call.)
__global__ __launch_bounds__(kDotThreads) void multi_dot_reduce_kernel(
    const double* __restrict__ partial, int nblk_x, int ngroups, int rb, int nc,
    double* __restrict__ out) {
  const int t = blockIdx.x;
  const int r = t / nc, c = t % nc;
  const int g = r / rb, i = r % rb;
  const double s = slab_entry_sum<kDotThreads>(nblk_x, [&](int b) {
    return partial[((int64_t)b * ngroups + g) * rb * nc + i * nc + c];
  });
  if (threadIdx.x == 0) out[t] = s;
}

// y = alpha * x + sum_i coef[i] * H[i, :]   (coef in device memory, nrows <= kLincombRows)
constexpr int kLincombRows = 256;
__global__ __launch_bounds__(256) void lincomb_kernel(const float* __restrict__ H, int64_t ldh,
                                                      int nrows, const float* __restrict__ coef,
                                                      float alpha, const float* __restrict__ x,
                                                      int64_t n, float* __restrict__ y) {
  __shared__ float c[kLincombRows];
  for (int i = threadIdx.x; i < nrows; i += blockDim.x) c[i] = coef[i];
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    float acc = x ? alpha * x[j] : 0.0f;
    for (int i = 0; i < nrows; ++i) acc = fmaf(c[i], H[(int64_t)i * ldh + j], acc);
    y[j] = acc;
  }
}

// rows per wave (SPLIT, >= 4 rows) or per thread (1-3 rows)
static int dot_rpw(int64_t nrows) {
  if (nrows < kDotWaves) return (int)nrows;
  const int64_t per = (nrows + kDotWaves - 1) / kDotWaves;
  return per <= 2 ? 2 : (per <= 4 ? 4 : (per <= 6 ? 6 : 8));
}
static int dot_rows_per_block(int64_t nrows) {
  return nrows < kDotWaves ? (int)nrows : kDotWaves * dot_rpw(nrows);
}

// Grid: the chunk count, capped at what the GPU holds resident at once (the occupancy of
// the instantiation times the CU count), so no workgroup starts after the first wave of
// workgroups has finished (a grid-stride loop with a late tail).
template <int NC, int RPW, bool SPLIT>
static void launch_dot(int64_t n, int gy, hipStream_t stream, bool vec, const float* a, int64_t lda,
                       int nrows, const RowPtrs& rp, double* ws, int* bx_out) {
  auto kv = multi_dot_kernel<NC, RPW, SPLIT, true>;
  auto ks = multi_dot_kernel<NC, RPW, SPLIT, false>;
  static GridCap cap;  // of the 16-byte-load instantiation: one grid for both load paths
  const int bx = chunk_grid(vec ? (n >> 2) : n, SPLIT ? kWave : kDotThreads,
                            resident_cap(cap, kDotMaxBlocks, kDotThreads, kv));
  *bx_out = bx;
  dim3 grid(bx, gy);
  hipLaunchKernelGGL(vec ? kv : ks, grid, dim3(kDotThreads), 0, stream, a, lda, nrows, rp, n, ws);
}

template <int NC>
static void launch_dot_nc(int64_t nrows, int64_t n, int gy, hipStream_t stream, bool vec,
                          const float* a, int64_t lda, const RowPtrs& rp, double* ws, int* bx) {
  const int r = (int)nrows;
  switch (dot_rpw(nrows) + (nrows < kDotWaves ? 100 : 0)) {
    case 101: launch_dot<NC, 1, false>(n, gy, stream, vec, a, lda, r, rp, ws, bx); break;
    case 102: launch_dot<NC, 2, false>(n, gy, stream, vec, a, lda, r, rp, ws, bx); break;
    case 103: launch_dot<NC, 3, false>(n, gy, stream, vec, a, lda, r, rp, ws, bx); break;
    case 2: launch_dot<NC, 2, true>(n, gy, stream, vec, a, lda, r, rp, ws, bx); break;
    case 4: launch_dot<NC, 4, true>(n, gy, stream, vec, a, lda, r, rp, ws, bx); break;
    case 6: launch_dot<NC, 6, true>(n, gy, stream, vec, a, lda, r, rp, ws, bx); break;
    default: launch_dot<NC, 8, true>(n, gy, stream, vec, a, lda, r, rp, ws, bx); break;
  }
}

// A: [nrows, lda] row-major rows; B: list of nc (<= 4) vectors; out [nrows, nc] fp64.
void multi_dot(torch::Tensor A, int64_t nrows, std::vector<torch::Tensor> B, int64_t n,
               torch::Tensor out, torch::Tensor workspace) {
  const int64_t nc = (int64_t)B.size();
  TORCH_CHECK(A.is_cuda() && out.is_cuda() && workspace.is_cuda(), "device tensors");
  TORCH_CHECK(A.scalar_type() == at::kFloat, "fp32 vectors");
  TORCH_CHECK(out.scalar_type() == at::kDouble && workspace.scalar_type() == at::kDouble, "fp64 out");
  TORCH_CHECK(A.dim() == 2 && A.stride(1) == 1, "A must be row-major 2-d");
  TORCH_CHECK(nrows >= 1 && nrows <= A.size(0) && nc >= 1 && nc <= kMaxCols, "bad shape");
  TORCH_CHECK(n >= 0 && n <= A.size(1), "n must be in 0..A.size(1)");
  TORCH_CHECK(out.numel() >= nrows * nc, "out too small");
  RowPtrs rp;
  for (int c = 0; c < kMaxCols; ++c) rp.p[c] = nullptr;
  for (int64_t c = 0; c < nc; ++c) {
    TORCH_CHECK(B[c].is_cuda() && B[c].scalar_type() == at::kFloat && B[c].is_contiguous() &&
                B[c].numel() >= n, "B vectors: contiguous fp32 device, >= n");
    rp.p[c] = B[c].data_ptr<float>();
  }
  const int rb = dot_rows_per_block(nrows);
  const int gy = (int)((nrows + rb - 1) / rb);
  TORCH_CHECK(workspace.numel() >= (int64_t)kDotMaxBlocks * gy * rb * nc, "workspace too small");
  auto stream = at::hip::getCurrentHIPStream();
  const float* a = A.data_ptr<float>();
  double* ws = workspace.data_ptr<double>();
  bool vec = aligned16(a) && A.stride(0) % 4 == 0;
  for (int64_t c = 0; c < nc; ++c) vec = vec && aligned16(rp.p[c]);
  int bx = 1;
  const int64_t lda = A.stride(0);
  switch (nc) {
    case 1: launch_dot_nc<1>(nrows, n, gy, stream, vec, a, lda, rp, ws, &bx); break;
    case 2: launch_dot_nc<2>(nrows, n, gy, stream, vec, a, lda, rp, ws, &bx); break;
    case 3: launch_dot_nc<3>(nrows, n, gy, stream, vec, a, lda, rp, ws, &bx); break;
    default: launch_dot_nc<4>(nrows, n, gy, stream, vec, a, lda, rp, ws, &bx); break;
  }
  const int tot = (int)(nrows * nc);
  hipLaunchKernelGGL(multi_dot_reduce_kernel, dim3(tot), dim3(kDotThreads), 0, stream, ws, bx, gy,
                     rb, (int)nc, out.data_ptr<double>());
}

int64_t multi_dot_workspace(int64_t nrows, int64_t n) {
  // any call with at most nrows rows fits (rows per block * groups grows with nrows)
  int64_t most = 0;
  for (int64_t r = 1; r <= nrows; ++r) {
    const int64_t rb = dot_rows_per_block(r);
    most = std::max(most, ((r + rb - 1) / rb) * rb);
  }
  (void)n;
  return (int64_t)kDotMaxBlocks * most * kMaxCols;
}

void lincomb(torch::Tensor H, int64_t nrows, torch::Tensor coef, double alpha,
             c10::optional<torch::Tensor> x, int64_t n, torch::Tensor y) {
  TORCH_CHECK(H.is_cuda() && coef.is_cuda() && y.is_cuda(), "device tensors");
  TORCH_CHECK(H.scalar_type() == at::kFloat && coef.scalar_type() == at::kFloat &&
              y.scalar_type() == at::kFloat, "fp32");
  TORCH_CHECK(n >= 0 && nrows >= 0, "bad sizes");
  TORCH_CHECK(H.dim() == 2 && H.stride(1) == 1 && nrows <= H.size(0) && nrows <= kLincombRows &&
              coef.numel() >= nrows && n <= H.size(1) && y.numel() >= n, "bad shapes");
  TORCH_CHECK(coef.is_contiguous() && y.is_contiguous(), "coef, y must be contiguous");
  const float* xp = nullptr;
  if (x.has_value() && x->defined()) {
    TORCH_CHECK(x->is_cuda() && x->scalar_type() == at::kFloat && x->is_contiguous() &&
                x->numel() >= n, "x: contiguous fp32 device vector, >= n");
    xp = x->data_ptr<float>();
  }
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048));
  hipLaunchKernelGGL(lincomb_kernel, dim3(blocks), dim3(256), 0, stream, H.data_ptr<float>(),
                     H.stride(0), (int)nrows, coef.data_ptr<float>(), (float)alpha, xp, n,
                     y.data_ptr<float>());
}

// ---------------------------------------------------------------------------------------
// Kernels of the inverse-Hessian operator a device L-BFGS run returns (optim/invhess.py).
//
// lincomb_cols: Y_c[j] = post[j] * (alpha * X_c[j] * pre[j] + sum_i coef[i, c] * H[i, j]) for
// c < NC <= 4 columns in ONE pass over the rows of H (`lincomb` would read the history once
// per column).  Per element and column the order is fixed: the alpha * x term first, then
// rows 0 .. nrows-1 by fmaf -- bitwise reproducible for every grid, vector width and NC.
struct ColPtrs {
  const float* x;  // [NC, ldx] or null
  float* y;        // [NC, ldy]
  int64_t ldx, ldy;
};

template <int NC, int VW>
__device__ __forceinline__ void lincomb_cols_span(
    const float* __restrict__ H, int64_t ldh, int nrows, const float* c, float alpha,
    const ColPtrs& cp, const float* __restrict__ pre, const float* __restrict__ post,
    int64_t j0, int64_t count, int64_t tid, int64_t stride) {
  using V = typename std::conditional<VW == 4, float4, float>::type;
  for (int64_t j = tid; j < count; j += stride) {
    const int64_t off = j0 + j * VW;
    float acc[NC][VW];
    if (cp.x != nullptr) {
      float p[VW];
      if (pre != nullptr) {
        const V pv = *reinterpret_cast<const V*>(pre + off);
#pragma unroll
        for (int e = 0; e < VW; ++e) p[e] = reinterpret_cast<const float*>(&pv)[e];
      }
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const V xv = *reinterpret_cast<const V*>(cp.x + k * cp.ldx + off);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          const float ax = alpha * reinterpret_cast<const float*>(&xv)[e];
          acc[k][e] = pre != nullptr ? ax * p[e] : ax;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < NC; ++k)
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[k][e] = 0.0f;
    }
#pragma unroll 4
    for (int i = 0; i < nrows; ++i) {
      const V hv = *reinterpret_cast<const V*>(H + (int64_t)i * ldh + off);
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const float ck = c[i * NC + k];
#pragma unroll
        for (int e = 0; e < VW; ++e)
          acc[k][e] = fmaf(ck, reinterpret_cast<const float*>(&hv)[e], acc[k][e]);
      }
    }
    if (post != nullptr) {
      const V qv = *reinterpret_cast<const V*>(post + off);
#pragma unroll
      for (int k = 0; k < NC; ++k)
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[k][e] *= reinterpret_cast<const float*>(&qv)[e];
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      V out;
#pragma unroll
      for (int e = 0; e < VW; ++e) reinterpret_cast<float*>(&out)[e] = acc[k][e];
      *reinterpret_cast<V*>(cp.y + k * cp.ldy + off) = out;
    }
  }
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void lincomb_cols_kernel(
    const float* __restrict__ H, int64_t ldh, int nrows, const float* __restrict__ coef,
    float alpha, ColPtrs cp, const float* __restrict__ pre, const float* __restrict__ post,
    int64_t n) {
  __shared__ float c[kLincombRows * NC];
  for (int i = threadIdx.x; i < nrows * NC; i += blockDim.x) c[i] = coef[i];
  __syncthreads();
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t j0 = 0;
  if constexpr (VEC) {
    lincomb_cols_span<NC, 4>(H, ldh, nrows, c, alpha, cp, pre, post, 0, n >> 2, tid, stride);
    j0 = (n >> 2) << 2;
  }
  lincomb_cols_span<NC, 1>(H, ldh, nrows, c, alpha, cp, pre, post, j0, n - j0, tid, stride);
}

// Grid of a streaming pass: the chunk count capped at what the GPU holds resident at once
// (as launch_dot), the rest by the grid-stride loop.  The cap is that of the instantiation
// that is launched (the float4 and the scalar kernels differ in registers).
template <typename K>
static int stream_grid(int64_t n, bool vec, K kernel, GridCap& cap) {
  return chunk_grid(sweep_chunks(n, vec), 256, resident_cap(cap, kDotMaxBlocks, 256, kernel));
}

template <int NC>
static void launch_lincomb_cols(bool vec, hipStream_t stream, const float* H, int64_t ldh,
                                int nrows, const float* coef, float alpha, const ColPtrs& cp,
                                const float* pre, const float* post, int64_t n) {
  static GridCap cap_v, cap_s;
  auto kv = lincomb_cols_kernel<NC, true>;
  auto ks = lincomb_cols_kernel<NC, false>;
  const int blocks = vec ? stream_grid(n, true, kv, cap_v) : stream_grid(n, false, ks, cap_s);
  hipLaunchKernelGGL(vec ? kv : ks, dim3(blocks), dim3(256), 0, stream, H, ldh, nrows, coef,
                     alpha, cp, pre, post, n);
}

static const float* opt_vec(const c10::optional<torch::Tensor>& t, int64_t n, const char* what) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() &&
              t->numel() >= n, what, ": contiguous fp32 device vector, >= n");
  return t->data_ptr<float>();
}

// H: [>= nrows, ldh]; coef: [nrows, nc] fp32 (device); x: [nc, >= n] or none; y: [nc, >= n].
void lincomb_cols(torch::Tensor H, int64_t nrows, torch::Tensor coef, double alpha,
                  c10::optional<torch::Tensor> x, c10::optional<torch::Tensor> pre,
                  c10::optional<torch::Tensor> post, int64_t n, torch::Tensor y) {
  TORCH_CHECK(H.is_cuda() && coef.is_cuda() && y.is_cuda(), "device tensors");
  TORCH_CHECK(H.scalar_type() == at::kFloat && coef.scalar_type() == at::kFloat &&
              y.scalar_type() == at::kFloat, "fp32");
  TORCH_CHECK(y.dim() == 2 && y.stride(1) == 1 && y.size(1) >= n, "y must be [nc, >= n]");
  const int64_t nc = y.size(0);
  TORCH_CHECK(nc >= 1 && nc <= kMaxCols, "1..4 columns");
  TORCH_CHECK(n >= 0 && nrows >= 0 && nrows <= kLincombRows, "bad sizes");
  TORCH_CHECK(H.dim() == 2 && H.stride(1) == 1 && nrows <= H.size(0) && n <= H.size(1),
              "H must be row-major [>= nrows, >= n]");
  TORCH_CHECK(coef.is_contiguous() && coef.numel() >= nrows * nc, "coef must be [nrows, nc]");
  if (n == 0) return;
  ColPtrs cp;
  cp.x = nullptr;
  cp.ldx = 0;
  cp.y = y.data_ptr<float>();
  cp.ldy = y.stride(0);
  if (x.has_value() && x->defined()) {
    TORCH_CHECK(x->is_cuda() && x->scalar_type() == at::kFloat && x->dim() == 2 &&
                x->size(0) == nc && x->stride(1) == 1 && x->size(1) >= n, "x must be [nc, >= n]");
    cp.x = x->data_ptr<float>();
    cp.ldx = x->stride(0);
  }
  const float* prep = opt_vec(pre, n, "pre");
  const float* postp = opt_vec(post, n, "post");
  const float* h = H.data_ptr<float>();
  bool vec = aligned16(h) && H.stride(0) % 4 == 0 && aligned16(cp.y) && (nc == 1 || cp.ldy % 4 == 0);
  if (cp.x) vec = vec && aligned16(cp.x) && (nc == 1 || cp.ldx % 4 == 0);
  if (prep) vec = vec && aligned16(prep);
  if (postp) vec = vec && aligned16(postp);
  auto stream = at::hip::getCurrentHIPStream();
  const float* cf = coef.data_ptr<float>();
  const int r = (int)nrows;
  const float a = (float)alpha;
  switch (nc) {
    case 1: launch_lincomb_cols<1>(vec, stream, h, H.stride(0), r, cf, a, cp, prep, postp, n); break;
    case 2: launch_lincomb_cols<2>(vec, stream, h, H.stride(0), r, cf, a, cp, prep, postp, n); break;
    case 3: launch_lincomb_cols<3>(vec, stream, h, H.stride(0), r, cf, a, cp, prep, postp, n); break;
    default: launch_lincomb_cols<4>(vec, stream, h, H.stride(0), r, cf, a, cp, prep, postp, n); break;
  }
}

// compact_diag: out[j] = (h0 + sum_{a,b} W[a,j] Q[a,b] W[b,j]) * scale[j]^2, the diagonal of
// the compact L-BFGS inverse Hessian, with W[a, :] = fac[a] * H[rows[a], :] and a symmetric
// Q [k2, k2].  Only the upper triangle of Q is used, off-diagonal entries doubled (exact):
//   out = h0 + sum_a w_a (Q_aa w_a + sum_{b > a} 2 Q_ab w_b),
// k2 (k2 + 1) / 2 terms in a fixed order.
//
// k2 <= 40 (`compact_diag_reg_kernel`): the k2 row values of a float4 of elements stay in
// registers, each history row is read once; Q sits in LDS, zero-padded to NR x NR so the
// unrolled loops need no bounds (a padded term is fmaf(0, 0, acc) = acc, exact).
template <int NR, int VW>
__device__ __forceinline__ void compact_diag_span(
    const float* __restrict__ H, int64_t ldh, const int* r, const float* f, const float* q,
    int k2, float h0, const float* __restrict__ scale, float* __restrict__ out, int64_t j0,
    int64_t count, int64_t tid, int64_t stride) {
  using V = typename std::conditional<VW == 4, float4, float>::type;
  for (int64_t j = tid; j < count; j += stride) {
    const int64_t off = j0 + j * VW;
    float w[NR][VW];
#pragma unroll
    for (int a = 0; a < NR; ++a) {
      if (a < k2) {
        const V hv = *reinterpret_cast<const V*>(H + (int64_t)r[a] * ldh + off);
#pragma unroll
        for (int e = 0; e < VW; ++e) w[a][e] = f[a] * reinterpret_cast<const float*>(&hv)[e];
      } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) w[a][e] = 0.0f;
      }
    }
    float acc[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[e] = h0;
    // Q is read from LDS where it is used: an offset the compiler cannot see through keeps it
    // from hoisting all NR (NR + 1) / 2 loop-invariant reads into registers (spills)
    int z = 0;
    asm volatile("" : "+s"(z));
    const float* qz = q + z;
#pragma unroll
    for (int a = 0; a < NR; ++a) {
      if (a < k2) {
        float u[VW];
        const float qaa = qz[a * NR + a];
#pragma unroll
        for (int e = 0; e < VW; ++e) u[e] = qaa * w[a][e];
#pragma unroll
        for (int b = a + 1; b < NR; ++b) {
          const float qab = qz[a * NR + b];
#pragma unroll
          for (int e = 0; e < VW; ++e) u[e] = fmaf(qab, w[b][e], u[e]);
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] = fmaf(w[a][e], u[e], acc[e]);
      }
    }
    if (scale != nullptr) {
      const V sv = *reinterpret_cast<const V*>(scale + off);
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        const float s = reinterpret_cast<const float*>(&sv)[e];
        acc[e] *= s * s;
      }
    }
    V o;
#pragma unroll
    for (int e = 0; e < VW; ++e) reinterpret_cast<float*>(&o)[e] = acc[e];
    *reinterpret_cast<V*>(out + off) = o;
  }
}

template <int NR, bool VEC>
__global__ __launch_bounds__(256, NR <= 20 ? 4 : 2) void compact_diag_reg_kernel(
    const float* __restrict__ H, int64_t ldh, const int* __restrict__ rows,
    const float* __restrict__ fac, const float* __restrict__ Q, int k2, int hrows, float h0,
    const float* __restrict__ scale, int64_t n, float* __restrict__ out) {
  __shared__ float q[NR * NR];
  __shared__ float f[NR];
  __shared__ int r[NR];
  for (int t = threadIdx.x; t < NR * NR; t += blockDim.x) {
    const int a = t / NR, b = t % NR;
    float v = 0.0f;
    if (a < k2 && b < k2 && a <= b) v = (a == b ? 1.0f : 2.0f) * Q[a * k2 + b];
    q[t] = v;
  }
  for (int t = threadIdx.x; t < NR; t += blockDim.x) {
    f[t] = t < k2 ? fac[t] : 0.0f;
    r[t] = t < k2 ? min(max(rows[t], 0), hrows - 1) : 0;  // never outside H
  }
  __syncthreads();
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t j0 = 0;
  if constexpr (VEC) {
    compact_diag_span<NR, 4>(H, ldh, r, f, q, k2, h0, scale, out, 0, n >> 2, tid, stride);
    j0 = (n >> 2) << 2;
  }
  compact_diag_span<NR, 1>(H, ldh, r, f, q, k2, h0, scale, out, j0, n - j0, tid, stride);
}

// k2 > 40 (`compact_diag_tiled_kernel`): columns b of Q are taken in strips of kDiagStrip
// (one LDS staging of Q[:, strip] each; 240 x 32 floats = 30 KB), inside a strip in tiles
// of kDiagTile rows whose values stay in registers while rows a <= b are re-read (from the
// caches):  out += sum_{b in tile} sum_{a <= b} w_a (m_ab Q_ab) w_b.  The running sum of an
// element passes through `out` between strips (always by the same thread).
constexpr int kDiagStrip = 32;
constexpr int kDiagTile = 8;
constexpr int kDiagMaxRows = 240;

__global__ __launch_bounds__(256) void compact_diag_tiled_kernel(
    const float* __restrict__ H, int64_t ldh, const int* __restrict__ rows,
    const float* __restrict__ fac, const float* __restrict__ Q, int k2, int hrows, float h0,
    const float* __restrict__ scale, int64_t n, float* __restrict__ out) {
  __shared__ float q[kDiagMaxRows * kDiagStrip];
  __shared__ float f[kDiagMaxRows];
  __shared__ int r[kDiagMaxRows];
  for (int t = threadIdx.x; t < k2; t += blockDim.x) {
    f[t] = fac[t];
    r[t] = min(max(rows[t], 0), hrows - 1);  // never outside H
  }
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int s0 = 0; s0 < k2; s0 += kDiagStrip) {
    __syncthreads();  // the previous strip's readers are done
    for (int t = threadIdx.x; t < k2 * kDiagStrip; t += blockDim.x) {
      const int a = t / kDiagStrip, b = s0 + t % kDiagStrip;
      float v = 0.0f;
      if (b < k2 && a <= b) v = (a == b ? 1.0f : 2.0f) * Q[a * k2 + b];
      q[t] = v;
    }
    __syncthreads();
    const bool last = s0 + kDiagStrip >= k2;
    for (int64_t j = tid; j < n; j += stride) {
      float acc = s0 == 0 ? h0 : out[j];
      for (int b0 = s0; b0 < min(s0 + kDiagStrip, k2); b0 += kDiagTile) {
        float wb[kDiagTile];
#pragma unroll
        for (int i = 0; i < kDiagTile; ++i)
          wb[i] = b0 + i < k2 ? f[b0 + i] * H[(int64_t)r[b0 + i] * ldh + j] : 0.0f;
        const int a_end = min(b0 + kDiagTile, k2);
        for (int a = 0; a < a_end; ++a) {
          const float wa = f[a] * H[(int64_t)r[a] * ldh + j];
          const float* qa = q + a * kDiagStrip + (b0 - s0);
          float u = qa[0] * wb[0];
#pragma unroll
          for (int i = 1; i < kDiagTile; ++i) u = fmaf(qa[i], wb[i], u);
          acc = fmaf(wa, u, acc);
        }
      }
      if (last && scale != nullptr) {
        const float s = scale[j];
        acc *= s * s;
      }
      out[j] = acc;
    }
  }
}

template <int NR>
static void launch_diag_reg(bool vec, hipStream_t stream, const float* H, int64_t ldh,
                            const int* rows, const float* fac, const float* Q, int k2, int hrows,
                            float h0, const float* scale, int64_t n, float* out) {
  static GridCap cap_v, cap_s;
  auto kv = compact_diag_reg_kernel<NR, true>;
  auto ks = compact_diag_reg_kernel<NR, false>;
  const int blocks = vec ? stream_grid(n, true, kv, cap_v) : stream_grid(n, false, ks, cap_s);
  hipLaunchKernelGGL(vec ? kv : ks, dim3(blocks), dim3(256), 0, stream, H, ldh, rows, fac, Q, k2,
                     hrows, h0, scale, n, out);
}

// H: [R, ldh] history; rows: [k2] int32 row of H per row of W; fac: [k2] fp32 factor per row;
// Q: [k2, k2] fp32 symmetric (device); scale: [>= n] or none; out: [>= n].
void compact_diag(torch::Tensor H, torch::Tensor rows, torch::Tensor fac, torch::Tensor Q,
                  double h0, c10::optional<torch::Tensor> scale, int64_t n, torch::Tensor out) {
  TORCH_CHECK(H.is_cuda() && rows.is_cuda() && fac.is_cuda() && Q.is_cuda() && out.is_cuda(),
              "device tensors");
  TORCH_CHECK(H.scalar_type() == at::kFloat && fac.scalar_type() == at::kFloat &&
              Q.scalar_type() == at::kFloat && out.scalar_type() == at::kFloat, "fp32");
  TORCH_CHECK(rows.scalar_type() == at::kInt && rows.is_contiguous(), "rows must be int32");
  const int64_t k2 = rows.numel();
  TORCH_CHECK(k2 >= 1 && k2 <= kDiagMaxRows, "1..240 rows of W");
  TORCH_CHECK(fac.is_contiguous() && fac.numel() == k2 && Q.is_contiguous() && Q.dim() == 2 &&
              Q.size(0) == k2 && Q.size(1) == k2, "fac [k2], Q [k2, k2]");
  TORCH_CHECK(H.dim() == 2 && H.stride(1) == 1 && n >= 0 && n <= H.size(1), "H row-major, n <= cols");
  TORCH_CHECK(out.is_contiguous() && out.numel() >= n, "out too small");
  if (n == 0) return;
  const float* sp = opt_vec(scale, n, "scale");
  const float* h = H.data_ptr<float>();
  float* o = out.data_ptr<float>();
  bool vec = aligned16(h) && H.stride(0) % 4 == 0 && aligned16(o) && (!sp || aligned16(sp));
  auto stream = at::hip::getCurrentHIPStream();
  const int* rp = rows.data_ptr<int>();
  const float* fp = fac.data_ptr<float>();
  const float* qp = Q.data_ptr<float>();
  const int k = (int)k2;
  const float h0f = (float)h0;
  const int hr = (int)H.size(0);
  if (k2 <= 8) {
    launch_diag_reg<8>(vec, stream, h, H.stride(0), rp, fp, qp, k, hr, h0f, sp, n, o);
  } else if (k2 <= 20) {
    launch_diag_reg<20>(vec, stream, h, H.stride(0), rp, fp, qp, k, hr, h0f, sp, n, o);
  } else if (k2 <= 40) {
    launch_diag_reg<40>(vec, stream, h, H.stride(0), rp, fp, qp, k, hr, h0f, sp, n, o);
  } else {
    static GridCap cap;
    const int blocks = stream_grid(n, false, compact_diag_tiled_kernel, cap);
    hipLaunchKernelGGL(compact_diag_tiled_kernel, dim3(blocks), dim3(256), 0, stream, h,
                       H.stride(0), rp, fp, qp, k, hr, h0f, sp, n, o);
  }
}

}  // namespace mg
