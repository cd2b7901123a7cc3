// Per-group Gaussian-binned sum on a GroupIndex plan (ops/binned_group.py):
//   out[g, k] = sum_{i : id_i = g} w_i * (Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i))
// the reduce-by-key of groups.hip with the binning of binned.hip fused in front of it, so that
// the [N, nb] table of bin masses is never written.
//
// Forward : over the plan's sorted positions (operands read through perm when the plan has
//           one).  One workgroup per chunk of kChunk = 1024 positions, four per thread.  The
//           head / tail flags of the runs and the structure of the lane and wave scans (which
//           additions happen) depend on the keys alone and are computed once per chunk; the
//           kernel then walks the edges as binned.hip does and, for every bin, forms the four
//           w * dPhi values of the thread and runs the segmented scan of that one column: the
//           thread's four entries, 64 lanes, the wave aggregates in LDS (double buffered: one
//           barrier per column).  Register use does not depend on nb.  A run inside the chunk
//           is stored to out[g, k]; a run that crosses a chunk edge leaves a partial in the
//           chunk's two carry slots, with the conventions of groups.hip (2c: the run entering
//           from the left, 2c + 1: the run leaving to the right).  At level 0, where
//           the keys are sorted, a full chunk whose first and last key are equal holds one
//           key (workgroup-uniform test; every chunk but a few when groups are large) and
//           skips the scan: (v0 + v1) + (v2 + v3), a wave butterfly, four wave totals.  The carry list (keys and nb value columns, equal keys adjacent) is
//           reduced by the same kernel reading its values from memory, level after level until
//           one chunk remains; a carry list has unused slots (key -1) between its keys, so the
//           carry levels always take the scan.
// Backward: per object in the original order, recomputing from mu / sigma / w (no residuals);
//           the cotangent row of object i is read from the [G, nb] table through ids[i] while
//           the edges are walked.  Per-object gradients are stored 16 bytes at a time;
//           gradients of broadcast operands go block sum -> slab -> fixed-order reduce.
// No float atomics and no data-dependent order: bitwise reproducible for a fixed plan, shapes
// and device.  Groups without objects keep the 0 of the zero-filled output.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <tuple>
#include <vector>

#include "binned_host.h"

namespace mg {

namespace {

constexpr int kGbThreads = 256;
constexpr int kGbChunk = kGbThreads * 4;  // sorted positions per chunk (groups.hip: kChunk)
constexpr int kGbWaves = kGbThreads / kWave;
constexpr int kGbNone = -1;  // an unused carry slot
constexpr int kGbPast = -2;  // a position beyond the list
constexpr int kGbEdge = -3;  // the neighbour of the first / last entry

struct GroupFwdArgs {
  const int* key;    // [m] keys with equal keys adjacent; negative keys are never stored
  const int* perm;   // level 0 of a permuted plan: position j is object perm[j]; else nullptr
  const float* mu;   // level 0: the operands of the binning
  const float* sigma;
  const float* w;    // nullptr: every weight is 1
  const float* x;    // upper levels: [nb, xstride] carry values of the level below
  int64_t xstride;
  float* out;        // [G, nb]
  int* ckey;         // [2 * nchunks] carry keys of the next level; nullptr on the last level
  float* cval;       // [nb, cstride] carry values
  int64_t cstride;
  int64_t m;
  int nb;
  int sig_b, w_b;    // sigma / w has one element
  int vec;           // level 0: key, and perm or every operand, are 16-byte aligned
  float edge[kMaxBins + 1];
};

__device__ __forceinline__ void put_carry(const GroupFwdArgs& a, int64_t slot, int col, int key,
                                          float val) {
  if (a.ckey == nullptr) return;
  if (col == 0) a.ckey[slot] = key;
  a.cval[col * a.cstride + slot] = val;
}

// L0: the values of a column are w * dPhi of the chunk's objects; else they are read from a.x.
template <bool L0>
__global__ __launch_bounds__(kGbThreads) void binned_group_fwd_kernel(GroupFwdArgs a) {
  __shared__ float wave_val[2][kGbWaves];
  __shared__ int wave_head[kGbWaves];
  __shared__ float red[kMaxBins * kGbWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wid = tid >> 6;
  const int64_t chunk = blockIdx.x;
  const int64_t c0 = chunk * kGbChunk;
  const int64_t p0 = c0 + (int64_t)tid * 4;
  const int64_t slot = chunk * 2;
  const int nb = a.nb;
  // uniform over the workgroup
  const bool whole = c0 + kGbChunk <= a.m;
  const bool full = whole && a.vec;

  int k[4];
  if (full) {
    const int4 kv = *reinterpret_cast<const int4*>(a.key + p0);
    k[0] = kv.x; k[1] = kv.y; k[2] = kv.z; k[3] = kv.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = p0 + j < a.m ? a.key[p0 + j] : kGbPast;
  }

  float m4[4], inv[4], wt[4], b0[4], f0[4];
  if constexpr (L0) {
    float s4[4];
    if (a.perm != nullptr) {
      int src[4];
      if (full) {
        const int4 sv = *reinterpret_cast<const int4*>(a.perm + p0);
        src[0] = sv.x; src[1] = sv.y; src[2] = sv.z; src[3] = sv.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) src[j] = p0 + j < a.m ? a.perm[p0 + j] : -1;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = src[j] >= 0;
        m4[j] = ok ? a.mu[src[j]] : 0.0f;
        s4[j] = ok ? a.sigma[a.sig_b ? 0 : src[j]] : 1.0f;
        wt[j] = !ok ? 0.0f : a.w == nullptr ? 1.0f : a.w[a.w_b ? 0 : src[j]];
      }
    } else {
      load_group<4>(a.mu, p0, a.m, full, false, 0.0f, 0.0f, m4);
      load_group<4>(a.sigma, p0, a.m, full, a.sig_b != 0, 1.0f, 1.0f, s4);
      load_group<4>(a.w, p0, a.m, full, a.w_b != 0, 1.0f, 0.0f, wt);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      inv[j] = 1.0f / s4[j];
      float gs;
      edge_cdf((a.edge[0] - m4[j]) * inv[j], b0[j], f0[j], gs);
    }
  }

  // the four values of column c; level 0 walks the edges, so c must go 0, 1, 2, ...
  auto column = [&](int c, float (&v)[4]) {
    if constexpr (L0) {
      const float e1 = a.edge[c + 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float b1, f1, gs;
        edge_cdf((e1 - m4[j]) * inv[j], b1, f1, gs);
        v[j] = wt[j] * ((b1 - b0[j]) + (f1 - f0[j]));
        b0[j] = b1;
        f0[j] = f1;
      }
    } else {
      const float* col = a.x + c * a.xstride;
      if (full) {  // the carry columns are fresh allocations with a stride of whole quads
        const float4 xv = *reinterpret_cast<const float4*>(col + p0);
        v[0] = xv.x; v[1] = xv.y; v[2] = xv.z; v[3] = xv.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p0 + j < a.m ? col[p0 + j] : 0.0f;
      }
    }
  };

  // Level 0 only: its keys are the plan's sorted ids, so an equal first and last key means that
  // one key fills the chunk.  (A carry list is not monotone -- unused slots, key -1, sit between
  // the real keys -- so equal ends say nothing about what lies between them; the carry levels
  // always take the scan.)
  if constexpr (L0) {
    const int kfirst = a.key[c0];
    if (whole && kfirst == a.key[c0 + kGbChunk - 1]) {
      // One key fills the chunk: a plain sum per column.
      const int kbefore = c0 > 0 ? a.key[c0 - 1] : kGbEdge;
      const int kafter = c0 + kGbChunk < a.m ? a.key[c0 + kGbChunk] : kGbEdge;
      for (int c = 0; c < nb; ++c) {
        float v[4];
        column(c, v);
        const float t = wave_sum((v[0] + v[1]) + (v[2] + v[3]));
        if (lane == 0) red[c * kGbWaves + wid] = t;
      }
      __syncthreads();
      if (tid < nb) {
        const float* r = red + tid * kGbWaves;
        const float tot = (r[0] + r[1]) + (r[2] + r[3]);
        const bool starts = kbefore != kfirst, ends = kafter != kfirst;
        if (starts && ends) {
          a.out[(int64_t)kfirst * nb + tid] = tot;
          put_carry(a, slot, tid, kGbNone, 0.0f);
          put_carry(a, slot + 1, tid, kGbNone, 0.0f);
        } else if (starts) {
          put_carry(a, slot, tid, kGbNone, 0.0f);
          put_carry(a, slot + 1, tid, kfirst, tot);
        } else {
          put_carry(a, slot, tid, kfirst, tot);
          put_carry(a, slot + 1, tid, ends ? kGbNone : kfirst, 0.0f);
        }
      }
      return;
    }
  }

  // The structure of the segmented scan, from the keys alone.
  int kprev = __shfl_up(k[3], 1, kWave);
  int knext = __shfl_down(k[0], 1, kWave);
  if (lane == 0) kprev = p0 > 0 && p0 - 1 < a.m ? a.key[p0 - 1] : kGbEdge;
  if (lane == kWave - 1) knext = p0 + 4 < a.m ? a.key[p0 + 4] : kGbEdge;
  bool hd[4], tl[4];  // entry j begins / ends a run
  hd[0] = k[0] != kprev;
  tl[3] = k[3] != knext;
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    hd[j] = k[j] != k[j - 1];
    tl[j - 1] = hd[j];
  }
  int f = hd[0] | hd[1] | hd[2] | hd[3];
  unsigned add = 0;  // bit s: step s of the lane scan adds the aggregate of lane - 2^s
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const int off = 1 << s;
    const int fo = __shfl_up(f, off, kWave);
    if (lane >= off && !f) add |= 1u << s;
    if (lane >= off) f |= fo;
  }
  int ef = __shfl_up(f, 1, kWave);  // a head in the lanes before this one in the wave
  if (lane == 0) ef = 0;
  if (lane == kWave - 1) wave_head[wid] = f;
  __syncthreads();
  unsigned heads = 0;  // bit w: wave w holds a head
#pragma unroll
  for (int w = 0; w < kGbWaves; ++w) heads |= wave_head[w] ? 1u << w : 0u;
  const bool pf = (heads & ((1u << wid) - 1u)) != 0;
  const bool inc_head = ef || pf;  // the run entering this thread began inside the chunk

  for (int c = 0; c < nb; ++c) {
    float v[4], s[4];
    column(c, v);
    // registers: s[j] = sum of the run of entry j over this thread's entries 0..j
    s[0] = v[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) s[j] = hd[j] ? v[j] : s[j - 1] + v[j];
    // lanes: inclusive segmented scan of the sum of each thread's last run
    float agg = s[3];
#pragma unroll
    for (int st = 0; st < 6; ++st) {
      const float ao = __shfl_up(agg, 1 << st, kWave);
      if ((add >> st) & 1u) agg += ao;
    }
    float ea = __shfl_up(agg, 1, kWave);
    if (lane == 0) ea = 0.0f;
    float* wv = wave_val[c & 1];
    if (lane == kWave - 1) wv[wid] = agg;
    __syncthreads();
    // LDS: the run that enters this wave, folded over the waves before it in a fixed order
    float pa = 0.0f;
#pragma unroll
    for (int w = 0; w < kGbWaves - 1; ++w)
      if (w < wid) pa = (heads >> w) & 1u ? wv[w] : pa + wv[w];
    const float inc = ef ? ea : pa + ea;
    bool seen = false, closed = false;
    float tot = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      seen = seen || hd[j];
      tot = seen ? s[j] : inc + s[j];
      closed = seen || inc_head;
      if (tl[j]) {
        if (!closed) {
          put_carry(a, slot, c, k[j], tot);  // the run entering from the left ends here
        } else if (k[j] >= 0) {
          a.out[(int64_t)k[j] * nb + c] = tot;
        }
      }
    }
    if (tid == 0 && hd[0]) put_carry(a, slot, c, kGbNone, 0.0f);
    if (tid == kGbThreads - 1) {  // tot / closed describe the chunk's last entry
      if (tl[3]) {
        put_carry(a, slot + 1, c, kGbNone, 0.0f);
      } else if (closed) {
        put_carry(a, slot + 1, c, k[3], tot);
      } else {  // one run covers the whole chunk
        put_carry(a, slot, c, k[3], tot);
        put_carry(a, slot + 1, c, k[3], 0.0f);
      }
    }
  }
}

// g is the [G, nb] table of cotangent rows; id[i] in [0, G) is the row of object i.
struct GroupGrad : BinnedGrad {
  const int* id;  // [n]
};

template <int NB, bool GMU, bool GSIG, bool GW>
__global__ __launch_bounds__(kBinThreads) void binned_group_bwd_kernel(BinnedArgs a,
                                                                       GroupGrad o, int direct) {
  __shared__ float red[2 * (kBinThreads / kWave)];
  const bool red_sig = GSIG && a.sig_b, red_w = GW && a.w_b;
  float rs[2] = {0.0f, 0.0f};  // this thread's share of the broadcast gradients
  const int64_t nq = (a.n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kBinThreads;
  for (int64_t q = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; q < nq; q += stride) {
    const int64_t i0 = q * 4;
    const bool full = i0 + 4 <= a.n;
    float m[4], inv[4], wt[4], b0[4], f0[4];
    float A[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sum_e h_e exp(-z_e^2/2)
    float B[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sum_e h_e z_e exp(-z_e^2/2)
    float C[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // sum_k g_k dPhi_k
    float gp[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // g[row, e - 1]
    load_quad(a, q, m, inv, wt);
    const float* row[4];  // the cotangent row of each object (row 0 beyond N: weight 0)
    if (a.vec && full) {
      const int4 iv = *reinterpret_cast<const int4*>(o.id + i0);
      row[0] = o.g + (int64_t)iv.x * a.nb;
      row[1] = o.g + (int64_t)iv.y * a.nb;
      row[2] = o.g + (int64_t)iv.z * a.nb;
      row[3] = o.g + (int64_t)iv.w * a.nb;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) row[j] = o.g + (int64_t)(i0 + j < a.n ? o.id[i0 + j] : 0) * a.nb;
    }
#pragma unroll
    for (int e = 0; e <= NB; ++e) {
      if (e <= a.nb) {  // wave-uniform: padded bins cost nothing
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gc = e < a.nb ? row[j][e] : 0.0f;
          const float z = (a.edge[e] - m[j]) * inv[j];
          float gs;
          if constexpr (GW) {
            float b1, f1;
            edge_cdf(z, b1, f1, gs);
            if (e > 0) C[j] = fmaf(gp[j], (b1 - b0[j]) + (f1 - f0[j]), C[j]);
            b0[j] = b1;
            f0[j] = f1;
          } else {
            const float ws = z * kWScale;
            gs = fast_exp2(-ws * ws);
          }
          const float hg = (gp[j] - gc) * gs;  // h_e = g_{e-1} - g_e (g_{-1} = g_{nb} = 0)
          if constexpr (GMU) A[j] += hg;
          if constexpr (GSIG) B[j] = fmaf(hg, z, B[j]);
          gp[j] = gc;
        }
      }
    }
    float dm[4], ds[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float c = -kInvSqrt2PiB * wt[j] * inv[j];  // 0 beyond N (weight 0)
      dm[j] = c * A[j];
      ds[j] = c * B[j];
      if (i0 + j >= a.n) C[j] = 0.0f;
    }
    if constexpr (GMU) store_group<4>(o.dmu, i0, a.n, dm);
    // put_quad and finish_broadcast (binned_common.h), written out: this kernel is close to
    // its register limits, and through the helpers (the same operations, blocks laid out in
    // another order) its instances are allocated up to 4 more VGPRs; NB = 16 with all three
    // gradients goes from 72 to 74 and loses a wave, and with it the grid and the sum order.
    if constexpr (GSIG) {
      if (red_sig) rs[0] += (ds[0] + ds[1]) + (ds[2] + ds[3]);
      else store_group<4>(o.dsigma, i0, a.n, ds);
    }
    if constexpr (GW) {
      if (red_w) rs[1] += (C[0] + C[1]) + (C[2] + C[3]);
      else store_group<4>(o.dw, i0, a.n, C);
    }
  }
  if (red_sig || red_w) {  // uniform over the grid
    block_sum_n<2>(rs, red);
    if (threadIdx.x == 0) {
      if (direct) {
        if (red_sig) o.dsigma[0] = rs[0];
        if (red_w) o.dw[0] = rs[1];
      } else {
        o.slab[(int64_t)blockIdx.x * 2 + 0] = rs[0];
        o.slab[(int64_t)blockIdx.x * 2 + 1] = rs[1];
      }
    }
  }
}

void check_plan(const torch::Tensor& ids, int64_t n, int64_t num_groups, const char* what) {
  check_dev(ids, what, at::kInt);
  TORCH_CHECK(n > 0 && n < (int64_t(1) << 31), "gaussian_binned_sum_by_group: 0 < N < 2^31 required");
  TORCH_CHECK(ids.numel() == n, what, " must have N elements");
  TORCH_CHECK(num_groups > 0 && num_groups < (int64_t(1) << 31),
              "gaussian_binned_sum_by_group: 0 < num_groups < 2^31 required");
}

}  // namespace

// sorted_ids are the plan's ids in sorted order; perm (optional) maps a sorted position to
// its object, for a plan whose index was not already sorted.  Returns [num_groups, nb].
torch::Tensor binned_group_forward(torch::Tensor sorted_ids, c10::optional<torch::Tensor> perm,
                                   torch::Tensor mu, torch::Tensor sigma,
                                   c10::optional<torch::Tensor> w, std::vector<double> edges,
                                   int64_t num_groups) {
  const BinnedArgs b = make_args(mu, sigma, w, edges);
  check_plan(sorted_ids, b.n, num_groups, "sorted_ids");
  GroupFwdArgs a;
  a.key = sorted_ids.data_ptr<int>();
  a.perm = nullptr;
  if (perm.has_value() && perm->defined()) {
    check_dev(*perm, "perm", at::kInt);
    TORCH_CHECK(perm->numel() == b.n, "perm must have N elements");
    a.perm = perm->data_ptr<int>();
  }
  a.mu = b.mu;
  a.sigma = b.sigma;
  a.w = b.w;
  a.x = nullptr;
  a.xstride = 0;
  a.m = b.n;
  a.nb = b.nb;
  a.sig_b = b.sig_b;
  a.w_b = b.w_b;
  a.vec = aligned16(a.key) && (a.perm != nullptr ? aligned16(a.perm) : b.vec != 0);
  for (int e = 0; e <= kMaxBins; ++e) a.edge[e] = b.edge[e];
  auto out = torch::zeros({num_groups, (int64_t)b.nb}, mu.options());
  a.out = out.data_ptr<float>();
  auto stream = at::hip::getCurrentHIPStream();
  const auto iopt = sorted_ids.options();
  torch::Tensor ckey, cval;  // keep a level's inputs alive until its launch is enqueued
  for (bool level0 = true;; level0 = false) {
    const int64_t nchunks = (a.m + kGbChunk - 1) / kGbChunk;
    torch::Tensor nkey, nval;
    if (nchunks > 1) {
      a.cstride = (2 * nchunks + 3) / 4 * 4;  // columns stay 16-byte aligned
      nkey = torch::empty({2 * nchunks}, iopt);
      nval = torch::empty({(int64_t)b.nb, a.cstride}, mu.options());
      a.ckey = nkey.data_ptr<int>();
      a.cval = nval.data_ptr<float>();
    } else {
      a.ckey = nullptr;
      a.cval = nullptr;
      a.cstride = 0;
    }
    if (level0)
      hipLaunchKernelGGL(binned_group_fwd_kernel<true>, dim3(nchunks), dim3(kGbThreads), 0, stream,
                         a);
    else
      hipLaunchKernelGGL(binned_group_fwd_kernel<false>, dim3(nchunks), dim3(kGbThreads), 0,
                         stream, a);
    if (nchunks == 1) break;
    ckey = nkey;
    cval = nval;
    a.key = a.ckey;
    a.perm = nullptr;
    a.x = a.cval;
    a.xstride = a.cstride;
    a.m = 2 * nchunks;
    a.vec = aligned16(a.key) && aligned16(a.x);
  }
  return out;
}

// Gradients of sum_{g,k} G[g, k] out[g, k] with respect to the requested operands, in the
// objects' original order (ids is the plan's unsorted int32 index); an operand that was not
// requested comes back undefined (None).  A broadcast operand gets the sum over objects.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> binned_group_backward(
    torch::Tensor ids, torch::Tensor mu, torch::Tensor sigma, c10::optional<torch::Tensor> w,
    std::vector<double> edges, torch::Tensor g, bool need_mu, bool need_sigma, bool need_w) {
  BinnedArgs a = make_args(mu, sigma, w, edges);
  check_dev(g, "grad_out", at::kFloat);
  TORCH_CHECK(g.dim() == 2 && g.size(1) == a.nb && g.size(0) > 0, "grad_out must be [G, nb]");
  check_plan(ids, a.n, g.size(0), "ids");
  TORCH_CHECK(!need_w || a.w != nullptr, "weights gradient requested without weights");
  TORCH_CHECK(need_mu || need_sigma || need_w, "no gradient requested");
  a.vec = a.vec && aligned16(ids.data_ptr<int>());
  const int nbp = padded_bins(a.nb, "gaussian_binned_sum");
  GroupGrad o = {};
  o.id = ids.data_ptr<int>();
  o.g = g.data_ptr<float>();
  auto dmu = alloc_grad(need_mu, a.n, mu, o.dmu);
  auto dsigma = alloc_grad(need_sigma, sigma.numel(), mu, o.dsigma);
  auto dw = alloc_grad(need_w, need_w ? w->numel() : 0, mu, o.dw);
  const auto r = reduce_sigma_w(a.sig_b ? o.dsigma : nullptr, a.w_b ? o.dw : nullptr);
  auto stream = at::hip::getCurrentHIPStream();
  MG_DISPATCH_BINNED(nbp, {
    with_need3(need_mu, need_sigma, need_w, [&](auto M, auto S, auto W) {
      launch_slab_bwd<binned_group_bwd_kernel<NB, decltype(M)::value, decltype(S)::value,
                                              decltype(W)::value>>(a, o, blocks_for(a.n), 2, r,
                                                                   mu, stream);
    });
  });
  return std::make_tuple(dmu, dsigma, dw);
}

}  // namespace mg
