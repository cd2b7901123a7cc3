// SMF kernels over the population-sorted halo array ("tiles"): the grid-stride forward, the
// slab reduction / loss / sumstat epilogue, and the tiles VJPs with their finalize (model
// and forward scheme: smf_device.h).
//
// The VJP recomputes z (no O(N*K) residuals) and contracts the edge
// weights h_e = (g_{e-1} scale_{e-1} - g_e scale_e)/sqrt(2 pi) with the Gaussian pdf in
// registers.  Per-population gradients are a *segmented* reduction over halos sorted
// by population.  A host-built tile schedule (build_tiles) cuts the halo array at
// population boundaries into tiles of <= 2048 halos / <= 2048 populations, so each tile
// is owned by one workgroup: blocked per-thread segments + a block-wide segmented scan
// write every population exactly once through LDS -- no float atomics, bitwise
// reproducible.  Populations larger than a tile are split into "partial" tiles whose
// sums are combined in a fixed order by a finalize kernel (this is also the path of the
// 2-parameter shared-parameter models).
#include "smf_device.h"
#include "smf_host.h"
#include "twoshot.h"

namespace mg {

// the fused exchange runs twoshot_block (grid-stride by kTsThreads) inside launches of
// kThreads threads: a mismatch would skip or double-update parameters
static_assert(kThreads == kTsThreads, "fused-exchange kernels must launch kTsThreads threads");

// Tiles-forward tunables (halos per thread per iteration; minimum resident waves per SIMD).
// Same-box A/B on the hashed per-rank proxy (1e7 params, 1/8 of the halos, ms/step, three
// alternating runs, profiles/fwd_knobs_r5/): unroll 1 0.1638-0.1665 vs 2 0.1668-0.1675;
// unroll 4 0.2901-0.2921 (spills); 6 waves 0.1659-0.1683 vs 8 0.1667-0.1691 (a tie).
#ifndef MG_FWD_UNROLL
#define MG_FWD_UNROLL 1
#endif
#ifndef MG_FWD_MINWAVES
#define MG_FWD_MINWAVES 8
#endif
constexpr int kFwdUnroll = MG_FWD_UNROLL;

// XS (fused exchange): workgroups [0, xs.blocks) run the two-shot exchange of the previous
// parameter chunk (twoshot.h) and the rest this forward, with their own block numbering --
// the exchange overlaps the forward without a second stream or cross-stream events.
// XS = 1: unbounded Adam (mode 1); 2: bounded (modes 2 / 3, its own instantiation so the
// unbounded kernel keeps its registers; 6 waves per SIMD instead of 8, which measured the
// same for this kernel, leave the bounded Adam 80 VGPRs instead of spilling at 64).
template <int NB, bool LOGSIG, bool HAS_POP, bool REL, int XS = 0>
__global__ __launch_bounds__(kThreads, XS == 2 ? 6 : MG_FWD_MINWAVES) void smf_fwd_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ pop,
    const float2* __restrict__ theta, int64_t begin, int64_t end, SmfBins bins,
    float* __restrict__ slab, TwoShotPack xs = TwoShotPack{}) {
  int bid = blockIdx.x, nblk = gridDim.x;
  if constexpr (XS > 0) {
    if (bid < xs.blocks) {
      __shared__ int xs_lds[2];  // 8 bytes: this kernel's occupancy is set by its VGPRs
      if constexpr (XS == 2) twoshot_block_fused_bounded(xs.a, xs.mode, bid, xs.blocks, xs_lds);
      else twoshot_block_fused(xs.a, bid, xs.blocks, xs_lds);
      return;
    }
    bid -= xs.blocks;
    nblk -= xs.blocks;
  }
  // signed-tail table: 8 replicas (8 workgroups per CU share the LDS)
  constexpr int kRepl = !REL ? 8 : 0;
  const float4* tb = nullptr;
  if constexpr (kRepl > 0) {
    __shared__ float4 tab[kTailTabN * (kRepl > 0 ? kRepl : 1)];
    tail_tab_fill<kRepl>(tab);
    __syncthreads();
    tb = tail_tab_lane<kRepl>(tab);
  }
  float acc[NB + 1];
  int cnt[NB + 1];
#pragma unroll
  for (int k = 0; k <= NB; ++k) acc[k] = 0.0f;
#pragma unroll
  for (int k = 0; k <= NB; ++k) cnt[k] = 0;
  const float2 th0 = HAS_POP ? make_float2(0.f, 0.f) : theta[0];
  const int64_t stride = (int64_t)nblk * kThreads;
  // the loop is wave-uniform (trip count from the wave's first halo; lanes past the end
  // are masked with x = -inf), so the ballot counts stay in SGPRs and are complete
  const int lane = threadIdx.x & (kWave - 1);
  const int wbase = __builtin_amdgcn_readfirstlane(threadIdx.x - lane);
  // Software pipeline over the grid-stride iterations: the halos of iteration k+2 (x and
  // population id) and the parameter gather of iteration k+1 are in flight while
  // iteration k is computed, so neither the id load nor the dependent gather is waited for
  // behind the math.
  if constexpr (HAS_POP) {
    const int64_t step = kFwdUnroll * stride;
    auto load_xp = [&](int64_t w, float (&xs)[kFwdUnroll], int (&ps)[kFwdUnroll]) {
#pragma unroll
      for (int u = 0; u < kFwdUnroll; ++u) {
        const int64_t i = w + lane + u * stride;
        const bool ok = i < end;
        xs[u] = ok ? x[i] : -INFINITY;
        ps[u] = ok ? pop[i] : 0;
      }
    };
    int64_t w0 = begin + (int64_t)bid * kThreads + wbase;
    float xa[kFwdUnroll], xb[kFwdUnroll];
    int pa[kFwdUnroll], pb[kFwdUnroll];
    float2 tha[kFwdUnroll];
    load_xp(w0, xa, pa);
#pragma unroll
    for (int u = 0; u < kFwdUnroll; ++u) tha[u] = theta[pa[u]];
    load_xp(w0 + step, xb, pb);
    for (; w0 < end; w0 += step) {
      float2 thb[kFwdUnroll];
#pragma unroll
      for (int u = 0; u < kFwdUnroll; ++u) thb[u] = theta[pb[u]];
      float xc[kFwdUnroll];
      int pc[kFwdUnroll];
      load_xp(w0 + 2 * step, xc, pc);
#pragma unroll
      for (int u = 0; u < kFwdUnroll; ++u)
        halo_mass<NB, LOGSIG, REL, kRepl>(xa[u], tha[u], bins, acc, cnt, tb);
#pragma unroll
      for (int u = 0; u < kFwdUnroll; ++u) {
        xa[u] = xb[u];
        tha[u] = thb[u];
        xb[u] = xc[u];
        pb[u] = pc[u];
      }
    }
  } else
  for (int64_t w0 = begin + (int64_t)bid * kThreads + wbase; w0 < end;
       w0 += kFwdUnroll * stride) {
    // issue every load of this iteration before any math (one dependent round trip)
    float xs[kFwdUnroll];
    int ps[kFwdUnroll];
    float2 ths[kFwdUnroll];
#pragma unroll
    for (int u = 0; u < kFwdUnroll; ++u) {
      const int64_t i = w0 + lane + u * stride;
      const bool ok = i < end;
      xs[u] = ok ? x[i] : -INFINITY;  // -inf: exactly zero contribution, no branch
      ps[u] = (HAS_POP && ok) ? pop[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < kFwdUnroll; ++u) ths[u] = HAS_POP ? theta[ps[u]] : th0;
#pragma unroll
    for (int u = 0; u < kFwdUnroll; ++u)
      halo_mass<NB, LOGSIG, REL, kRepl>(xs[u], ths[u], bins, acc, cnt, tb);
  }
  const bool counter = lane == 0;  // the counts are per wave: fold them in once
#pragma unroll
  for (int k = 0; k < NB; ++k)
    acc[k] = (acc[k + 1] - acc[k]) + (counter ? (float)(cnt[k + 1] - cnt[k]) : 0.0f);
  __shared__ float scratch[NB * (kThreads / kWave)];
  float(&bin)[NB] = *reinterpret_cast<float(*)[NB]>(acc);
  block_sum_n<NB>(bin, scratch);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NB; ++k) slab[(int64_t)bid * NB + k] = acc[k];
  }
}

// Sum nrows slab rows per bin in a fixed order (double accumulation), apply the bin
// scale, write out[bin].  One workgroup per bin.
__global__ __launch_bounds__(kThreads) void slab_reduce_kernel(
    const float* __restrict__ slab, int nrows, int nb, SmfBins bins, float* __restrict__ out) {
  __shared__ double scratch[kThreads / kWave];
  const int k = blockIdx.x;
  double s = 0.0;
  for (int r = threadIdx.x; r < nrows; r += kThreads) s += (double)slab[(int64_t)r * nb + k];
  double v[1] = {s};
  block_sum_n<1>(v, scratch);
  if (threadIdx.x == 0) out[k] = (float)(v[0] * (double)bins.scale[k]);
}

__global__ void edge_weights_kernel(const float* __restrict__ g, int nb, SmfBins bins,
                                    float* __restrict__ h) {
  const int e = threadIdx.x;
  if (e <= nb) h[e] = edge_weight(g, bins, e, nb);
}

// log-MSE loss on total sumstats (reference tests/smf_example/smf_grad_descent.py:78-82,
// docs variant adds eps=1e-10): loss = mean_k (log10(S_k+eps) - log10(T_k+eps))^2.
// Writes loss[0], the cotangent-derived edge weights h[0..nb] and dL/dS into g_out.
__global__ void logmse_loss_kernel(const float* __restrict__ S, const float* __restrict__ target,
                                   float eps, int nb, SmfBins bins, float* __restrict__ loss,
                                   float* __restrict__ g_out, float* __restrict__ h) {
  __shared__ float g[kMaxBins];
  __shared__ float d2[kMaxBins];
  const int k = threadIdx.x;
  if (k < nb) {
    const float s = S[k] + eps;
    const float d = log10f(s) - log10f(target[k] + eps);
    d2[k] = d * d;
    g[k] = 2.0f / nb * d / (s * kLn10);
    if (g_out) g_out[k] = g[k];
  }
  __syncthreads();
  if (k == 0) {
    float acc = 0.0f;
    for (int j = 0; j < nb; ++j) acc += d2[j];
    loss[0] = acc / nb;
  }
  if (k <= nb && h) h[k] = edge_weight(g, bins, k, nb);
}

// Sumstat epilogue of one engine step in ONE launch (one workgroup of MG_EPI_THREADS):
//   slab rows -> local S (fixed-order double sums, bin scale)       [slab_reduce_kernel]
//   -> cross-rank sum through the one-shot peer-memory exchange      [xgmi.h, size > 1]
//   -> log-MSE loss and edge weights h (padded edges zeroed)         [logmse_loss_kernel]
// Replaces three launches and a memset per step (~14 us on an 8-GPU owner shard).
// MG_EPI_THREADS: the block reduction and its barriers cost more than the extra rounds of
// slab-row loads they save -- same-box A/B, ms/step: 1024 threads 14.6 vs 8.0 us per launch
// at the headline (round 2); owner-shard proxy 512: 0.0644-0.0646 vs 256: 0.0622-0.0625;
// 128: 0.0615-0.0619 vs 256: 0.0624-0.0628, headline 0.4338-0.4348 vs 0.4348-0.4375;
// 64: 0.0617-0.0619 vs 128: 0.0615-0.0616 (round 4, tools/ab_bench_so.sh)
#ifndef MG_EPI_THREADS
#define MG_EPI_THREADS 128
#endif
constexpr int kEpiThreads = MG_EPI_THREADS;

// The epilogue as the work of ONE whole workgroup of NT threads, reducing the slab row by
// row.  (A flat-array reduction with coalesced loads measured within the run-to-run spread
// on the owner proxy and the headline -- round 4, profiles/knobs_r4/ -- and was removed.)
template <int NB, int NT, int U = 4>
__device__ __forceinline__ void epilogue_block(const EpiArgs& E, const SmfBins& bins) {
  __shared__ double scratch[NB * (NT / kWave)];
  __shared__ float Sv[kXMaxFloats];
  __shared__ float g[kMaxBins];
  __shared__ float d2[kMaxBins];
  const float* __restrict__ slab = E.slab;
  const int nrows = E.nrows, nb = E.nb;
  {
    double v[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) v[k] = 0.0;
    // rows U at a time with every load issued before the first add (one memory round trip
    // per U rows instead of one per row); the per-thread order of the sums is the row order
    // whatever U is (the same bits)
    auto ld = [&](int64_t i) -> float { return slab[i]; };
    int r = threadIdx.x;
    for (; r + (U - 1) * NT < nrows; r += U * NT) {
      float a[U][NB];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < NB; ++k) a[u][k] = ld((int64_t)(r + u * NT) * NB + k);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] += (double)a[u][k];
    }
    for (; r < nrows; r += NT) {
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] += (double)ld((int64_t)r * NB + k);
    }
    block_sum_n<NB>(v, scratch);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < NB; ++k) Sv[k] = (float)(v[k] * (double)bins.scale[k]);
    }
  }
  __syncthreads();
  if (E.size > 1) xgmi_block_allreduce(E.peers, E.rank, E.size, Sv, NB, E.seq, E.err, E.ticks);
  const int k = threadIdx.x;
  if (k < NB) E.S_out[k] = Sv[k];
  if (k < nb) {
    const float s = Sv[k] + E.eps;
    const float d = log10f(s) - log10f(E.target[k] + E.eps);
    d2[k] = d * d;
    g[k] = 2.0f / nb * d / (s * kLn10);
  }
  __syncthreads();
  if (k == 0) {
    float acc = 0.0f;
    for (int j = 0; j < nb; ++j) acc += d2[j];
    E.loss[0] = acc / nb;
  }
  if (k <= NB) E.h[k] = k <= nb ? edge_weight(g, bins, k, nb) : 0.0f;
  // the pipelined engine's device step counter, advanced here (the last launch of a step)
  // instead of by a one-thread kernel of its own
  if (E.advance != nullptr && threadIdx.x == 0) E.advance[0] += 1;
}

// Rows per load round of the stand-alone epilogue: MG_EPI_UNROLL rows of NB floats in
// flight per thread.  16 measured slower than 4 (owner proxy 0.0620-0.0623 vs 0.0609-0.0614
// ms/step, same-box A/B, round 4)
#ifndef MG_EPI_UNROLL
#define MG_EPI_UNROLL 4
#endif

template <int NB>
__global__ __launch_bounds__(kEpiThreads) void smf_epilogue_kernel(EpiArgs E, SmfBins bins) {
  epilogue_block<NB, kEpiThreads, MG_EPI_UNROLL>(E, bins);
}

// Segmented-scan combine: (flag, A, B) pairs.
struct Seg {
  int f;
  float a, b;
};

template <int NB, bool LOGSIG>
__global__ __launch_bounds__(kThreads) void smf_vjp_tiles_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ pop,
    const float2* __restrict__ theta, const Tile* __restrict__ tiles,
    const float* __restrict__ hvec, SmfBins bins, float2* __restrict__ grad,
    float2* __restrict__ partials) {
  const Tile t = tiles[blockIdx.x];
  float h[NB + 1];
#pragma unroll
  for (int e = 0; e <= NB; ++e) h[e] = hvec[e];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wid = tid >> 6;

  if (t.slot >= 0) {  // partial tile: one population, plain block reduction
    const float2 th = theta[t.p0];
    const float inv = inv_sigma<LOGSIG>(th.y) * kWScale;
    float v[2] = {0.0f, 0.0f};
    for (int64_t i0 = t.h0 + tid; i0 < t.h1; i0 += 4 * kThreads) {
      float xs[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) xs[u] = i0 + u * kThreads < t.h1 ? x[i0 + u * kThreads] : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i0 + u * kThreads < t.h1) halo_vjp<NB, LOGSIG>(xs[u], th, inv, h, bins, v[0], v[1]);
    }
    __shared__ float scratch[2 * (kThreads / kWave)];
    block_sum_n<2>(v, scratch);
    if (tid == 0) partials[t.slot] = make_float2(v[0], v[1]);
    return;
  }

  // LDS: per-halo (A, B) contributions, later re-used as the per-population result
  // array (kTileHalos == kTilePops), local population ids, and the scan scratch.
  __shared__ float2 s_ab[kTileHalos];
  __shared__ int16_t s_lp[kTileHalos];
  __shared__ int s_tailpop[kThreads];
  __shared__ int s_headpop[kThreads];
  __shared__ float2 s_incl[kThreads];
  __shared__ Seg s_wagg[kThreads / kWave];
  float2* res = s_ab;
  static_assert(kTileHalos == kTilePops, "result array aliases the contribution array");

  // ---- phase 1: coalesced loads (all rounds issued up front), per-halo contributions
  {
    float xs[kItems];
    int ps[kItems];
    float2 ths[kItems];
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
      const int64_t i = t.h0 + r * kThreads + tid;
      const bool ok = i < t.h1;
      xs[r] = ok ? x[i] : 0.0f;
      ps[r] = ok ? pop[i] : t.p0;
    }
#pragma unroll
    for (int r = 0; r < kItems; ++r) ths[r] = theta[ps[r]];
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
      float A = 0.f, B = 0.f;
      const float inv = inv_sigma<LOGSIG>(ths[r].y) * kWScale;
      halo_vjp<NB, LOGSIG>(xs[r], ths[r], inv, h, bins, A, B);
      s_ab[r * kThreads + tid] = make_float2(A, B);
      s_lp[r * kThreads + tid] = (int16_t)(ps[r] - t.p0);
    }
  }
  __syncthreads();
  // ---- phase 2: blocked per-thread sequential segmented reduction over <= kItems halos
  const int base = tid * kItems;
  const int cnt = (int)max((int64_t)0, min((int64_t)kItems, (t.h1 - t.h0) - base));
  float2 ab[kItems];
  int lp[kItems];
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    ab[j] = s_ab[base + j];
    lp[j] = s_lp[base + j];
  }
  __syncthreads();  // contributions are in registers: s_ab becomes res
  const int npops = t.p1 - t.p0;
  for (int k = tid; k < npops; k += kThreads) res[k] = make_float2(0.f, 0.f);
  __syncthreads();
  int headpop = -1, curpop = -1, nseg = 0;  // local population ids
  float headA = 0.f, headB = 0.f, curA = 0.f, curB = 0.f;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    if (j < cnt) {
      const int c = lp[j];
      if (c != curpop) {
        if (nseg == 1) {
          headpop = curpop; headA = curA; headB = curB;
        } else if (nseg > 1) {
          res[curpop] = make_float2(curA, curB);  // interior segment owned by this thread
        }
        curpop = c; curA = 0.f; curB = 0.f; ++nseg;
      }
      curA += ab[j].x;
      curB += ab[j].y;
    }
  }
  if (nseg == 1) { headpop = curpop; headA = curA; headB = curB; }
  const bool boundary = nseg > 1;
  // ---- block-wide segmented inclusive scan of the tail segments
  s_headpop[tid] = cnt ? headpop : -1;
  s_tailpop[tid] = cnt ? curpop : -1;
  __syncthreads();
  const int prevtail = tid ? s_tailpop[tid - 1] : -1;
  Seg s;
  s.f = (cnt == 0) || boundary || tid == 0 || prevtail != curpop;
  s.a = cnt ? curA : 0.f;
  s.b = cnt ? curB : 0.f;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int f2 = __shfl_up(s.f, o, kWave);
    const float a2 = __shfl_up(s.a, o, kWave);
    const float b2 = __shfl_up(s.b, o, kWave);
    if (lane >= o && !s.f) { s.a += a2; s.b += b2; }
    if (lane >= o) s.f |= f2;
  }
  if (lane == kWave - 1) s_wagg[wid] = s;
  __syncthreads();
  if (!s.f) {  // no segment start between wave start and this lane: add earlier waves
    for (int w = wid - 1; w >= 0; --w) {
      const Seg g = s_wagg[w];
      s.a += g.a; s.b += g.b;
      if (g.f) break;
    }
  }
  s_incl[tid] = make_float2(s.a, s.b);
  __syncthreads();
  // head segment completes inside this thread: add the carry from earlier threads
  if (cnt && boundary) {
    float2 carry = make_float2(0.f, 0.f);
    if (tid && prevtail == headpop) carry = s_incl[tid - 1];
    res[headpop] = make_float2(headA + carry.x, headB + carry.y);
  }
  // tail segment ends here unless the next thread continues it
  if (cnt) {
    const int nexthead = tid + 1 < kThreads ? s_headpop[tid + 1] : -1;
    if (nexthead != curpop) res[curpop] = s_incl[tid];
  }
  __syncthreads();
  for (int k = tid; k < npops; k += kThreads) {
    const int c = t.p0 + k;
    const float2 r = res[k];
    grad[c] = pop_grad<LOGSIG>(theta[c], r.x, r.y);
  }
}

// giant[g] = {pop, slot_begin, slot_end}: sum partial slots in order.
template <bool LOGSIG>
__global__ __launch_bounds__(kThreads) void smf_vjp_finalize_kernel(
    const int32_t* __restrict__ giant, const float2* __restrict__ partials,
    const float2* __restrict__ theta, float2* __restrict__ grad) {
  const int c = giant[3 * blockIdx.x], s0 = giant[3 * blockIdx.x + 1], s1 = giant[3 * blockIdx.x + 2];
  double v[2] = {0.0, 0.0};
  for (int s = s0 + threadIdx.x; s < s1; s += kThreads) {
    const float2 p = partials[s];
    v[0] += p.x; v[1] += p.y;
  }
  __shared__ double scratch[2 * (kThreads / kWave)];
  block_sum_n<2>(v, scratch);
  if (threadIdx.x == 0) grad[c] = pop_grad<LOGSIG>(theta[c], (float)v[0], (float)v[1]);
}

// ================================================= tiles VJP, recurrence + owner segments
// Uniform unpadded bins: the tiles VJP of the hashed shards with
// (1) the Gaussian factors of one halo's equally spaced edges from one seed pair at the
//     middle edges and the exact ratio recurrence f_{e+2} = f_e exp2(-4 dw w_{e+1}) (the
//     ratio itself advances by the constant exp2(-8 dw^2)): 6 transcendentals per halo
//     instead of 12, two v_pk_fma per edge pair for the sums A = sum h_e f_e and
//     D = sum (e - 2M) h_e f_e, and B = sum h_e f_e w_e = w_{2M} A + dw D by linearity;
// (2) per-halo contributions already in gradient units (every halo of a population
//     shares its inverse sigma), so a population's gradient is the plain sum of its
//     halos' contributions; and
// (3) no block-wide scan: after the coalesced per-halo pass, each thread walks 8
//     consecutive halos; the thread holding a population's FIRST halo owns it, adds the
//     head partials of the following threads it continues into (fixed order: bitwise
//     reproducible), writes the gradient straight to HBM and zero-fills the ids up to the
//     next population present (populations without halos on this rank).
// The seed sits at the middle pair, so a seed that underflows (|z| > 13) is at least
// 13 - NB/2 h sigma away from every edge; with h = delta/sigma <= 1 (dw <= kWScale, checked
// wave-uniformly, else the per-edge path of halo_vjp) the dropped terms are below 3e-15.

template <int NB>
struct VjpPairs {
  v2f h[EdgePairs<NB>::NV];  // h_e in the edge-pair layout (odd last edge in .x of the extra pair)
  v2f d[EdgePairs<NB>::NV];  // (e - 2M) h_e
};

// One halo: A = sum_e h_e f_e, D = sum_e (e - 2M) h_e f_e, wc = w_{2M}; nm = -(x + a) inv.
template <int NB>
__device__ __forceinline__ void halo_vjp_rec(float nm, float inv, float dw, const VjpPairs<NB>& W,
                                             const SmfBins& b, float& A, float& D, float& wc) {
  using EP = EdgePairs<NB>;
  constexpr int M = EP::NP / 2;
  v2f e2;
  e2.x = b.edge[2 * M];
  e2.y = b.edge[2 * M + 1];
  const v2f ws = e2 * inv + nm;
  const v2f q = -ws * ws;
  v2f p0;
  p0.x = fast_exp2(q.x);
  p0.y = fast_exp2(q.y);
  const float dw4 = -4.0f * dw;
  const float C2 = fast_exp2(dw4 * dw);  // exp2(-4 dw^2): ratio of the two halves of a pair
  const float C4 = C2 * C2;              // per-pair advance of the ratio
  v2f Af = W.h[M] * p0, Df = W.d[M] * p0;
  v2f R;
  R.x = fast_exp2(__builtin_amdgcn_fmed3f(dw4 * ws.y, -126.0f, 126.0f));
  R.y = R.x * C2;
  v2f p = p0;
#pragma unroll
  for (int i = M + 1; i < EP::NP; ++i) {
    p = p * R;
    Af = W.h[i] * p + Af;
    Df = W.d[i] * p + Df;
    R = R * C4;
  }
  if constexpr (EP::NX) {
    const float f = p.x * R.x;
    Af.x = fmaf(W.h[EP::NP].x, f, Af.x);
    Df.x = fmaf(W.d[EP::NP].x, f, Df.x);
  }
  if constexpr (M > 0) {
    v2f Rb;
    Rb.y = fast_exp2(__builtin_amdgcn_fmed3f(-dw4 * ws.x, -126.0f, 126.0f));
    Rb.x = Rb.y * C2;
    p = p0;
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
      p = p * Rb;
      Af = W.h[i] * p + Af;
      Df = W.d[i] * p + Df;
      Rb = Rb * C4;
    }
  }
  A = Af.x + Af.y;
  D = Df.x + Df.y;
  wc = ws.x;
}

template <int NB, bool LOGSIG, int XS = 0>
#ifndef MG_VJP_REC_MINWAVES
#define MG_VJP_REC_MINWAVES 8  // 20 KB of LDS and <= 64 VGPRs: 8 workgroups per CU
#endif
__global__ __launch_bounds__(kThreads, XS == 2 ? 6 : MG_VJP_REC_MINWAVES) void smf_vjp_tiles_rec_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ pop,
    const float2* __restrict__ theta, const Tile* __restrict__ tiles,
    const float* __restrict__ hvec, SmfBins bins, float2* __restrict__ grad,
    float2* __restrict__ partials, TwoShotPack xs = TwoShotPack{}) {
  // XS (fused exchange): workgroups [0, xs.blocks) run the two-shot exchange of the
  // previous parameter chunk (its gradient is complete: the launch that wrote it ended
  // before this one), the rest one tile each
  // LDS (20 KB, so 8 workgroups fit a CU): per-halo contributions (later the per-population
  // results) and local population ids (later the head partials and their successors); the
  // exchange workgroups of the XS variant borrow its first 8 bytes for their flags, so the
  // fused kernel keeps the same 20 KB and 8 workgroups per CU
  __shared__ __attribute__((aligned(16))) char smem[kTileHalos * (sizeof(float2) + sizeof(int16_t))];
  int tb = blockIdx.x;
  if constexpr (XS > 0) {
    if (tb < xs.blocks) {
      if constexpr (XS == 2)
        twoshot_block_fused_bounded(xs.a, xs.mode, tb, xs.blocks, reinterpret_cast<int*>(smem));
      else
        twoshot_block_fused(xs.a, tb, xs.blocks, reinterpret_cast<int*>(smem));
      return;
    }
    tb -= xs.blocks;
  }
  using EP = EdgePairs<NB>;
  constexpr int M = EP::NP / 2;
  const Tile t = tiles[tb];
  const int tid = threadIdx.x;
  if (t.slot >= 0) {  // partial tile (one giant population): the per-edge block reduction
    float h[NB + 1];
#pragma unroll
    for (int e = 0; e <= NB; ++e) h[e] = hvec[e];
    const float2 th = theta[t.p0];
    const float inv = inv_sigma<LOGSIG>(th.y) * kWScale;
    float v[2] = {0.0f, 0.0f};
    for (int64_t i = t.h0 + tid; i < t.h1; i += kThreads)
      halo_vjp<NB, LOGSIG>(x[i], th, inv, h, bins, v[0], v[1]);
    block_sum_n<2>(v, reinterpret_cast<float*>(smem));
    if (tid == 0) partials[t.slot] = make_float2(v[0], v[1]);
    return;
  }
  const int n = (int)(t.h1 - t.h0);
  const int npops = t.p1 - t.p0;
  float2* __restrict__ gout = grad + t.p0;
  if (n <= 0) {  // populations without halos on this rank
    for (int k = tid; k < npops; k += kThreads) gout[k] = make_float2(0.f, 0.f);
    return;
  }
  VjpPairs<NB> W;
#pragma unroll
  for (int i = 0; i < EP::NV; ++i) {
    const int e0 = 2 * i, e1 = 2 * i + 1;
    W.h[i].x = hvec[e0];
    W.h[i].y = e1 <= NB ? hvec[e1] : 0.0f;
    W.d[i].x = (float)(e0 - 2 * M) * W.h[i].x;
    W.d[i].y = (float)(e1 - 2 * M) * W.h[i].y;
  }
  // s_g: per-halo contributions, 16-byte slot s (halos 2s, 2s+1) stored at slot
  // swz(s) = s ^ ((s >> 4) & 3): thread t's blocked read of slots 4t..4t+3 then hits 16
  // distinct bank slots per ds_read_b128 lane group (t mod 4 x (t >> 2) mod 4), and the
  // striped phase-1 writes stay contiguous per 8 slots.  s_lp: local ids, plain order.
  float2* s_g = reinterpret_cast<float2*>(smem);
  int16_t* s_lp = reinterpret_cast<int16_t*>(smem + kTileHalos * sizeof(float2));
  float2* res = s_g;                                      // per-population results (phase 2)
  float2* s_head = reinterpret_cast<float2*>(s_lp);       // head partials (phase 2)
  int* s_pass = reinterpret_cast<int*>(s_head + kThreads);
  static_assert(kThreads * (sizeof(float2) + sizeof(int)) <= kTileHalos * sizeof(int16_t),
                "head partials alias the id array");
  static_assert(kTileHalos == kTilePops, "result array aliases the contribution array");
  auto swz = [](int i) { return i ^ (((i >> 5) & 3) << 1); };  // halo index -> float2 index
  // ---- phase 1: coalesced loads, per-halo gradient contributions in halo order
  {
    float xs[kItems];
    int ps[kItems];
    float2 ths[kItems];
    // uniform tile base + clamped 32-bit offsets (always valid addresses, no branches)
    const float* __restrict__ xt = x + t.h0;
    const int32_t* __restrict__ pt = pop + t.h0;
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
      const int i = min(r * kThreads + tid, n - 1);
      xs[r] = xt[i];
      ps[r] = pt[i];
    }
#pragma unroll
    for (int r = 0; r < kItems; ++r) ths[r] = theta[ps[r]];
    bool ok = true;
#pragma unroll
    for (int r = 0; r < kItems; ++r) ok = ok && bins.delta * inv_sigma<LOGSIG>(ths[r].y) <= 1.0f;
    constexpr float kInvW = 1.0f / kWScale;
    if (__builtin_amdgcn_ballot_w64(!ok) == 0) {  // wave-uniform: the recurrence for all 8
#pragma unroll
      for (int r = 0; r < kItems; ++r) {
        const float is = inv_sigma<LOGSIG>(ths[r].y);
        const float inv = is * kWScale;
        const float dw = bins.delta * inv;
        float A, D, wc;
        halo_vjp_rec<NB>(-(xs[r] + ths[r].x) * inv, inv, dw, W, bins, A, D, wc);
        const float B = fmaf(wc, A, dw * D);
        const int li = r * kThreads + tid;
        s_g[swz(li)] = make_float2(-is * A, LOGSIG ? -(kLn10 * kInvW) * B : -(is * kInvW) * B);
        s_lp[li] = (int16_t)(ps[r] - t.p0);
      }
    } else {
      float h[NB + 1];
#pragma unroll
      for (int e = 0; e <= NB; ++e) h[e] = hvec[e];
#pragma unroll
      for (int r = 0; r < kItems; ++r) {
        const float is = inv_sigma<LOGSIG>(ths[r].y);
        float A = 0.f, B = 0.f;
        halo_vjp<NB, LOGSIG>(xs[r], ths[r], is * kWScale, h, bins, A, B);
        const int li = r * kThreads + tid;
        s_g[swz(li)] = make_float2(-is * A, LOGSIG ? -(kLn10 * kInvW) * B : -(is * kInvW) * B);
        s_lp[li] = (int16_t)(ps[r] - t.p0);
      }
    }
  }
  __syncthreads();
  // ---- phase 2: 8 consecutive halos per thread; a population belongs to the thread that
  // holds its FIRST halo in the tile
  const int base = tid * kItems;
  const int cnt = max(0, min(kItems, n - base));
  float2 g[kItems];
  int lp[kItems];
  {
    const float4* sg4 = reinterpret_cast<const float4*>(s_g);
    const int sw = (tid >> 2) & 3;
#pragma unroll
    for (int k = 0; k < kItems / 2; ++k) {
      const float4 v = sg4[4 * tid + (k ^ sw)];
      g[2 * k] = make_float2(v.x, v.y);
      g[2 * k + 1] = make_float2(v.z, v.w);
    }
    const uint4 l4 = reinterpret_cast<const uint4*>(s_lp)[tid];
    const unsigned lw[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lp[2 * k] = (int)(lw[k] & 0xFFFFu);
      lp[2 * k + 1] = (int)(lw[k] >> 16);
    }
  }
#pragma unroll
  for (int j = 1; j < kItems; ++j) {  // past the tile end: same population, zero contribution
    const bool in = j < cnt;
    lp[j] = in ? lp[j] : lp[j - 1];
    g[j].x = in ? g[j].x : 0.0f;
    g[j].y = in ? g[j].y : 0.0f;
  }
  const int prevlp = (cnt > 0 && base > 0) ? (int)s_lp[base - 1] : -1;
  const int nextlp = base + kItems < n ? (int)s_lp[base + kItems] : npops;
  __syncthreads();  // contributions and ids are in registers: s_g, s_lp are reused
  for (int k = tid; k < npops; k += kThreads) res[k] = make_float2(0.f, 0.f);  // no halos: 0
  __syncthreads();
  int c = lp[0];
  float2 cur = g[0];
  const bool headcont = cnt > 0 && c == prevlp;  // first segment continues an earlier thread's
  bool inhead = true;
  float2 hsum = make_float2(0.f, 0.f);
  if (cnt > 0) {
#pragma unroll
    for (int j = 1; j < kItems; ++j) {
      const bool brk = lp[j] != c;
      const bool hb = brk && inhead && headcont;
      if (brk && !hb) res[c] = cur;  // a whole segment inside this thread
      hsum.x = hb ? cur.x : hsum.x;
      hsum.y = hb ? cur.y : hsum.y;
      inhead = inhead && !brk;
      cur.x = brk ? g[j].x : cur.x + g[j].x;
      cur.y = brk ? g[j].y : cur.y + g[j].y;
      c = lp[j];
    }
  }
  const bool contonly = cnt > 0 && inhead && headcont;  // every halo continues the head
  if (contonly) hsum = cur;
  s_head[tid] = hsum;
  s_pass[tid] = contonly && nextlp == c;  // ... and it goes on into the next thread
  __syncthreads();
  if (cnt > 0 && !contonly) {  // this thread owns its tail segment (population c)
    if (nextlp == c) {
      for (int k = tid + 1; k < kThreads; ++k) {
        const float2 hp = s_head[k];
        cur.x += hp.x;
        cur.y += hp.y;
        if (!s_pass[k]) break;
      }
    }
    res[c] = cur;
  }
  __syncthreads();
  for (int k = tid; k < npops; k += kThreads) gout[k] = res[k];
}

// ------------------------------------------------------------------ host side
int smf_padded_bins(int64_t nb) { return padded_bins((int)nb); }

// Grid that exactly fills the chip with resident forward workgroups (occupancy x CUs), so
// the grid-stride loop runs in a single wave of workgroups without a partial tail round.
int64_t smf_fwd_max_blocks(int64_t nb, bool log_sigma, bool has_pop, bool rel_tail) {
  const int nbp = padded_bins((int)nb);
  int64_t blocks = 0;
  MG_DISPATCH_NB(nbp, {
    with_bool(log_sigma, [&](auto LS) { with_bool(has_pop, [&](auto HP) { with_bool(rel_tail, [&](auto RT) {
      blocks = resident_blocks(
          (const void*)smf_fwd_kernel<NB, decltype(LS)::value, decltype(HP)::value, decltype(RT)::value>,
          kThreads);
    }); }); });
  });
  return blocks;
}

// Forward over halos [begin, end); writes slab[nblocks * NBP].
// exchange (bytes of xgmi_twoshot_pack, or empty): a two-shot exchange this launch runs in
// extra leading workgroups (fused exchange); kernels that cannot carry it (no population
// ids, relative tails) launch it on its own first.
void smf_forward(torch::Tensor x, c10::optional<torch::Tensor> pop, torch::Tensor theta,
                 std::vector<double> edges, std::vector<double> scale, bool log_sigma,
                 int64_t begin, int64_t end, torch::Tensor slab, int64_t nblocks, bool rel_tail,
                 std::string exchange) {
  check_dev(x, "x", at::kFloat);
  check_dev(theta, "theta", at::kFloat);
  check_dev(slab, "slab", at::kFloat);
  const int nbp = padded_bins((int)scale.size());
  TORCH_CHECK(begin >= 0 && end <= x.numel() && begin <= end, "bad halo range");
  TORCH_CHECK(slab.numel() >= nblocks * nbp, "slab too small");
  TORCH_CHECK(nblocks >= 1 && nblocks <= 65535, "bad block count");
  const bool has_pop = pop.has_value() && pop->defined();
  if (has_pop) {
    check_dev(*pop, "pop", at::kInt);
    TORCH_CHECK(pop->numel() == x.numel(), "pop/x size mismatch");
  } else {
    TORCH_CHECK(theta.numel() >= 2, "theta needs 2 entries");
  }
  const SmfBins b = make_bins(edges, scale, nbp);
  auto stream = at::hip::getCurrentHIPStream();
  const float* xp = x.data_ptr<float>();
  const int32_t* pp = has_pop ? pop->data_ptr<int32_t>() : nullptr;
  const float2* tp = reinterpret_cast<const float2*>(theta.data_ptr<float>());
  float* sp = slab.data_ptr<float>();
  if (!exchange.empty()) {
    const TwoShotPack xs = twoshot_unpack(exchange);
    if (has_pop && !rel_tail && xs.mode >= 1 && xs.mode <= 3) {
      TORCH_CHECK(nblocks + xs.blocks <= 65535, "bad block count");
      MG_DISPATCH_NB(nbp, {
        with_bool(log_sigma, [&](auto LS) {
          if (xs.mode == 1)
            hipLaunchKernelGGL((smf_fwd_kernel<NB, decltype(LS)::value, true, false, 1>),
                               dim3(nblocks + xs.blocks), dim3(kThreads), 0, stream, xp, pp, tp,
                               begin, end, b, sp, xs);
          else
            hipLaunchKernelGGL((smf_fwd_kernel<NB, decltype(LS)::value, true, false, 2>),
                               dim3(nblocks + xs.blocks), dim3(kThreads), 0, stream, xp, pp, tp,
                               begin, end, b, sp, xs);
        });
      });
      return;
    }
    twoshot_launch(xs, stream);
  }
  MG_DISPATCH_NB(nbp, {
    with_bool(log_sigma, [&](auto LS) { with_bool(has_pop, [&](auto HP) { with_bool(rel_tail, [&](auto RT) {
      hipLaunchKernelGGL((smf_fwd_kernel<NB, decltype(LS)::value, decltype(HP)::value, decltype(RT)::value>),
                         dim3(nblocks), dim3(kThreads), 0, stream, xp, pp, tp, begin, end, b, sp,
                         TwoShotPack{});
    }); }); });
  });
}

void smf_slab_reduce(torch::Tensor slab, int64_t nrows, std::vector<double> edges,
                     std::vector<double> scale, torch::Tensor out) {
  check_dev(slab, "slab", at::kFloat);
  check_dev(out, "out", at::kFloat);
  const int nbp = padded_bins((int)scale.size());
  TORCH_CHECK(slab.numel() >= nrows * nbp, "slab too small");
  TORCH_CHECK(out.numel() >= nbp, "out too small");
  const SmfBins b = make_bins(edges, scale, nbp);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(nbp), dim3(kThreads), 0, stream,
                     slab.data_ptr<float>(), (int)nrows, nbp, b, out.data_ptr<float>());
}

void smf_edge_weights(torch::Tensor g, std::vector<double> edges, std::vector<double> scale,
                      torch::Tensor h) {
  check_dev(g, "g", at::kFloat);
  check_dev(h, "h", at::kFloat);
  const int nb = (int)scale.size();
  const int nbp = padded_bins(nb);
  TORCH_CHECK(g.numel() >= nb && h.numel() >= nbp + 1, "bad sizes");
  const SmfBins b = make_bins(edges, scale, nbp);
  auto stream = at::hip::getCurrentHIPStream();
  // padded edges (e > nb) must get weight 0: zero h first
  hipMemsetAsync(h.data_ptr<float>(), 0, sizeof(float) * (nbp + 1), stream);
  hipLaunchKernelGGL(edge_weights_kernel, dim3(1), dim3(64), 0, stream, g.data_ptr<float>(), nb,
                     b, h.data_ptr<float>());
}

void smf_logmse(torch::Tensor S, torch::Tensor target, double eps, std::vector<double> edges,
                std::vector<double> scale, torch::Tensor loss, torch::Tensor g_out,
                torch::Tensor h) {
  check_dev(S, "S", at::kFloat);
  check_dev(target, "target", at::kFloat);
  check_dev(loss, "loss", at::kFloat);
  check_dev(h, "h", at::kFloat);
  const int nb = (int)scale.size();
  const int nbp = padded_bins(nb);
  TORCH_CHECK(S.numel() >= nb && target.numel() >= nb && h.numel() >= nbp + 1, "bad sizes");
  const SmfBins b = make_bins(edges, scale, nbp);
  auto stream = at::hip::getCurrentHIPStream();
  float* gp = nullptr;
  if (g_out.defined() && g_out.numel()) {
    check_dev(g_out, "g_out", at::kFloat);
    gp = g_out.data_ptr<float>();
  }
  if (nbp > nb) hipMemsetAsync(h.data_ptr<float>(), 0, sizeof(float) * (nbp + 1), stream);
  hipLaunchKernelGGL(logmse_loss_kernel, dim3(1), dim3(64), 0, stream, S.data_ptr<float>(),
                     target.data_ptr<float>(), (float)eps, nb, b, loss.data_ptr<float>(), gp,
                     h.data_ptr<float>());
}

// Fused sumstat epilogue (see smf_epilogue_kernel); peers empty = single rank.
EpiArgs make_epi(torch::Tensor slab, int64_t nrows, int nb, int nbp, torch::Tensor target,
                 double eps, torch::Tensor S, torch::Tensor loss, torch::Tensor h,
                 const std::vector<int64_t>& peers, int64_t rank, int* seq, int* err,
                 double timeout_s, int* adv) {
  check_dev(slab, "slab", at::kFloat);
  check_dev(target, "target", at::kFloat);
  check_dev(S, "S", at::kFloat);
  check_dev(loss, "loss", at::kFloat);
  check_dev(h, "h", at::kFloat);
  TORCH_CHECK(slab.numel() >= nrows * nbp && nrows >= 1, "slab too small");
  TORCH_CHECK(S.numel() >= nbp && target.numel() >= nb && h.numel() >= nbp + 1, "bad sizes");
  TORCH_CHECK(nbp <= kXMaxFloats, "too many bins for the one-shot exchange");
  const int size = peers.empty() ? 1 : (int)peers.size();
  TORCH_CHECK(size <= kXMaxRanks && rank >= 0 && rank < size, "bad rank/size");
  EpiArgs E{};
  for (int r = 0; r < kXMaxRanks; ++r)
    E.peers.base[r] = r < (int)peers.size() ? reinterpret_cast<char*>(peers[r]) : nullptr;
  if (size > 1) TORCH_CHECK(seq != nullptr && err != nullptr, "multi-rank epilogue needs seq/err");
  E.slab = slab.data_ptr<float>();
  E.nrows = (int)nrows;
  E.nb = nb;
  E.rank = (int)rank;
  E.size = size;
  E.on = 1;
  E.seq = reinterpret_cast<unsigned*>(seq);
  E.err = err;
  E.ticks = (long long)(timeout_s * 1e8);
  E.target = target.data_ptr<float>();
  E.eps = (float)eps;
  E.S_out = S.data_ptr<float>();
  E.loss = loss.data_ptr<float>();
  E.h = h.data_ptr<float>();
  E.advance = adv;
  return E;
}

void launch_epilogue(int nbp, const EpiArgs& E, const SmfBins& b, hipStream_t stream) {
  MG_DISPATCH_NB(nbp, {
    hipLaunchKernelGGL((smf_epilogue_kernel<NB>), dim3(1), dim3(kEpiThreads), 0, stream, E, b);
  });
}

void smf_epilogue(torch::Tensor slab, int64_t nrows, std::vector<double> edges,
                  std::vector<double> scale, torch::Tensor target, double eps, torch::Tensor S,
                  torch::Tensor loss, torch::Tensor h, std::vector<int64_t> peers, int64_t rank,
                  c10::optional<torch::Tensor> seq, c10::optional<torch::Tensor> err,
                  double timeout_s, c10::optional<torch::Tensor> advance) {
  int* adv = nullptr;
  if (advance.has_value()) {
    TORCH_CHECK(advance->is_cuda() && advance->scalar_type() == at::kInt, "advance: int32 device");
    adv = advance->data_ptr<int>();
  }
  const int nb = (int)scale.size();
  const int nbp = padded_bins(nb);
  int* sq = (seq.has_value() && seq->defined()) ? seq->data_ptr<int>() : nullptr;
  int* er = (err.has_value() && err->defined()) ? err->data_ptr<int>() : nullptr;
  const EpiArgs E = make_epi(slab, nrows, nb, nbp, target, eps, S, loss, h, peers, rank,
                             peers.size() > 1 ? sq : nullptr, peers.size() > 1 ? er : nullptr,
                             timeout_s, adv);
  const SmfBins b = make_bins(edges, scale, nbp);
  launch_epilogue(nbp, E, b, at::hip::getCurrentHIPStream());
}

void launch_vjp_finalize(const torch::Tensor& giant, const float2* partials, const float2* theta,
                         float2* grad, bool log_sigma, hipStream_t stream) {
  const int64_t ng = giant.numel() / 3;
  if (ng == 0) return;
  check_dev(giant, "giant", at::kInt);
  TORCH_CHECK(partials != nullptr, "partials buffer required");
  with_bool(log_sigma, [&](auto LS) {
    hipLaunchKernelGGL((smf_vjp_finalize_kernel<decltype(LS)::value>), dim3(ng), dim3(kThreads), 0,
                       stream, giant.data_ptr<int32_t>(), partials, theta, grad);
  });
}

// VJP over a tile schedule; grad is interleaved [2 * npop]; partials [nslots * 2].
// exchange: as in smf_forward (the recurrence kernel carries it; the others launch it on
// its own first).
void smf_vjp(torch::Tensor x, c10::optional<torch::Tensor> pop, torch::Tensor theta,
             torch::Tensor tiles, int64_t tile_begin, int64_t tile_end, torch::Tensor h,
             std::vector<double> edges, std::vector<double> scale, bool log_sigma,
             torch::Tensor grad, torch::Tensor partials, torch::Tensor giant,
             std::string exchange) {
  check_dev(x, "x", at::kFloat);
  check_dev(theta, "theta", at::kFloat);
  check_dev(h, "h", at::kFloat);
  check_dev(grad, "grad", at::kFloat);
  check_dev(tiles, "tiles", at::kLong);
  TORCH_CHECK(tiles.size(1) == 4, "tiles must be [ntiles, 4] int64 (32-byte records)");
  const int nbp = padded_bins((int)scale.size());
  TORCH_CHECK(h.numel() >= nbp + 1, "h too small");
  TORCH_CHECK(grad.numel() == theta.numel(), "grad/theta size mismatch");
  const bool has_pop = pop.has_value() && pop->defined();
  if (has_pop) check_dev(*pop, "pop", at::kInt);
  const int64_t ntiles = tile_end - tile_begin;
  TORCH_CHECK(tile_begin >= 0 && tile_end <= tiles.size(0) && ntiles >= 0, "bad tile range");
  const SmfBins b = make_bins(edges, scale, nbp);
  auto stream = at::hip::getCurrentHIPStream();
  const float* xp = x.data_ptr<float>();
  const int32_t* pp = has_pop ? pop->data_ptr<int32_t>() : nullptr;
  const float2* tp = reinterpret_cast<const float2*>(theta.data_ptr<float>());
  const Tile* tl = reinterpret_cast<const Tile*>(tiles.data_ptr<int64_t>()) + tile_begin;
  float2* gp = reinterpret_cast<float2*>(grad.data_ptr<float>());
  float2* pa = partials.numel() ? reinterpret_cast<float2*>(partials.data_ptr<float>()) : nullptr;
  // the recurrence kernel needs uniform, unpadded bins (b.delta > 0) and population ids
  const bool rec = b.delta > 0.0f && has_pop;
  const float* hp = h.data_ptr<float>();
  bool fused = false;
  if (!exchange.empty()) {
    const TwoShotPack xs = twoshot_unpack(exchange);
    fused = rec && xs.mode >= 1 && xs.mode <= 3;
    if (fused) {
      TORCH_CHECK(ntiles + xs.blocks <= INT32_MAX, "bad block count");
      MG_DISPATCH_NB(nbp, {
        with_bool(log_sigma, [&](auto LS) { with_bool(xs.mode == 1, [&](auto UNB) {
          constexpr int XS = decltype(UNB)::value ? 1 : 2;  // unbounded / bounded Adam
          hipLaunchKernelGGL((smf_vjp_tiles_rec_kernel<NB, decltype(LS)::value, XS>),
                             dim3(ntiles + xs.blocks), dim3(kThreads), 0, stream, xp, pp, tp, tl, hp,
                             b, gp, pa, xs);
        }); });
      });
    } else {
      twoshot_launch(xs, stream);
    }
  }
  if (ntiles > 0 && !fused) {
    MG_DISPATCH_NB(nbp, {
      with_bool(log_sigma, [&](auto LS) {
        if (rec)
          hipLaunchKernelGGL((smf_vjp_tiles_rec_kernel<NB, decltype(LS)::value>), dim3(ntiles),
                             dim3(kThreads), 0, stream, xp, pp, tp, tl, hp, b, gp, pa);
        else
          hipLaunchKernelGGL((smf_vjp_tiles_kernel<NB, decltype(LS)::value>), dim3(ntiles),
                             dim3(kThreads), 0, stream, xp, pp, tp, tl, hp, b, gp, pa);
      });
    });
  }
  launch_vjp_finalize(giant, pa, tp, gp, log_sigma, stream);
}

}  // namespace mg
