// SMF kernels over the lanes layout: the lanes forward (with the pipelined Adam update), the
// residual and recompute VJPs, and the pack kernel (model: smf_device.h).
//
// One wavefront per group of 64 population slots, one slot per lane (schedule built by
// runtime.cpp:build_lanes).  Halo j of lane l lives at xi[group_base + 64 j + l]
// (coalesced); lanes shorter than the group are padded with kLaneSentinel, which
// contributes exactly zero everywhere (n -> -huge: Gaussian factor 0, sign bit set on
// every edge so the integer parts cancel, and 0 * finite = 0 in the residuals).
//
// RESID: the forward also keeps, per slot and edge, the Gaussian-factor sums the VJP
// needs -- G_e = sum_i exp2(-w_ie^2) and W_e = sum_i exp2(-w_ie^2) w_ie (w = -n) -- and
// stores them group-major as residuals [ngroups][2 (NB+1)][64] (coalesced, one contiguous
// block per group).  The VJP is then linear in the
// edge weights: A = sum_e h_e G_e, B = sum_e h_e W_e, a memory-bound pass over 22
// floats per population instead of a recomputation over every halo (what jax.vjp does
// with its saved residuals, reference multigrad/multigrad.py:518-532).
#include "smf_device.h"
#include "smf_host.h"

namespace mg {

// Pipelined update (see smf_fwd_lanes_kernel<..., UPD>): the previous step's residual
// VJP + Adam of a population run in the lane that is about to evaluate the population's
// halos at the new parameters.  BND (bounded fits, reference multigrad/adam.py:133-189):
// Adam runs on the unbounded coordinates u (indexed like m, v), the gradient is scaled by
// the diagonal dp/du (at u, or at the old p with the reference's legacy Jacobian, SURVEY
// Q1) and the forward evaluates p = T^-1(u) (csrc/adam.h); the bound kind of a coordinate
// follows from which of its bounds are finite.
struct LanesUpdate {
  const float* h;       // edge weights of the previous step (NB+1)
  float2* theta_w;      // parameters, updated in place (same array the kernel reads)
  float2* m;            // Adam moments, indexed by unit - unit_offset
  float2* v;
  float* traj;          // trajectory base or null (row r at traj + r * traj_stride)
  int64_t traj_stride;
  int64_t unit_offset;
  const int* step;      // device step counter (read when host_step < 0)
  int host_step;
  float lr, b1, b2, eps;
  float2* u;            // BND: unbounded coordinates (indexed like m, v)
  const float2* lo;     // BND: bounds, -inf / +inf where absent (indexed like m, v)
  const float2* hi;
  int legacy;           // BND: dp/du at the old p (reference quirk Q1)
};

// dp/du and p = T^-1(u) of csrc/adam.h with hardware reciprocals (v_rcp / v_rsq, ~1 ulp)
// instead of IEEE divisions (~10 VALU ops each, three per coordinate): the update runs in the
// VALU-bound forward, where they measured 480 vs 440 us per step (the stand-alone bounded
// Adam keeps the exact forms; the two schedules agree to a few ulps, as the unbounded
// pipelined update's reciprocal bias corrections do).  What the bounded update costs
// (profiles/bounded_r5/): 1.72e8 vs 1.63e8 VALU wave instructions per step, ~115 per lane
// group, a third of them SGPR spill traffic (v_readlane / v_writelane) around the group
// transition; a wave-uniform fast path for all-both-bounded waves measured no faster.
__device__ __forceinline__ float dpdu_fast(float at, float lo, float hi, int8_t k) {
  if (k == kBoth) {
    const float r = at * __builtin_amdgcn_rcpf((hi - lo) * (1.0f / kPi));
    return __builtin_amdgcn_rcpf(fmaf(r, r, 1.0f));
  }
  if (k == kLow || k == kHigh) {
    const float x = fmaf(at, at, 4.0f);
    const float rs = __builtin_amdgcn_rsqf(x);
    // towards the bound: h/r with h = 2/(r + |at|), r = x * rs (no cancellation, as adam.h)
    if (k == kLow ? at < 0.0f : at > 0.0f)
      return 2.0f * __builtin_amdgcn_rcpf(fmaf(x, rs, fabsf(at))) * rs;
    const float q = at * rs;
    return 0.5f * (k == kLow ? 1.0f + q : 1.0f - q);
  }
  return 1.0f;
}

__device__ __forceinline__ float inv_transform_fast(float u, float lo, float hi, int8_t k) {
  if (k == kBoth) {
    const float s = (hi - lo) * (1.0f / kPi);
    const float p = fmaf(s, atanf(u * __builtin_amdgcn_rcpf(s)), (hi + lo) * 0.5f);
    return fminf(fmaxf(p, lo), hi);  // stays in the box, as adam.h
  }
  // one-sided: the distance to the bound is 2/(sqrt(u^2+4) + |u|) on the side towards it
  if (k == kLow) {
    const float r = __builtin_amdgcn_sqrtf(fmaf(u, u, 4.0f));
    return u < 0.0f ? fmaf(2.0f, __builtin_amdgcn_rcpf(r - u), lo) : 0.5f * (2.0f * lo + u + r);
  }
  if (k == kHigh) {
    const float r = __builtin_amdgcn_sqrtf(fmaf(u, u, 4.0f));
    return u > 0.0f ? fmaf(-2.0f, __builtin_amdgcn_rcpf(r + u), hi) : 0.5f * (2.0f * hi + u - r);
  }
  return u;
}

// Edge-pair packing: the NB+1 edges of ONE halo are evaluated two at a time in packed
// fp32 (v_pk_fma / v_pk_mul / v_pk_add on (edge 2i, edge 2i+1)), so every per-edge sum --
// the signed-tail accumulator and the two residual sums -- is itself a register pair and
// accumulates with one packed instruction, with no cross-lane shuffles or moves.  With an
// odd edge count the last edge of the two halos of an unrolled pair forms the remaining
// pair (its accumulators keep one partial per halo, folded once at the end).
// Packed per pair: the edge fma, w^2, the Horner chain, the accumulate and both residual
// updates; per element: |w|+K, v_rcp, v_exp, the sign (v_bfi) and the count compare.
// (EdgePairs<NB>: the edge-pair layout, defined in smf_device.h)

template <int NB, bool REL, bool RESID>
__device__ __forceinline__ void ep_eval(v2f n, v2f (&acc)[EdgePairs<NB>::NV],
                                        v2f (&G)[EdgePairs<NB>::NV], v2f (&W)[EdgePairs<NB>::NV],
                                        int i, int& ca, int& cb) {
  v2f p, g;
  normal_tail_parts_w2<REL>(n, p, g);
  v2f sg;
  sg.x = __builtin_copysignf(g.x, n.x);
  sg.y = __builtin_copysignf(g.y, n.y);
  acc[i] = p * sg + acc[i];
  ca += __builtin_popcountll(__builtin_amdgcn_ballot_w64(n.x < 0.0f));
  cb += __builtin_popcountll(__builtin_amdgcn_ballot_w64(n.y < 0.0f));
  if constexpr (RESID) {
    G[i] = G[i] + g;
    W[i] = (-g) * n + W[i];
  }
}

template <int NB, bool RESID, int REPL>
__device__ __forceinline__ void ep_eval_tab(v2f n, const float4* __restrict__ tb,
                                            v2f (&acc)[EdgePairs<NB>::NV],
                                            v2f (&G)[EdgePairs<NB>::NV], v2f (&W)[EdgePairs<NB>::NV],
                                            int i, int& ca, int& cb) {
  constexpr float kLo = -(float)(kTailTabN / 2);
  constexpr float kHi = (float)(kTailTabN / 2) - 1.0f / 4096;
  v2f t = n * kTailTabInvH;
  t.x = __builtin_amdgcn_fmed3f(t.x, kLo, kHi);
  t.y = __builtin_amdgcn_fmed3f(t.y, kLo, kHi);
  const float4 cx = tb[cvt_flr_i32(t.x) * REPL];
  const float4 cy = tb[cvt_flr_i32(t.y) * REPL];
  const float sx = __builtin_amdgcn_fractf(t.x);
  const float sy = __builtin_amdgcn_fractf(t.y);
  // scalar Horner on purpose: packing the two chains would need a v_mov per operand pair
  // (the coefficients of the two elements come from different table reads)
  v2f v;
  v.x = fma_scalar(fma_scalar(fma_scalar(cx.w, sx, cx.z), sx, cx.y), sx, cx.x);
  v.y = fma_scalar(fma_scalar(fma_scalar(cy.w, sy, cy.z), sy, cy.y), sy, cy.x);
  acc[i] = acc[i] + v;
  ca += __builtin_popcountll(__builtin_amdgcn_ballot_w64(t.x < 0.0f));
  cb += __builtin_popcountll(__builtin_amdgcn_ballot_w64(t.y < 0.0f));
  if constexpr (RESID) {
    const v2f e = -n * n;
    v2f g;
    g.x = fast_exp2(e.x);
    g.y = fast_exp2(e.y);
    G[i] = G[i] + g;
    W[i] = (-g) * n + W[i];
  }
}

template <int NB, bool LOGSIG, bool REL, bool RESID, int REPL = 0>
__device__ __forceinline__ void lane_halo_ep(float x0, float x1, float ninv, float mua,
                                             const SmfBins& b,
                                             v2f (&acc)[EdgePairs<NB>::NV], int (&cnt)[NB + 1],
                                             v2f (&G)[EdgePairs<NB>::NV],
                                             v2f (&W)[EdgePairs<NB>::NV],
                                             const float4* tb = nullptr) {
  using E = EdgePairs<NB>;
  auto eval = [&](v2f n, int i, int& ca, int& cb) {
    if constexpr (REPL > 0)
      ep_eval_tab<NB, RESID, REPL>(n, tb, acc, G, W, i, ca, cb);
    else
      ep_eval<NB, REL, RESID>(n, acc, G, W, i, ca, cb);
  };
  const float mu0 = fmaf(x0, -ninv, mua);
  const float mu1 = fmaf(x1, -ninv, mua);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float mu = h ? mu1 : mu0;
#pragma unroll
    for (int i = 0; i < E::NP; ++i) {
      v2f e2;
      e2.x = b.edge[2 * i];
      e2.y = b.edge[2 * i + 1];
      const v2f n = e2 * ninv + mu;
      eval(n, i, cnt[2 * i], cnt[2 * i + 1]);
    }
  }
  if constexpr (E::NX) {
    v2f m2;
    m2.x = mu0;
    m2.y = mu1;
    const v2f n = (v2f)(b.edge[E::NE - 1] * ninv) + m2;
    int c2 = 0;
    eval(n, E::NP, cnt[E::NE - 1], c2);
    cnt[E::NE - 1] += c2;
  }
}

// Keep the scheduler from interleaving consecutive halos (their
// temporaries would double the register footprint of the pipelined-update kernel)
template <int NB, bool RESID, bool A5 = true>
__device__ __forceinline__ void lane_halo_em(float x, const EmLane& L, float nma,
                                             const SmfBins& b, v2f (&F)[EdgePairs<NB>::NV],
                                             v2f (&Wa)[EdgePairs<NB>::NV],
                                             v2f (&E)[EdgePairs<NB>::NV]) {
  em_halo<NB, RESID, false, A5>(fmaf(x, -L.inv, nma), L.inv, L.dw4, L.a1, L.a3, L.a5, b, F, Wa, E);
  __builtin_amdgcn_sched_barrier(0);
}

// Measured on MI355X (1e7 params, 1.34e8 halos, internal order, with residuals): the
// edge-pair path at 4 waves/SIMD (118 VGPRs, no spills) 595 us vs 615-624 us for the
// compiler-packed scalar path at 6 waves; at 5 or 6 waves the edge-pair path spills.
// The Euler-Maclaurin residual forwards evaluate a group outside the EM range by an
// out-of-line per-edge call inside the main launch (LMODE 3): full machine parallelism at
// any out-of-range fraction, no fix-up launch, no list atomics.  Measured and removed in
// round 5 (docs/design.md "Open performance items"): the inline per-edge fallback (LMODE 0
// with residuals: it costs the hot loop registers and spills), the round-3 deferral list +
// narrow fix-up launch (LMODE 1 + 2), and the sumstat epilogue folded into the last
// workgroup of the lanes forward (headline 0.4352-0.4357 vs 0.4352-0.4364 ms/step, owner
// proxy 0.0626-0.0628 vs 0.0618-0.0619: not faster than its own one-workgroup launch).
constexpr int kLanesMainMode = 3;

// Two-term Euler-Maclaurin groups (kEmH2) in the lanes forward: 1 = on (default), 0 = off
#ifndef MG_EM2
#define MG_EM2 1
#endif

// Minimum resident waves per SIMD of the lanes forward: the edge-pair path needs up to 128
// VGPRs (4 waves/SIMD) to avoid spills; at 5 or 6 waves it spills.
#ifndef MG_LANES_MINWAVES
#define MG_LANES_MINWAVES 4
#endif
#ifndef MG_LANES_UNROLL
#define MG_LANES_UNROLL 2
#endif
constexpr int kLanesUnroll = MG_LANES_UNROLL;

// The lanes kernel addresses xi, slot_pop and the residuals through buffer
// descriptors (4 SGPRs, rebuilt per group) and one 32-bit lane offset, instead of the 64-bit
// per-lane pointers the compiler otherwise hoists into VGPR pairs (two VGPRs each): that is
// what the pipelined-update instantiation needs to stay within 128 VGPRs without spills.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p) {
  // raw buffer, stride 0; range 2 GB from the base (every access is base + lane*4 + small)
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ float buf_load_f32(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ int buf_load_i32(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  return (int)__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
}
__device__ __forceinline__ void buf_store_f32(__amdgpu_buffer_rsrc_t r, int voff, int soff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, 0);
}

// Halo j of a lane (sentinel past the end).  The load is a buffer load at a wave-uniform
// row offset; an unconditional load with the select at the use measured no faster and was
// removed in round 5.
struct LaneSrc {  // this group's halos: descriptor at the group base, lane byte offset
  __amdgpu_buffer_rsrc_t r;
  int voff;
};
__device__ __forceinline__ float lane_load(const LaneSrc& xp, int j, int len) {
  return j < len ? buf_load_f32(xp.r, xp.voff, j * kWave * 4) : kLaneSentinel;
}

// Diagnostics build (-DMG_FWD_TRACE): every wavefront of the lanes forward records its
// start / end time (s_memrealtime, 100 MHz) and its group count, read back with
// smf_fwd_trace(); used to split a launch's time into dispatch skew, work and tail.
#ifdef MG_FWD_TRACE
constexpr int kTraceWaves = 16384;
__device__ unsigned long long g_fwd_trace[3 * kTraceWaves];
#endif

// LMODE 3: ONE whole lanes group by per-edge tails (the groups outside the Euler-Maclaurin
// range), out of line.  The main kernel's registers are sized by its hot EM loop; a call
// keeps this path's live ranges out of that allocation (the callee saves what it clobbers,
// on the cold path only), where the inline fallback cost spills (126 VGPRs, 8 spilled) and
// the deferral list of round 3 ran the out-of-range groups on a narrow fix-up launch.
// Per-edge accumulators in the edge-pair layout of lane_halo_ep (signed tails, wave counts
// by ballot); the residuals G, W are stored here, in the group-major layout of the kernel.
template <int NB>
struct LaneGroupSums {
  v2f acc[EdgePairs<NB>::NV];
  int cnt[NB + 1];
};

template <int NB>
__device__ __attribute__((noinline)) LaneGroupSums<NB> lanes_group_exact(
    const float* __restrict__ xg, int len, float x0, float x1, float ninv, float mua, float e0,
    float delta, float* __restrict__ rg) {
  using EP = EdgePairs<NB>;
  const int lane = threadIdx.x & (kWave - 1);
  // uniform edges from (e0, delta) in registers: a reference to the kernel's SmfBins would
  // make the kernel copy the whole struct to private memory at its start
  SmfBins b;
#pragma unroll
  for (int e = 0; e <= NB; ++e) b.edge[e] = fmaf((float)e, delta, e0);
  LaneGroupSums<NB> o;
  v2f G[EP::NV], W[EP::NV];
#pragma unroll
  for (int i = 0; i < EP::NV; ++i) {
    o.acc[i] = (v2f)(0.0f);
    G[i] = (v2f)(0.0f);
    W[i] = (v2f)(0.0f);
  }
#pragma unroll
  for (int e = 0; e <= NB; ++e) o.cnt[e] = 0;
  // two halos per iteration with the next pair's loads in flight: buffer loads at a wave-
  // uniform row offset, unconditional (the rows past a group's end belong to the next group
  // or to the 16 padding rows of xi) and masked to the sentinel at the use; the first pair
  // (x0, x1) comes from the caller, which loaded it with the group
  const __amdgpu_buffer_rsrc_t xr = buf_rsrc(xg);
  const int voff = lane * 4;
  for (int j = 0; j < len; j += 2) {
    const float c0 = x0;
    const float c1 = j + 1 < len ? x1 : kLaneSentinel;
    x0 = buf_load_f32(xr, voff, (j + 2) * kWave * 4);
    x1 = buf_load_f32(xr, voff, (j + 3) * kWave * 4);
    lane_halo_ep<NB, true, false, true>(c0, c1, ninv, mua, b, o.acc, o.cnt, G, W);
  }
  float Gs[NB + 1], Ws[NB + 1];
#pragma unroll
  for (int i = 0; i < EP::NP; ++i) {
    Gs[2 * i] = G[i].x;
    Gs[2 * i + 1] = G[i].y;
    Ws[2 * i] = W[i].x;
    Ws[2 * i + 1] = W[i].y;
  }
  if constexpr (EP::NX) {
    Gs[NB] = G[EP::NP].x + G[EP::NP].y;
    Ws[NB] = W[EP::NP].x + W[EP::NP].y;
  }
  const __amdgpu_buffer_rsrc_t rr = buf_rsrc(rg);
#pragma unroll
  for (int e = 0; e <= NB; ++e) {
    buf_store_f32(rr, voff, e * kWave * 4, Gs[e]);
    buf_store_f32(rr, voff, (NB + 1 + e) * kWave * 4, Ws[e]);
  }
  return o;
}

// LMODE: 0 = plain (forwards without residuals: Euler-Maclaurin where the group is in
// range, inline per-edge tails otherwise); 3 = CALL (EM residual forwards): a group outside
// the EM range is evaluated by lanes_group_exact, out of line -- an inline fallback cost
// ~3.5% of the headline step in registers although the headline data never takes it
// (profiles/em_forward/); 4 = PER-EDGE: no EM path, every group by the packed two-halo
// per-edge tails, for shards where most lane groups are outside the EM range anyway.
template <int NB, bool LOGSIG, bool REL, bool RESID, bool UPD = false, int LMODE = 0,
          bool BND = false>
__global__ __launch_bounds__(kThreads, MG_LANES_MINWAVES) void smf_fwd_lanes_kernel(
    const float* __restrict__ xi, const int32_t* __restrict__ slot_pop,
    const int64_t* __restrict__ group_base, const int32_t* __restrict__ group_len,
    const int32_t* __restrict__ fwd_order, const float2* __restrict__ theta, int64_t g0,
    int64_t g1, SmfBins bins, float* __restrict__ slab, float* __restrict__ resid,
    const int32_t* __restrict__ wave_start, int* __restrict__ queues, int nq,
    LanesUpdate upd = LanesUpdate{}) {
  static_assert(!UPD || RESID, "the pipelined update reads the residuals it overwrites");
  static_assert(!BND || UPD, "bounds belong to the pipelined update");
  static_assert(LMODE == 0 || LMODE == 3 || LMODE == 4, "lanes mode");
  static_assert(LMODE != 3 || (RESID && !REL), "CALL: EM residual forwards");
  // signed-tail table (absolute contract, per-edge forwards without residuals): 16
  // replicas (conflict-free reads), 8 next to the pipelined update's staging buffer (LDS
  // budget of 4 workgroups per CU); with the EM path the fallback is the lean per-edge path
  constexpr bool kEmOn = LMODE != 4;
  constexpr int kRepl = (!REL && !kEmOn && !RESID) ? (UPD ? 8 : 16) : 0;
  constexpr bool kEm = kEmOn && !REL;
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
  for (int k = 0; k <= NB; ++k) {
    acc[k] = 0.0f;
    cnt[k] = 0;
  }
  using EP = EdgePairs<NB>;
  static_assert(kLanesUnroll % 2 == 0, "edge-pair path takes halos two at a time");
  v2f accp[EP::NV];
#pragma unroll
  for (int k = 0; k < EP::NV; ++k) accp[k] = (v2f)(0.0f);
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (kThreads / kWave);
  // Software pipeline across groups as well as within one: the next group's parameters
  // and first halos are loaded *before* this group's residual stores (so the in-order
  // memory counter never makes the next group wait for those stores), and the slot ->
  // population index is fetched one group further ahead, so the dependent theta gather
  // does not wait for a load issued in the same transition.
  // Work list: with wave_start (host LPT schedule, runtime.cpp:lpt_waves) wave w takes
  // positions [wave_start[w], wave_start[w+1]) of its own list; otherwise positions
  // k in [g0, g1) of the longest-first order, grid-strided.  g = fwd_order[k].
  const int64_t w_id = (int64_t)blockIdx.x * (kThreads / kWave) + wid;
#ifdef MG_FWD_TRACE
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
  int n_groups_done = 0;
#endif
  // Dynamic (queues != null): nq work queues, queue q holding positions q, q + nq, ... of
  // the longest-first order; the waves of block b draw from queue b % nq through an atomic
  // ticket, one group ahead.  Issue arbitration favours the oldest wave of a SIMD, so
  // waves with equal static loads finish up to 3x apart and the youngest runs the tail
  // alone (tools/fwd_trace.py); drawing work dynamically lets the fast waves take more.
  // Every wave makes exactly one failing draw, so draw n_q + waves_q - 1 is the queue's
  // last of the launch and resets it (graph-replay safe, no extra atomics).
  const bool dyn = queues != nullptr;
  const int qid = dyn ? (int)(blockIdx.x % nq) : 0;
  const int n_items = (int)(g1 - g0);
  const int n_q = dyn && qid < n_items ? (n_items - qid + nq - 1) / nq : 0;
  const int waves_q = dyn ? (kThreads / kWave) * (int)((gridDim.x - qid + nq - 1) / nq) : 0;
  auto draw = [&]() -> int64_t {
    int t = 0;
    if (lane == 0) {
      t = atomicAdd(queues + qid, 1);
      if (t == n_q + waves_q - 1)
        __hip_atomic_store(queues + qid, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    t = __builtin_amdgcn_readfirstlane(t);
    return t < n_q ? g0 + qid + (int64_t)t * nq : g1;
  };
  int64_t k = dyn ? draw() : wave_start ? (int64_t)wave_start[w_id] : g0 + w_id;
  const int64_t kstride = wave_start ? 1 : nwaves;
  if (wave_start && !dyn) g1 = wave_start[w_id + 1];
  int64_t k_next = g1;
  int64_t g = 0;
  float2 th = make_float2(0.f, 0.f);
  const int lane4 = lane * 4;
  LaneSrc xp{buf_rsrc(xi), lane4};
  auto slot_of = [&](int64_t kk) {
    return buf_load_i32(buf_rsrc(slot_pop + (int64_t)fwd_order[kk] * kWave), lane4, 0);
  };
  int len = 0;
  int c_next = 0;
  int c_cur = -1;
  float xn[kLanesUnroll];
  float ubc1 = 1.0f, ubc2 = 1.0f;  // UPD: 1 / (1 - b^t)
  float* utrow = nullptr;
  if constexpr (UPD) {
    const int st = upd.host_step >= 0
                       ? upd.host_step
                       : __hip_atomic_load(upd.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // reciprocal bias corrections (uniform): the per-population update below is multiply /
    // v_rcp / v_sqrt instead of three IEEE divisions per parameter (~30 VALU ops each),
    // within an ulp or two of the division form (csrc/adam.hip, the stand-alone kernels)
    ubc1 = 1.0f / bias_correction(upd.b1, st + 1);
    ubc2 = 1.0f / bias_correction(upd.b2, st + 1);
    if (upd.traj) utrow = upd.traj + (int64_t)(st + 1) * upd.traj_stride;
  }
  // UPD: the update inputs of a group (its residual block, 1 KB per dwordx4 instruction, and
  // the lanes' Adam moments) are staged into this wave's LDS slice by global_load_lds when
  // the group is loaded -- no VGPRs (the 64-bit per-lane pointers of a register load spill
  // this kernel), and they travel with the theta gather and the first halos, so the group
  // transition still costs one memory round trip.
  // rows: G[NB+1], W[NB+1], m.x m.y v.x v.y (BND: + u.x u.y lo.x lo.y hi.x hi.y)
  constexpr int kUR = UPD ? 2 * (NB + 1) + 4 + (BND ? 6 : 0) : 1;
  float* ubuf = nullptr;
  const float* uh = nullptr;  // the edge weights, in LDS (a vector load of them would be
                              // counted by vmcnt and make every group wait for its stores)
  if constexpr (UPD) {
    __shared__ __attribute__((aligned(16))) float ub[(kThreads / kWave) * kUR * kWave];
    __shared__ float hs[NB + 1];
    if (threadIdx.x <= NB) hs[threadIdx.x] = upd.h[threadIdx.x];
    __syncthreads();
    ubuf = ub + wid * (kUR * kWave);
    uh = hs;
  }
  auto stage_update = [&](int64_t gg, int c) {
    if constexpr (UPD) {
      constexpr int NR = 2 * (NB + 1);  // residual rows, contiguous in global memory
      lds_stage_block<NR>(resid + gg * (NR * kWave), ubuf, lane);
      const int64_t j = c < 0 ? 0 : c - upd.unit_offset;
      const float* mp = reinterpret_cast<const float*>(upd.m + j);
      const float* vp = reinterpret_cast<const float*>(upd.v + j);
      __builtin_amdgcn_global_load_lds(mp, ubuf + NR * kWave, 4, 0, 0);
      __builtin_amdgcn_global_load_lds(mp + 1, ubuf + (NR + 1) * kWave, 4, 0, 0);
      __builtin_amdgcn_global_load_lds(vp, ubuf + (NR + 2) * kWave, 4, 0, 0);
      __builtin_amdgcn_global_load_lds(vp + 1, ubuf + (NR + 3) * kWave, 4, 0, 0);
      if constexpr (BND) {
        const float* up = reinterpret_cast<const float*>(upd.u + j);
        const float* lp = reinterpret_cast<const float*>(upd.lo + j);
        const float* hp = reinterpret_cast<const float*>(upd.hi + j);
        __builtin_amdgcn_global_load_lds(up, ubuf + (NR + 4) * kWave, 4, 0, 0);
        __builtin_amdgcn_global_load_lds(up + 1, ubuf + (NR + 5) * kWave, 4, 0, 0);
        __builtin_amdgcn_global_load_lds(lp, ubuf + (NR + 6) * kWave, 4, 0, 0);
        __builtin_amdgcn_global_load_lds(lp + 1, ubuf + (NR + 7) * kWave, 4, 0, 0);
        __builtin_amdgcn_global_load_lds(hp, ubuf + (NR + 8) * kWave, 4, 0, 0);
        __builtin_amdgcn_global_load_lds(hp + 1, ubuf + (NR + 9) * kWave, 4, 0, 0);
      }
    }
  };
  // previous step's VJP of the current group's populations from the staged residuals, then
  // Adam: the halos are evaluated at the updated parameters
  auto apply_update = [&]() {
    if constexpr (UPD) {
      constexpr int NR = 2 * (NB + 1);
      float A = 0.0f, B = 0.0f;
#pragma unroll
      for (int e = 0; e <= NB; ++e) {
        A = fmaf(uh[e], ubuf[e * kWave + lane], A);
        B = fmaf(uh[e], ubuf[(NB + 1 + e) * kWave + lane], B);
      }
      if (c_cur >= 0) {
        const float2 gr = pop_grad<LOGSIG>(th, A, B);
        const int64_t j = c_cur - upd.unit_offset;
        float2 mm = make_float2(ubuf[NR * kWave + lane], ubuf[(NR + 1) * kWave + lane]);
        float2 vv = make_float2(ubuf[(NR + 2) * kWave + lane], ubuf[(NR + 3) * kWave + lane]);
        if constexpr (BND) {
          float2 uu = make_float2(ubuf[(NR + 4) * kWave + lane], ubuf[(NR + 5) * kWave + lane]);
          const float2 lo = make_float2(ubuf[(NR + 6) * kWave + lane], ubuf[(NR + 7) * kWave + lane]);
          const float2 hi = make_float2(ubuf[(NR + 8) * kWave + lane], ubuf[(NR + 9) * kWave + lane]);
          const int8_t kx = bound_kind(lo.x, hi.x), ky = bound_kind(lo.y, hi.y);
          const float gx = gr.x * dpdu_fast(upd.legacy ? th.x : uu.x, lo.x, hi.x, kx);
          const float gy = gr.y * dpdu_fast(upd.legacy ? th.y : uu.y, lo.y, hi.y, ky);
          mm.x = (1.0f - upd.b1) * gx + upd.b1 * mm.x;
          mm.y = (1.0f - upd.b1) * gy + upd.b1 * mm.y;
          vv.x = (1.0f - upd.b2) * (gx * gx) + upd.b2 * vv.x;
          vv.y = (1.0f - upd.b2) * (gy * gy) + upd.b2 * vv.y;
          uu.x -= upd.lr * (mm.x * ubc1) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(vv.x * ubc2) + upd.eps);
          uu.y -= upd.lr * (mm.y * ubc1) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(vv.y * ubc2) + upd.eps);
          th.x = inv_transform_fast(uu.x, lo.x, hi.x, kx);
          th.y = inv_transform_fast(uu.y, lo.y, hi.y, ky);
          upd.u[j] = uu;
        } else {
          mm.x = (1.0f - upd.b1) * gr.x + upd.b1 * mm.x;
          mm.y = (1.0f - upd.b1) * gr.y + upd.b1 * mm.y;
          vv.x = (1.0f - upd.b2) * (gr.x * gr.x) + upd.b2 * vv.x;
          vv.y = (1.0f - upd.b2) * (gr.y * gr.y) + upd.b2 * vv.y;
          th.x -= upd.lr * (mm.x * ubc1) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(vv.x * ubc2) + upd.eps);
          th.y -= upd.lr * (mm.y * ubc1) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(vv.y * ubc2) + upd.eps);
        }
        upd.m[j] = mm;
        upd.v[j] = vv;
        upd.theta_w[c_cur] = th;
        if (utrow) reinterpret_cast<float2*>(utrow)[j] = th;
      }
    }
  };
  auto fetch_next_slot = [&]() {
    if (k_next < g1) c_next = slot_of(k_next);
  };
  auto load_group = [&](int64_t kk, int c, bool fetch_next = true) {
    g = fwd_order[kk];
    c_cur = c;
    stage_update(g, c);
    th = theta[c < 0 ? 0 : c];
    xp.r = buf_rsrc(xi + group_base[g]);
    len = group_len[g];
#pragma unroll
    for (int u = 0; u < kLanesUnroll; ++u) xn[u] = lane_load(xp, u, len);
    k_next = dyn ? draw() : kk + kstride;
    if (fetch_next) fetch_next_slot();
  };
  if (k < g1) {
    load_group(k, slot_of(k), !UPD);
    if constexpr (UPD) {
      vmem_wait_all();
      apply_update();
      fetch_next_slot();
    }
  }
  const int64_t k_first = k;
  while (k < g1) {
    // Static lists: the wave's issue priority falls as its list drains, so the SIMD's
    // arbiter prefers the waves that are behind instead of always the oldest one (which
    // leaves the youngest wave running the tail alone, profiles/fwd_wave_timeline.md).
    if (!dyn && wave_start) {
      const int64_t tot = g1 - k_first;
      const int lvl = (int)((4 * (g1 - k) - 1) / tot);
      if (lvl >= 3) __builtin_amdgcn_s_setprio(3);
      else if (lvl == 2) __builtin_amdgcn_s_setprio(2);
      else if (lvl == 1) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    const int64_t gc = g;
    const float ninv = -inv_sigma<LOGSIG>(th.y) * kWScale;
    const float mua = -th.x * ninv;
    v2f Gp[EP::NV], Wp[EP::NV];
#pragma unroll
    for (int e = 0; e < EP::NV; ++e) {
      Gp[e] = (v2f)(0.0f);
      Wp[e] = (v2f)(0.0f);
    }
    // Euler-Maclaurin path (see em_halo) when every occupied lane's bin width is inside
    // kEmHMax; the ballot makes the choice wave-uniform
    bool em = false, em2 = false;
    if constexpr (kEm) {
      const float inv = -ninv;
      const float h = bins.delta * inv * (1.0f / kWScale);
      const bool bad = c_cur >= 0 && !(h <= kEmHMax);
      em = bins.delta > 0.0f && __builtin_amdgcn_ballot_w64(bad) == 0;
#if MG_EM2
      em2 = em && __builtin_amdgcn_ballot_w64(c_cur >= 0 && !(h <= kEmH2)) == 0;
#endif
    }
    if constexpr (kEm) if (em) {
      const EmLane eml = em2 ? em_lane2(-ninv, bins.delta) : em_lane(-ninv, bins.delta);
      v2f Ep[EP::NV];
#pragma unroll
      for (int e = 0; e < EP::NV; ++e) Ep[e] = (v2f)(0.0f);
      auto em_loop = [&](auto a5c) {
        for (int j = 0; j < len; j += kLanesUnroll) {
          float xc[kLanesUnroll];
#pragma unroll
          for (int u = 0; u < kLanesUnroll; ++u) {
            xc[u] = xn[u];
            xn[u] = lane_load(xp, j + kLanesUnroll + u, len);
          }
#pragma unroll
          for (int u = 0; u < kLanesUnroll; ++u)
            lane_halo_em<NB, RESID, decltype(a5c)::value>(xc[u], eml, -mua, bins, Gp, Wp, Ep);
        }
      };
      if (em2) em_loop(std::false_type{});   // two-term EM (the group's h <= kEmH2)
      else em_loop(std::true_type{});
      em_group_end<NB>(eml, Gp, Wp, Ep, accp);
    }
    // the next kLanesUnroll loads are in flight while the current halos are computed;
    // past-the-end halos are the sentinel (exact zero contribution)
    if constexpr (LMODE == 3) {
      if (!em) {  // outside the EM range: per-edge tails, out of line (stores the residuals)
        const LaneGroupSums<NB> o = lanes_group_exact<NB>(
            xi + group_base[gc], len, xn[0], xn[1], ninv,
            mua, bins.edge[0], bins.delta,
            resid + gc * (2 * (NB + 1) * kWave));
#pragma unroll
        for (int i = 0; i < EP::NV; ++i) accp[i] = accp[i] + o.acc[i];
#pragma unroll
        for (int e = 0; e <= NB; ++e) cnt[e] += __builtin_amdgcn_readfirstlane(o.cnt[e]);
      }
    } else
    if (!em)
    for (int j = 0; j < len; j += kLanesUnroll) {
      float xc[kLanesUnroll];
#pragma unroll
      for (int u = 0; u < kLanesUnroll; ++u) {
        xc[u] = xn[u];
        const int jn = j + kLanesUnroll + u;
        xn[u] = lane_load(xp, jn, len);
      }
      if constexpr (kEm) {  // lean fallback of the Euler-Maclaurin kernels
#pragma unroll
        for (int u = 0; u < kLanesUnroll; ++u)
          lane_halo_exact1<NB, RESID>(xc[u], ninv, mua, bins, accp, cnt, Gp, Wp);
      } else {
#pragma unroll
        for (int u = 0; u < kLanesUnroll; u += 2)
          lane_halo_ep<NB, LOGSIG, REL, RESID, kRepl>(xc[u], xc[u + 1], ninv, mua, bins, accp,
                                                      cnt, Gp, Wp, tb);
      }
    }
    const int64_t kn = k_next;
#ifdef MG_FWD_TRACE
    ++n_groups_done;
#endif
    if constexpr (!UPD)
      if (kn < g1) load_group(kn, c_next);
    // group-major [g][2 (NB+1)][64]: one block per group (LMODE 3: the groups outside the
    // EM range are stored by lanes_group_exact).  Plain stores: non-temporal ones measured
    // no faster and were removed in round 5.
    if (RESID && (LMODE != 3 || em)) {
      const __amdgpu_buffer_rsrc_t rr = buf_rsrc(resid + gc * (2 * (NB + 1) * kWave));
      float G[NB + 1], W[NB + 1];
#pragma unroll
      for (int i = 0; i < EP::NP; ++i) {
        G[2 * i] = Gp[i].x;
        G[2 * i + 1] = Gp[i].y;
        W[2 * i] = Wp[i].x;
        W[2 * i + 1] = Wp[i].y;
      }
      if constexpr (EP::NX) {
        G[NB] = Gp[EP::NP].x + Gp[EP::NP].y;
        W[NB] = Wp[EP::NP].x + Wp[EP::NP].y;
      }
#pragma unroll
      for (int e = 0; e <= NB; ++e) {
        buf_store_f32(rr, lane4, e * kWave * 4, G[e]);
        buf_store_f32(rr, lane4, (NB + 1 + e) * kWave * 4, W[e]);
      }
    }
    k = kn;
    // UPD: the next group is loaded after the stores, and everything is waited for before
    // the staged inputs are read (the compiler does not track global_load_lds): the stores
    // went out first, so the wait is the one round trip the first halos need anyway
    if constexpr (UPD) {
      if (k < g1) {
        load_group(k, c_next, false);
        vmem_wait_all();
        apply_update();
        fetch_next_slot();  // after the wait: it is not needed before the next transition
      }
    }
  }
#pragma unroll
  for (int i = 0; i < EP::NP; ++i) {
    acc[2 * i] = accp[i].x;
    acc[2 * i + 1] = accp[i].y;
  }
  if constexpr (EP::NX) acc[NB] = accp[EP::NP].x + accp[EP::NP].y;
#ifdef MG_FWD_TRACE
  if (lane == 0 && w_id < kTraceWaves) {
    g_fwd_trace[3 * w_id] = t_start;
    g_fwd_trace[3 * w_id + 1] = __builtin_amdgcn_s_memrealtime();
    g_fwd_trace[3 * w_id + 2] = (unsigned long long)n_groups_done;
  }
#endif
  const bool counter = lane == 0;  // the counts are per wave: fold them in once
#pragma unroll
  for (int k = 0; k < NB; ++k)
    acc[k] = (acc[k + 1] - acc[k]) + (counter ? (float)(cnt[k + 1] - cnt[k]) : 0.0f);
  __shared__ float scratch[NB * (kThreads / kWave)];
  float(&bin)[NB] = *reinterpret_cast<float(*)[NB]>(acc);
  block_sum_n<NB>(bin, scratch);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NB; ++k) slab[(int64_t)blockIdx.x * NB + k] = acc[k];
  }
}

// Residual VJP over slots [s0, s1): whole populations write their gradient, parts of
// split populations write partials[part] (summed by smf_vjp_finalize_kernel).
// Fused VJP + Adam (unbounded) for shards whose populations are all whole: a lane that
// has its population's gradient applies the Adam update to the population's (a, s) pair
// directly -- theta, m, v and the trajectory row -- so the gradient never round-trips
// through HBM (reference Adam math: multigrad/adam.py:52-68 via jax optimizers.adam; the
// same expression order as csrc/adam.hip:adam_elem).
struct VjpAdam {
  float2* theta;        // parameters (the same array the kernel reads), updated in place
  float2* m;            // moments, indexed by unit - unit_offset
  float2* v;
  float2* traj;         // trajectory base (row r at traj + r * traj_stride floats) or null
  int64_t traj_stride;  // floats per trajectory row
  int64_t unit_offset;  // first unit owned by these moment / trajectory arrays
  const int* step;      // device step counter [step, ticket] (read when host_step < 0)
  int host_step;
  float lr, b1, b2, eps;
};

__device__ __forceinline__ void adam_pair(const VjpAdam& o, float bc1, float bc2, float2 g,
                                          float2& u, float2& m, float2& v) {
  m.x = (1.0f - o.b1) * g.x + o.b1 * m.x;
  m.y = (1.0f - o.b1) * g.y + o.b1 * m.y;
  v.x = (1.0f - o.b2) * (g.x * g.x) + o.b2 * v.x;
  v.y = (1.0f - o.b2) * (g.y * g.y) + o.b2 * v.y;
  u.x = u.x - o.lr * (m.x / bc1) / (sqrtf(v.x / bc2) + o.eps);
  u.y = u.y - o.lr * (m.y / bc1) / (sqrtf(v.y / bc2) + o.eps);
}

__global__ void smf_advance_step_kernel(int* step) { step[0] += 1; }

template <int NB, bool LOGSIG, bool ADAM = false>
__global__ __launch_bounds__(kThreads) void smf_vjp_lanes_kernel(
    const int32_t* __restrict__ slot_pop, const int32_t* __restrict__ slot_part,
    const float2* theta, const float* __restrict__ hvec,  // theta: written back under ADAM
    const float* __restrict__ resid, int64_t s0, int64_t s1,
    float2* __restrict__ grad, float2* __restrict__ partials, VjpAdam adam = VjpAdam{}) {
  float bc1 = 1.0f, bc2 = 1.0f;
  float2* trow = nullptr;
  if constexpr (ADAM) {
    const int st = adam.host_step >= 0
                       ? adam.host_step
                       : __hip_atomic_load(adam.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bc1 = bias_correction(adam.b1, st + 1);
    bc2 = bias_correction(adam.b2, st + 1);
    if (adam.traj)
      trow = reinterpret_cast<float2*>(reinterpret_cast<float*>(adam.traj) +
                                       (int64_t)(st + 1) * adam.traj_stride);
  }
  constexpr int R = 2 * (NB + 1);
  const int lane = threadIdx.x & (kWave - 1);
  // Persistent wavefronts, one group per iteration, the next group's residuals in flight
  // while the current one is contracted and written.  XCD-aware: workgroups are
  // dispatched round-robin over the kXcds L2 domains, so XCD x = blockIdx % kXcds takes
  // the x-th contiguous slice of the (window-ordered) groups -- each window's gradient
  // lines are then fully written, and its parameter lines fetched once, in ONE L2.
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
    float A = 0.0f, B = 0.0f;
#pragma unroll
    for (int e = 0; e <= NB; ++e) {
      A = fmaf(hvec[e], r[e], A);
      B = fmaf(hvec[e], r[NB + 1 + e], B);
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
        partials[pp] = make_float2(A, B);
      } else if constexpr (ADAM) {
        float2 u = theta[cc];
        const float2 gr = pop_grad<LOGSIG>(u, A, B);
        const int64_t j = cc - adam.unit_offset;
        float2 mm = adam.m[j], vv = adam.v[j];
        adam_pair(adam, bc1, bc2, gr, u, mm, vv);
        adam.m[j] = mm;
        adam.v[j] = vv;
        adam.theta[cc] = u;  // each lane owns its population's pair
        if (trow) trow[j] = u;
      } else {
        grad[cc] = pop_grad<LOGSIG>(theta[cc], A, B);
      }
    }
    g = gn;
  }
}

// VJP by recomputation over the lanes layout (no residuals): one wavefront per 64-slot
// group, each lane accumulates A = sum_e h_e exp2(-w^2), B = sum_e h_e exp2(-w^2) w over
// its population's halos (halo_vjp, as the tiles VJP) and writes the population's
// gradient -- or a partial for a split population (finalized in fixed order).  Used for
// data-parallel "hashed" shards, where a rank holds few halos per population (~3.4 at 8
// ranks): re-evaluating them is cheaper than writing and reading 2(NB+1) residual floats
// per population slot (profiles/hashed_proxy.md).  Groups are visited in creation
// (window) order, grid-strided over persistent wavefronts, so the gradient writes of one
// window of populations stay close in time.
template <int NB, bool LOGSIG>
__global__ __launch_bounds__(kThreads) void smf_vjp_lanes_rc_kernel(
    const float* __restrict__ xi, const int32_t* __restrict__ slot_idx,
    const int32_t* __restrict__ slot_part, const int64_t* __restrict__ group_base,
    const int32_t* __restrict__ group_len, const float2* __restrict__ theta,
    const float* __restrict__ hvec, SmfBins bins, int64_t g0, int64_t g1,
    float2* __restrict__ grad, float2* __restrict__ partials) {
  float h[NB + 1];
#pragma unroll
  for (int e = 0; e <= NB; ++e) h[e] = hvec[e];
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nw = (int64_t)gridDim.x * (kThreads / kWave);
  for (int64_t g = g0 + (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6); g < g1;
       g += nw) {
    const int64_t s = g * kWave + lane;
    const int c = slot_idx[s];
    const float2 th = theta[c < 0 ? 0 : c];
    const float inv = inv_sigma<LOGSIG>(th.y) * kWScale;
    const int len = group_len[g];
    const float* xp = xi + group_base[g] + lane;
    float A = 0.0f, B = 0.0f;
    int j = 0;
    for (; j + 2 <= len; j += 2) {
      const float x0 = xp[(int64_t)j * kWave];
      const float x1 = xp[(int64_t)(j + 1) * kWave];
      halo_vjp<NB, LOGSIG>(x0, th, inv, h, bins, A, B);
      halo_vjp<NB, LOGSIG>(x1, th, inv, h, bins, A, B);
    }
    if (j < len) halo_vjp<NB, LOGSIG>(xp[(int64_t)j * kWave], th, inv, h, bins, A, B);
    if (c >= 0) {
      const int part = slot_part[s];
      if (part >= 0) partials[part] = make_float2(A, B);
      else grad[c] = pop_grad<LOGSIG>(th, A, B);
    }
  }
}

// Interleave the population-sorted halos into the lanes layout (one wave per group).
__global__ __launch_bounds__(kThreads) void smf_lanes_pack_kernel(
    const float* __restrict__ xs, const int64_t* __restrict__ slot_src,
    const int32_t* __restrict__ slot_len, const int64_t* __restrict__ group_base,
    const int32_t* __restrict__ group_len, int64_t ngroups, float* __restrict__ xi) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t g = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
  if (g >= ngroups) return;
  const int64_t s = g * kWave + lane;
  const int64_t src = slot_src[s];
  const int len = slot_len[s];
  const int glen = group_len[g];
  float* dst = xi + group_base[g] + lane;
  for (int j = 0; j < glen; ++j) dst[(int64_t)j * kWave] = j < len ? xs[src + j] : kLaneSentinel;
}

// ------------------------------------------------------------------ host side
// graph replays keep the step on the device: advance it once every block has read it
static void launch_advance_step(int* step, hipStream_t stream) {
  hipLaunchKernelGGL(smf_advance_step_kernel, dim3(1), dim3(1), 0, stream, step);
}

// Fused residual VJP + unbounded Adam over slots [s0, s1) (whole populations only: the
// caller checks that no split population lies in the range).  m, v (and the optional
// trajectory rows) cover units [unit_offset, unit_offset + m.numel()/2).
void smf_vjp_adam_lanes(torch::Tensor slot_pop, torch::Tensor slot_part, torch::Tensor theta,
                        torch::Tensor h, torch::Tensor resid, int64_t s0, int64_t s1,
                        std::vector<double> scale, bool log_sigma, torch::Tensor m,
                        torch::Tensor v, int64_t unit_offset, torch::Tensor step,
                        int64_t host_step, double lr, double b1, double b2, double eps,
                        c10::optional<torch::Tensor> traj, int64_t traj_stride) {
  check_dev(slot_pop, "slot_pop", at::kInt);
  check_dev(slot_part, "slot_part", at::kInt);
  check_dev(theta, "theta", at::kFloat);
  check_dev(h, "h", at::kFloat);
  check_dev(resid, "resid", at::kFloat);
  check_dev(m, "m", at::kFloat);
  check_dev(v, "v", at::kFloat);
  TORCH_CHECK(step.is_cuda() && step.scalar_type() == at::kInt && step.numel() >= 2, "step: [2] int32 device");
  const int nbp = padded_bins((int)scale.size());
  TORCH_CHECK(h.numel() >= nbp + 1, "h too small");
  const int64_t ns = slot_pop.numel();
  TORCH_CHECK(slot_part.numel() == ns && resid.dim() == 3 && resid.size(0) * kWave == ns &&
                  resid.size(1) == 2 * (nbp + 1) && resid.size(2) == kWave && resid.is_contiguous(),
              "inconsistent residuals");
  TORCH_CHECK(s0 >= 0 && s1 <= ns && s0 <= s1 && s0 % kWave == 0 && s1 % kWave == 0, "bad slot range");
  TORCH_CHECK(m.numel() == v.numel() && m.numel() % 2 == 0, "m/v must hold whole units");
  TORCH_CHECK(unit_offset >= 0 && 2 * (unit_offset + m.numel() / 2) <= theta.numel(), "bad unit offset");
  VjpAdam a;
  a.theta = reinterpret_cast<float2*>(theta.data_ptr<float>());
  a.m = reinterpret_cast<float2*>(m.data_ptr<float>());
  a.v = reinterpret_cast<float2*>(v.data_ptr<float>());
  a.traj = nullptr;
  a.traj_stride = traj_stride;
  if (traj.has_value() && traj->defined()) {
    check_dev(*traj, "traj", at::kFloat);
    TORCH_CHECK(traj_stride % 2 == 0, "trajectory stride must keep float2 alignment");
    a.traj = reinterpret_cast<float2*>(traj->data_ptr<float>());
  }
  a.unit_offset = unit_offset;
  a.step = step.data_ptr<int>();
  a.host_step = (int)host_step;
  a.lr = (float)lr; a.b1 = (float)b1; a.b2 = (float)b2; a.eps = (float)eps;
  auto stream = at::hip::getCurrentHIPStream();
  const float2* tp = reinterpret_cast<const float2*>(theta.data_ptr<float>());
  if (s1 > s0) {
    // resident-workgroup cap, computed once per padded bin count: the device-property and
    // occupancy queries cost ~20 us of host time, which showed up as a gap before the
    // pipelined engine's drain launch
    static int64_t caps[kMaxBins + 1] = {0};
    int64_t& cap = caps[nbp];
    if (cap == 0)
      MG_DISPATCH_NB(nbp, {
        cap = resident_blocks((const void*)smf_vjp_lanes_kernel<NB, true, true>, kThreads);
      });
    const int64_t want = (s1 - s0 + kThreads - 1) / kThreads;
    const int64_t nblk = std::max<int64_t>(kXcds, std::min(cap, want) / kXcds * kXcds);
    MG_DISPATCH_NB(nbp, {
      with_bool(log_sigma, [&](auto LS) {
        hipLaunchKernelGGL((smf_vjp_lanes_kernel<NB, decltype(LS)::value, true>), dim3(nblk), dim3(kThreads), 0,
                           stream, slot_pop.data_ptr<int32_t>(), slot_part.data_ptr<int32_t>(), tp,
                           h.data_ptr<float>(), resid.data_ptr<float>(), s0, s1, nullptr, nullptr, a);
      });
    });
  }
  if (host_step < 0) launch_advance_step(step.data_ptr<int>(), stream);
}

torch::Tensor smf_fwd_trace() {
#ifdef MG_FWD_TRACE
  auto out = torch::empty({kTraceWaves, 3}, torch::kLong);
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out.data_ptr<int64_t>(), HIP_SYMBOL(g_fwd_trace), sizeof(g_fwd_trace));
  return out;
#else
  return torch::empty({0, 3}, torch::kLong);
#endif
}

int64_t smf_fwd_lanes_max_blocks(int64_t nb, bool log_sigma, bool rel_tail, bool resid) {
  const int nbp = padded_bins((int)nb);
  int64_t blocks = 0;
  MG_DISPATCH_NB(nbp, {
    with_bool(log_sigma, [&](auto LS) { with_bool(rel_tail, [&](auto RT) { with_bool(resid, [&](auto RS) {
      blocks = resident_blocks(
          (const void*)smf_fwd_lanes_kernel<NB, decltype(LS)::value, decltype(RT)::value, decltype(RS)::value>,
          kThreads);
    }); }); });
  });
  return blocks;
}

void smf_lanes_pack(torch::Tensor xs, torch::Tensor slot_src, torch::Tensor slot_len,
                    torch::Tensor group_base, torch::Tensor group_len, torch::Tensor xi) {
  check_dev(xs, "xs", at::kFloat);
  check_dev(slot_src, "slot_src", at::kLong);
  check_dev(slot_len, "slot_len", at::kInt);
  check_dev(group_base, "group_base", at::kLong);
  check_dev(group_len, "group_len", at::kInt);
  check_dev(xi, "xi", at::kFloat);
  const int64_t ng = group_len.numel();
  TORCH_CHECK(group_base.numel() == ng + 1 && slot_src.numel() == ng * kWave &&
                  slot_len.numel() == ng * kWave, "inconsistent lane schedule");
  if (ng == 0) return;
  const int64_t gpb = kThreads / kWave;
  hipLaunchKernelGGL(smf_lanes_pack_kernel, dim3((ng + gpb - 1) / gpb), dim3(kThreads), 0,
                     at::hip::getCurrentHIPStream(), xs.data_ptr<float>(),
                     slot_src.data_ptr<int64_t>(), slot_len.data_ptr<int32_t>(),
                     group_base.data_ptr<int64_t>(), group_len.data_ptr<int32_t>(), ng,
                     xi.data_ptr<float>());
}

// Forward over groups [g0, g1) of the lanes layout; optional residuals [ngroups, 2(NBP+1), 64].
int64_t smf_forward_lanes(torch::Tensor xi, torch::Tensor slot_pop, torch::Tensor group_base,
                       torch::Tensor group_len, torch::Tensor fwd_order, torch::Tensor theta,
                       std::vector<double> edges,
                       std::vector<double> scale, bool log_sigma, int64_t g0, int64_t g1,
                       torch::Tensor slab, int64_t nblocks, bool rel_tail,
                       c10::optional<torch::Tensor> resid,
                       c10::optional<torch::Tensor> wave_order,
                       c10::optional<torch::Tensor> wave_start,
                       c10::optional<torch::Tensor> queues,
                       c10::optional<std::vector<torch::Tensor>> update,
                       std::vector<double> update_scalars,
                       std::vector<torch::Tensor> epi_tensors, std::vector<double> epi_scalars,
                       std::vector<int64_t> epi_peers, bool per_edge) {
  check_dev(xi, "xi", at::kFloat);
  check_dev(slot_pop, "slot_pop", at::kInt);
  check_dev(group_base, "group_base", at::kLong);
  check_dev(group_len, "group_len", at::kInt);
  check_dev(fwd_order, "fwd_order", at::kInt);
  check_dev(theta, "theta", at::kFloat);
  check_dev(slab, "slab", at::kFloat);
  const int nbp = padded_bins((int)scale.size());
  const int64_t ng = group_len.numel();
  TORCH_CHECK(fwd_order.numel() == ng, "fwd_order must list every group");
  TORCH_CHECK(g0 >= 0 && g1 <= ng && g0 <= g1, "bad group range");
  TORCH_CHECK(slot_pop.numel() == ng * kWave && group_base.numel() == ng + 1, "inconsistent lane schedule");
  TORCH_CHECK(slab.numel() >= nblocks * nbp, "slab too small");
  TORCH_CHECK(nblocks >= 1 && nblocks <= 65535, "bad block count");
  const bool has_resid = resid.has_value() && resid->defined();
  float* rp = nullptr;
  if (has_resid) {
    check_dev(*resid, "resid", at::kFloat);
    TORCH_CHECK(resid->dim() == 3 && resid->size(0) == ng && resid->size(1) == 2 * (nbp + 1) &&
                    resid->size(2) == kWave, "resid must be [ngroups, 2*(nbp+1), 64]");
    rp = resid->data_ptr<float>();
  }
  const int32_t* order = fwd_order.data_ptr<int32_t>();
  const int32_t* ws = nullptr;
  if (wave_start.has_value() && wave_start->defined()) {
    // per-wave LPT lists over the groups [g0, g1): every wave of the grid has an entry
    TORCH_CHECK(wave_order.has_value() && wave_order->defined(), "wave_start needs wave_order");
    check_dev(*wave_order, "wave_order", at::kInt);
    check_dev(*wave_start, "wave_start", at::kInt);
    TORCH_CHECK(wave_start->numel() == nblocks * (kThreads / kWave) + 1,
                "wave_start must have one entry per wavefront of the grid (+1)");
    TORCH_CHECK(wave_order->numel() == g1 - g0, "wave_order must list the chunk's groups");
    order = wave_order->data_ptr<int32_t>();
    ws = wave_start->data_ptr<int32_t>();
  }
  int* qp = nullptr;
  int nq = 0;
  if (queues.has_value() && queues->defined()) {
    // dynamic schedule over fwd_order[g0, g1); the counters must be 0 (they are left at 0)
    TORCH_CHECK(!ws, "queues and wave_start are exclusive");
    check_dev(*queues, "queues", at::kInt);
    nq = (int)std::min<int64_t>(queues->numel(), nblocks);
    TORCH_CHECK(nq >= 1, "queues: at least one int32 counter");
    qp = queues->data_ptr<int>();
  }
  const SmfBins b = make_bins(edges, scale, nbp);
  auto stream = at::hip::getCurrentHIPStream();
  const float2* tp = reinterpret_cast<const float2*>(theta.data_ptr<float>());
  // the Euler-Maclaurin residual forwards: out-of-range groups through the out-of-line call
  // (LMODE 3); per_edge (the caller's choice when most groups are outside the EM range, e.g.
  // a fit with narrow populations everywhere): LMODE 4, the per-edge kernel for every group
  const bool em_resid = has_resid && !rel_tail && b.delta > 0.0f;
  const bool ledge = per_edge && em_resid;
  const bool lcall = !ledge && em_resid;
  // Sumstat epilogue launched right after this forward (epi_tensors = [slab of all chunks,
  // target, S, loss, h, seq, err, advance] (empty = absent), epi_scalars = [rows before this
  // chunk, eps, rank, timeout_s], epi_peers): one host call per chunk instead of two.
  const bool with_epi = !epi_tensors.empty();
  EpiArgs epi{};
  if (with_epi) {
    TORCH_CHECK(epi_tensors.size() == 8 && epi_scalars.size() == 4, "epilogue: 8 tensors, 4 scalars");
    auto ptr_i = [](const torch::Tensor& t) -> int* {
      return t.defined() && t.numel() ? t.data_ptr<int>() : nullptr;
    };
    const int64_t row0 = (int64_t)epi_scalars[0];
    TORCH_CHECK(row0 >= 0, "bad row offset");
    epi = make_epi(epi_tensors[0], row0 + nblocks, (int)scale.size(), nbp, epi_tensors[1],
                   epi_scalars[1], epi_tensors[2], epi_tensors[3], epi_tensors[4], epi_peers,
                   (int64_t)epi_scalars[2], ptr_i(epi_tensors[5]), ptr_i(epi_tensors[6]),
                   epi_scalars[3], ptr_i(epi_tensors[7]));
    TORCH_CHECK(epi.slab + row0 * nbp == slab.data_ptr<float>(),
                "the chunk's slab must start at the row offset of the full slab");
  }
  const bool upd = update.has_value();
  bool bnd = false;
  int* step_ctr = nullptr;  // device step counter to advance after this launch
  LanesUpdate u{};
  if (upd) {
    // pipelined update: tensors [h, m, v, step(int32[2]), traj (or empty)] (+ [u, lo, hi]
    // for bounded fits); scalars [unit_offset, host_step, lr, b1, b2, eps, traj_stride
    // (, defer_advance (, legacy))]
    const auto& U = *update;
    TORCH_CHECK((U.size() == 5 || U.size() == 8) && update_scalars.size() >= 7 &&
                    update_scalars.size() <= 9,
                "update: 5 tensors (+ u, lo, hi), 7 scalars (+ defer_advance, legacy)");
    // defer_advance: the caller advances the device step counter itself (the epilogue)
    const bool defer_advance = update_scalars.size() >= 8 && update_scalars[7] != 0.0;
    bnd = U.size() == 8;
    TORCH_CHECK(has_resid, "the pipelined update needs the residual buffer");
    check_dev(U[0], "h", at::kFloat);
    check_dev(U[1], "m", at::kFloat);
    check_dev(U[2], "v", at::kFloat);
    TORCH_CHECK(U[0].numel() >= nbp + 1 && U[1].numel() == U[2].numel(), "bad h/m/v");
    TORCH_CHECK(U[3].is_cuda() && U[3].scalar_type() == at::kInt, "step: int32 device");
    u.h = U[0].data_ptr<float>();
    u.theta_w = reinterpret_cast<float2*>(theta.data_ptr<float>());
    u.m = reinterpret_cast<float2*>(U[1].data_ptr<float>());
    u.v = reinterpret_cast<float2*>(U[2].data_ptr<float>());
    u.traj = U[4].numel() ? U[4].data_ptr<float>() : nullptr;
    u.unit_offset = (int64_t)update_scalars[0];
    u.host_step = (int)update_scalars[1];
    u.lr = (float)update_scalars[2];
    u.b1 = (float)update_scalars[3];
    u.b2 = (float)update_scalars[4];
    u.eps = (float)update_scalars[5];
    u.traj_stride = (int64_t)update_scalars[6];
    TORCH_CHECK(u.traj_stride % 2 == 0, "trajectory stride must keep float2 alignment");
    TORCH_CHECK(u.unit_offset >= 0 && 2 * (u.unit_offset + U[1].numel() / 2) <= theta.numel(),
                "bad unit offset");
    u.step = U[3].data_ptr<int>();
    u.legacy = update_scalars.size() >= 9 && update_scalars[8] != 0.0;
    if (bnd) {
      // bounded fits: the Euler-Maclaurin / per-edge residual forwards of the population
      // models (log10 sigma, absolute tails)
      TORCH_CHECK(log_sigma && (lcall || ledge), "the bounded pipelined update needs the "
                  "log-sigma Euler-Maclaurin or per-edge residual forward");
      for (int i = 5; i < 8; ++i) {
        check_dev(U[i], i == 5 ? "u" : i == 6 ? "lo" : "hi", at::kFloat);
        TORCH_CHECK(U[i].numel() == U[1].numel(), "u / lo / hi must be shaped like m");
      }
      u.u = reinterpret_cast<float2*>(U[5].data_ptr<float>());
      u.lo = reinterpret_cast<const float2*>(U[6].data_ptr<float>());
      u.hi = reinterpret_cast<const float2*>(U[7].data_ptr<float>());
    }
    if (u.host_step < 0 && !defer_advance) step_ctr = U[3].data_ptr<int>();
  }
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(kThreads), 0, stream, xi.data_ptr<float>(),
                       slot_pop.data_ptr<int32_t>(), group_base.data_ptr<int64_t>(),
                       group_len.data_ptr<int32_t>(), order, tp, g0, g1, b,
                       slab.data_ptr<float>(), rp, ws, qp, nq, u);
  };
  // smf_fwd_lanes_kernel<NB, LOGSIG, REL, RESID, UPD, LMODE, BND> by runtime arguments
  // (LS = log_sigma, RT = rel_tail, RS = has_resid; lcall and ledge imply RS && !RT):
  //   update  bounded  lcall/ledge   instance
  //   no      -        lcall         <NB, LS, false, true, false, kLanesMainMode>
  //   no      -        ledge         <NB, LS, false, true, false, 4>
  //   no      -        neither       <NB, LS, RT, RS>
  //   yes     no       lcall         <NB, LS, false, true, true, kLanesMainMode>
  //   yes     no       ledge         <NB, LS, false, true, true, 4>
  //   yes     no       neither       <NB, LS, RT, true, true>         (RS checked above)
  //   yes     yes      lcall         <NB, true, false, true, true, kLanesMainMode, true>
  //   yes     yes      ledge         <NB, true, false, true, true, 4, true>
  //   (bounded needs LS and lcall or ledge: checked above)
  MG_DISPATCH_NB(nbp, {
    with_bool(log_sigma, [&](auto LS_) { with_bool(upd, [&](auto UPD_) {
      constexpr bool LS = decltype(LS_)::value;
      constexpr bool UPD = decltype(UPD_)::value;
      if (lcall || ledge) {
        with_bool(lcall, [&](auto CALL_) {
          constexpr int LMODE = decltype(CALL_)::value ? kLanesMainMode : 4;
          if constexpr (LS && UPD) {
            if (bnd) return launch(smf_fwd_lanes_kernel<NB, true, false, true, true, LMODE, true>);
          }
          launch(smf_fwd_lanes_kernel<NB, LS, false, true, UPD, LMODE>);
        });
      } else {
        with_bool(rel_tail, [&](auto RT_) { with_bool(has_resid, [&](auto RS_) {
          constexpr bool RS = UPD || decltype(RS_)::value;
          launch(smf_fwd_lanes_kernel<NB, LS, decltype(RT_)::value, RS, UPD>);
        }); });
      }
    }); });
  });
  if (with_epi) launch_epilogue(nbp, epi, b, stream);
  if (step_ctr) launch_advance_step(step_ctr, stream);
  return nblocks;
}

// Residual VJP over slots [s0, s1) plus the fixed-order finalize of split populations
// listed in giant [G,3] = {pop, part_begin, part_end}.
void smf_vjp_lanes(torch::Tensor slot_pop, torch::Tensor slot_part, torch::Tensor theta,
                   torch::Tensor h, torch::Tensor resid, int64_t s0, int64_t s1,
                   std::vector<double> scale, bool log_sigma, torch::Tensor grad,
                   torch::Tensor partials, torch::Tensor giant) {
  check_dev(slot_pop, "slot_pop", at::kInt);
  check_dev(slot_part, "slot_part", at::kInt);
  check_dev(theta, "theta", at::kFloat);
  check_dev(h, "h", at::kFloat);
  check_dev(resid, "resid", at::kFloat);
  check_dev(grad, "grad", at::kFloat);
  const int nbp = padded_bins((int)scale.size());
  TORCH_CHECK(h.numel() >= nbp + 1, "h too small");
  TORCH_CHECK(grad.numel() == theta.numel(), "grad/theta size mismatch");
  const int64_t ns = slot_pop.numel();
  TORCH_CHECK(slot_part.numel() == ns && resid.dim() == 3 && resid.size(0) * kWave == ns &&
                  resid.size(1) == 2 * (nbp + 1) && resid.size(2) == kWave, "inconsistent residuals");
  TORCH_CHECK(s0 >= 0 && s1 <= ns && s0 <= s1, "bad slot range");
  auto stream = at::hip::getCurrentHIPStream();
  const float2* tp = reinterpret_cast<const float2*>(theta.data_ptr<float>());
  float2* gp = reinterpret_cast<float2*>(grad.data_ptr<float>());
  float2* pa = partials.numel() ? reinterpret_cast<float2*>(partials.data_ptr<float>()) : nullptr;
  TORCH_CHECK(s0 % kWave == 0 && s1 % kWave == 0, "slot ranges must be group aligned");
  TORCH_CHECK(resid.is_contiguous(), "resid must be contiguous");
  if (s1 > s0) {
    static int64_t caps[kMaxBins + 1] = {0};  // per padded bin count (register use differs)
    int64_t& cap = caps[nbp];
    if (cap == 0)
      MG_DISPATCH_NB(nbp, {
        cap = resident_blocks((const void*)smf_vjp_lanes_kernel<NB, true>, kThreads);
      });
    const int64_t want = (s1 - s0 + kThreads - 1) / kThreads;
    const int64_t nblk = std::max<int64_t>(kXcds, std::min(cap, want) / kXcds * kXcds);
    MG_DISPATCH_NB(nbp, {
      with_bool(log_sigma, [&](auto LS) {
        hipLaunchKernelGGL((smf_vjp_lanes_kernel<NB, decltype(LS)::value>), dim3(nblk), dim3(kThreads), 0,
                           stream, slot_pop.data_ptr<int32_t>(), slot_part.data_ptr<int32_t>(), tp,
                           h.data_ptr<float>(), resid.data_ptr<float>(), s0, s1, gp, pa);
      });
    });
  }
  launch_vjp_finalize(giant, pa, tp, gp, log_sigma, stream);
}

// Recompute VJP over groups [g0, g1) of the lanes schedule (whole shard or one chunk)
// plus the fixed-order finalize of split populations (giant [G,3]).
void smf_vjp_lanes_rc(torch::Tensor xi, torch::Tensor slot_idx, torch::Tensor slot_part,
                      torch::Tensor group_base, torch::Tensor group_len, torch::Tensor theta,
                      torch::Tensor h, std::vector<double> edges, std::vector<double> scale,
                      bool log_sigma, int64_t g0, int64_t g1, torch::Tensor grad,
                      torch::Tensor partials, torch::Tensor giant) {
  check_dev(xi, "xi", at::kFloat);
  check_dev(slot_idx, "slot_idx", at::kInt);
  check_dev(slot_part, "slot_part", at::kInt);
  check_dev(group_base, "group_base", at::kLong);
  check_dev(group_len, "group_len", at::kInt);
  check_dev(theta, "theta", at::kFloat);
  check_dev(h, "h", at::kFloat);
  check_dev(grad, "grad", at::kFloat);
  const int nbp = padded_bins((int)scale.size());
  const int64_t ng = group_len.numel();
  TORCH_CHECK(h.numel() >= nbp + 1, "h too small");
  TORCH_CHECK(grad.numel() >= theta.numel(), "grad smaller than theta");
  TORCH_CHECK(slot_idx.numel() == ng * kWave && slot_part.numel() == ng * kWave &&
                  group_base.numel() == ng + 1, "inconsistent lane schedule");
  TORCH_CHECK(g0 >= 0 && g1 <= ng && g0 <= g1, "bad group range");
  const SmfBins b = make_bins(edges, scale, nbp);
  auto stream = at::hip::getCurrentHIPStream();
  const float2* tp = reinterpret_cast<const float2*>(theta.data_ptr<float>());
  float2* gp = reinterpret_cast<float2*>(grad.data_ptr<float>());
  float2* pa = partials.numel() ? reinterpret_cast<float2*>(partials.data_ptr<float>()) : nullptr;
  if (g1 > g0) {
    static int64_t caps[kMaxBins + 1] = {0};
    int64_t& cap = caps[nbp];
    if (cap == 0)
      MG_DISPATCH_NB(nbp, {
        cap = resident_blocks((const void*)smf_vjp_lanes_rc_kernel<NB, true>, kThreads);
      });
    const int64_t want = (g1 - g0 + (kThreads / kWave) - 1) / (kThreads / kWave);
    const int64_t nblk = std::max<int64_t>(1, std::min(cap, want));
    MG_DISPATCH_NB(nbp, {
      with_bool(log_sigma, [&](auto LS) {
        hipLaunchKernelGGL((smf_vjp_lanes_rc_kernel<NB, decltype(LS)::value>), dim3(nblk), dim3(kThreads), 0,
                           stream, xi.data_ptr<float>(), slot_idx.data_ptr<int32_t>(),
                           slot_part.data_ptr<int32_t>(), group_base.data_ptr<int64_t>(),
                           group_len.data_ptr<int32_t>(), tp, h.data_ptr<float>(), b, g0, g1, gp, pa);
      });
    });
  }
  launch_vjp_finalize(giant, pa, tp, gp, log_sigma, stream);
}

}  // namespace mg
