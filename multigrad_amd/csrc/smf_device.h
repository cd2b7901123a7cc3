// Stellar-mass-function (SMF) summed-statistic kernels for gfx950 (MI355X).
//
// Model (reference tests/smf_example/smf_grad_descent.py:32-48 and
// docs/source/notebooks/smf_gradient_descent.py:20-35, generalised to populations):
//   halo i belongs to population c_i; theta is interleaved (a_c, s_c) per population;
//   mu_i = x_i + a_c ;  sigma_c = LOGSIG ? 10^{s_c} : s_c
//   S_k  = scale_k * sum_i [ Phi((e_{k+1}-mu_i)/sigma) - Phi((e_k-mu_i)/sigma) ]
// The reference issues one XLA dispatch per bin with 2 erf per halo per bin; here ONE
// pass evaluates all NB+1 edge tails per halo (Q(z) to float32-erf absolute accuracy, or
// tail-accurate to ~1e-6 relative: SmfBins.tail, see common.h), keeps
// the NB bin sums in registers across a grid-stride loop, and reduces them
// deterministically (wave shuffles -> LDS -> per-block slab -> fixed-order slab sum).
//
// This header: the device-side pieces shared by the kernel families (smf_tiles.hip,
// smf_lanes.hip, smf2.hip).
#pragma once
#include "common.h"
#include "adam.h"
#include "xgmi.h"
#include "tail_table.h"

#include <type_traits>
#include <utility>

namespace mg {

constexpr int kMaxBins = 32;
constexpr int kXcds = 8;  // MI355X: 8 XCDs (L2 domains), workgroups dispatched round-robin
constexpr int kThreads = 256;
constexpr int kItems = 8;                      // halos per thread in a tile
constexpr int kTileHalos = kThreads * kItems;   // 2048
constexpr int kTilePops = 2048;
constexpr float kLn10 = 2.302585092994046f;
constexpr float kLog2_10 = 3.321928094887362f;

struct SmfBins {
  float edge[kMaxBins + 1];  // NBP+1 edges (padded bins are zero width, scale 0)
  float scale[kMaxBins];     // 1 / (volume * width) per bin
  float delta;               // edge spacing when uniform (== 0: non-uniform)
};

struct Tile {
  int64_t h0, h1;  // halo range [h0, h1)
  int32_t p0, p1;  // population range [p0, p1) (p1 = p0+1 for partial tiles)
  int32_t slot;    // -1: whole populations; >=0: partial-sum slot of population p0
  int32_t pad;
};

// Edge-pair layout of the packed-fp32 kernels: edges (2i, 2i+1) form pair i; with an odd
// edge count the last edge gets a pair of its own (.x used).
template <int NB>
struct EdgePairs {
  static constexpr int NE = NB + 1;
  static constexpr int NP = NE / 2;             // pairs inside one halo
  static constexpr int NX = NE & 1;             // 1: cross-halo pair for the last edge
  static constexpr int NV = NP + NX;            // accumulator pairs
};

template <bool LOGSIG>
__device__ __forceinline__ float inv_sigma(float s) {
  return LOGSIG ? fast_exp2(-s * kLog2_10) : 1.0f / s;
}

// Table path of the absolute contract: the signed tail V(n) = sign(n) Q(|n|)
// is read from a piecewise-cubic table (tail_table.h, tools/fit_tail_table.py: 96 pieces
// over |z| <= 6, float32 chain error 8.8e-8 against 1.6e-7 for the rational polynomial)
// held in LDS, instead of v_rcp + a degree-5 Horner chain + the product with exp2(-w^2):
//   t = clamp(n * INVH), k = floor(t) (v_cvt_flr), s = fract(t), V = c_k(s)
// The exponential is still evaluated for the residuals G, W (unchanged semantics) but no
// longer for the forward sums.  The integer part is counted from t < 0, so it always
// agrees with the piece that was read (the jump of V at n = 0 is a piece boundary).
// LDS layout: REPL replicas of every entry, lane l reading replica l % REPL, so the 16
// lanes of a ds_read_b128 lane group hit distinct bank quads (REPL = 16: conflict free;
// 8: two lanes per replica).
// Forwards WITHOUT residuals use the table -- there it also removes the v_exp, and the
// lanes forward measured 440 vs 536-540 us at 1.34e8 halos.  Using it in the residual
// forwards too, where the exponential stays (for G, W), measured slower (pipelined 702 vs
// 628 us, residual 620 vs 570 us; the switch was removed in round 5).  The
// index arithmetic (v_med3, v_cvt_flr, v_fract, v_lshl_or: 4.2-4.3 cycles per wave each,
// tools/ubench/op_rates.hip, against 2.7 for v_fma) eats most of what the v_rcp and the
// Horner chain cost, and at 119-128 VGPRs the compiler waits for each table read right
// after issuing it (docs/design.md, forward floor).
__device__ __forceinline__ int cvt_flr_i32(float t) {
  int k;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(k) : "v"(t));
  return k;
}

__device__ __forceinline__ float fma_scalar(float a, float b, float c) {
  float d;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

template <int REPL>
__device__ __forceinline__ void tail_tab_fill(float4* tab) {
  for (int i = threadIdx.x; i < kTailTabN * REPL; i += blockDim.x) tab[i] = g_tail_tab[i / REPL];
}

// this lane's view of the LDS table: entry k in [-N/2, N/2) at tb[k * REPL]
template <int REPL>
__device__ __forceinline__ const float4* tail_tab_lane(const float4* tab) {
  return tab + (kTailTabN / 2) * REPL + (threadIdx.x & (REPL - 1));
}

// Accumulate the NB bin masses of one halo.
// Work with the negated scaled coordinate n_e = -w_e = (mu - e_e) * kWScale / sigma.
// With signed tails V_e = copysign(Q(|z_e|), n_e) and pos_e = [n_e < 0] = [z_e > 0]
// (sign bit of n), Phi(z_e) = pos_e + V_e, so mass_k = (V_{k+1} - V_k) + (pos_{k+1} -
// pos_k).  Per thread the kernel accumulates the per-EDGE sums sum V_e (one fma per edge:
// the sign is folded into the Gaussian factor) and the 0/1 parts as exact integer
// counts; the per-bin differences are formed once per thread at the end.
// A halo with x = -inf contributes exactly zero (used to mask the unrolled tail): every
// V_e is -0 and every pos_e is 1, which cancels in the differences.
template <int NB, bool LOGSIG, bool REL, int REPL = 0>
__device__ __forceinline__ void halo_mass(float x, float2 th, const SmfBins& b,
                                          float (&acc)[NB + 1], int (&cnt)[NB + 1],
                                          const float4* __restrict__ tb = nullptr) {
  // table path: the coordinate is formed directly in table units (the piece scale folded
  // into the two per-halo factors: one multiply per halo instead of one per edge)
  constexpr bool kFold = REPL > 0;
  const float ninv = -inv_sigma<LOGSIG>(th.y) * (kFold ? kWScale * kTailTabInvH : kWScale);
  const float mu = -(x + th.x) * ninv;  // = (x + a) * kWScale / sigma (x kTailTabInvH)
#pragma unroll
  for (int e = 0; e <= NB; ++e) {
    const float n = fmaf(b.edge[e], ninv, mu);
    if constexpr (REPL > 0) {  // signed-tail table (see ep_eval_tab)
      const float t = __builtin_amdgcn_fmed3f(n, -(float)(kTailTabN / 2),
                                              (float)(kTailTabN / 2) - 1.0f / 4096);
      const float4 c = tb[cvt_flr_i32(t) * REPL];
      const float s = __builtin_amdgcn_fractf(t);
      acc[e] += fma_scalar(fma_scalar(fma_scalar(c.w, s, c.z), s, c.y), s, c.x);
      cnt[e] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(t < 0.0f));
      continue;
    }
    float p, g;
    normal_tail_parts_w<REL>(n, p, g);
    acc[e] = fmaf(p, __builtin_copysignf(g, n), acc[e]);
    // wave-wide count of the 0/1 parts: one v_cmp, the popcount/add run on the SALU
    cnt[e] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(n < 0.0f));
  }
}

// Edge weights h_e from the sumstat cotangent g (dL/dS), folded with 1/sqrt(2 pi).
__device__ __forceinline__ float edge_weight(const float* g, const SmfBins& b, int e, int nb) {
  float h = 0.0f;
  if (e >= 1) h += g[e - 1] * b.scale[e - 1];
  if (e < nb) h -= g[e] * b.scale[e];
  return h * 0.3989422804014327f;
}

// Arguments of the sumstat epilogue (see smf_epilogue_kernel); `on` = 0: none.
struct EpiArgs {
  const float* slab;
  int nrows, nb, rank, size, on;
  XgmiPeers peers;
  unsigned* seq;
  int* err;
  long long ticks;
  const float* target;
  float eps;
  float* S_out;
  float* loss;
  float* h;
  int* advance;
};

// Per-halo VJP contributions in the scaled coordinate w = z*kWScale:
//   A += sum_e h_e exp2(-w_e^2),   B += sum_e h_e exp2(-w_e^2) w_e
// (h_e already carries 1/sqrt(2 pi); B is converted back to z units in pop_grad).
// Edges two at a time in packed fp32 (v_pk_fma / v_pk_mul / v_pk_add on the
// pair (edge 2i, edge 2i+1), as in the lanes forward's EdgePairs), so w, w^2, h*g and both
// accumulations cost one issue per pair; v_exp stays per element.
template <int NB, bool LOGSIG>
__device__ __forceinline__ void halo_vjp(float x, float2 th, float inv, const float (&h)[NB + 1],
                                         const SmfBins& b, float& A, float& B) {
  const float nmi = -(x + th.x) * inv;
  constexpr int NP = (NB + 1) / 2;
  v2f Ap = (v2f)(0.0f), Bp = (v2f)(0.0f);
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    v2f e2, h2;
    e2.x = b.edge[2 * i];
    e2.y = b.edge[2 * i + 1];
    h2.x = h[2 * i];
    h2.y = h[2 * i + 1];
    const v2f w = e2 * inv + nmi;
    const v2f q = -w * w;
    v2f g;
    g.x = fast_exp2(q.x);
    g.y = fast_exp2(q.y);
    const v2f t = h2 * g;
    Ap = Ap + t;
    Bp = t * w + Bp;
  }
  if constexpr ((NB + 1) & 1) {
    const float w = fmaf(b.edge[NB], inv, nmi);
    const float t = h[NB] * fast_exp2(-w * w);
    Ap.x += t;
    Bp.x = fmaf(t, w, Bp.x);
  }
  A += Ap.x + Ap.y;
  B += Bp.x + Bp.y;
}

// inv is the scaled inverse sigma (kWScale / sigma); A, B from halo_vjp.
template <bool LOGSIG>
__device__ __forceinline__ float2 pop_grad(float2 th, float A, float B) {
  constexpr float kInvW = 1.0f / kWScale;
  const float inv = inv_sigma<LOGSIG>(th.y);
  return make_float2(-inv * A, LOGSIG ? -(kLn10 * kInvW) * B : -(inv * kInvW) * B);
}

// bound kind from the finite bounds (csrc/adam.h BoundKind)
__device__ __forceinline__ int8_t bound_kind(float lo, float hi) {
  const bool l = __builtin_isfinite(lo), h = __builtin_isfinite(hi);
  return l ? (h ? kBoth : kLow) : (h ? kHigh : kNone);
}

// Padding halo of the lanes layout (smf_lanes.hip) and the masked halos of the shared-parameter
// loops: it contributes exactly zero on the per-edge and the Euler-Maclaurin paths.
constexpr float kLaneSentinel = -1e30f;

// ---------------------------------------------------------- Euler-Maclaurin bin masses
// Euler-Maclaurin path (absolute contract, uniformly spaced edges): inside a lanes group every halo of
// a lane shares the lane's sigma, so the bin width in sigma units h = delta / sigma is a
// lane constant.  The mass of bin k is then the integral of the Gaussian over one panel of
// width h, evaluated by the Euler-Maclaurin formula from the Gaussian factor and its odd
// derivatives at the two edges (f = exp(-z^2/2), f' = -z f, f''' = (3z - z^3) f,
// f^(5) = -(z^5 - 10 z^3 + 15 z) f):
//   mass_k = (h/2)(f_k + f_{k+1}) + [E]_k^{k+1},   E(z) = f z (c1 + c3 z^2 + c5 z^4)
//   c1 = h^2/12 + 3h^4/720 + 15h^6/30240,  c3 = -(h^4/720 + 10h^6/30240),  c5 = h^6/30240
// (all over sqrt(2 pi)).  The remainder is h^9 B_8/8! f^(8) <= 3.5e-5 h^9: 6.8e-8 absolute at
// the largest width the path accepts (kEmHMax = 0.5, about the float32 erf of the
// reference), far below the argument rounding of any per-edge evaluation.
// The Gaussian factors of the NB+1 equally spaced edges come from ONE seed pair per halo by
// the exact recurrence f_{e+2} = f_e exp2(-4 dw w_{e+1}) (w = z * kWScale, dw = edge spacing
// in w): the seed pair (edges 2M, 2M+1, M = NP/2) and R = exp2(-4 dw w_{2M+1}) are three
// v_exp and one v_rcp per halo; pair M+j is p_j = (f_2M, f_2M+1) R^j, exact up to the lane
// constant Q_j = (exp2(-4 dw^2 j(j-1)), exp2(-4 dw^2 j^2)), which is applied to the per-group
// sums once per group instead of per halo.  Every per-edge sum the forward needs -- the trap
// part F = sum f, E = sum E(w), and the VJP residuals G = F, W = sum f w -- is linear in f, so
// a halo costs 9 packed ops per edge pair and no per-edge transcendental, no v_rcp and no
// sign / count bookkeeping: 4 v_exp/v_rcp per halo against 22 for the rational tail.
// A group whose lanes are not all inside kEmHMax (or non-uniform / padded bins, or the
// relative-tail contract) runs the per-edge tail evaluation instead (the ballot is
// wave-uniform).  The VJP residuals agree with the per-edge exponentials to the chain's
// rounding (~1e-6 relative), inside the VJP's contract.
constexpr float kEmHMax = 0.5f;
constexpr float kInvSqrt2Pi = 0.39894228040143268f;

struct EmLane {
  float inv;         // kWScale / sigma
  float dw4;         // -4 dw
  float a1, a3, a5;  // E(w) = f w (a1 + a3 w^2 + a5 w^4)  (w units)
};

__device__ __forceinline__ EmLane em_lane(float inv, float delta) {
  constexpr float ik = 1.0f / kWScale;
  EmLane L;
  L.inv = inv;
  const float dw = delta * inv;
  L.dw4 = -4.0f * dw;
  const float h = dw * ik;
  const float h2 = h * h, h4 = h2 * h2, h6 = h4 * h2;
  L.a1 = (h2 * (1.0f / 12.0f) + h4 * (3.0f / 720.0f) + h6 * (15.0f / 30240.0f)) * ik;
  L.a3 = -(h4 * (1.0f / 720.0f) + h6 * (10.0f / 30240.0f)) * (ik * ik * ik);
  L.a5 = h6 * (1.0f / 30240.0f) * (ik * ik * ik * ik * ik);
  return L;
}

// Two-term Euler-Maclaurin (B_2, B_4 only: c1 = h^2/12 + 3h^4/720, c3 = -h^4/720): its
// remainder, the B_6 term, is at most 1.26e-7 of one halo's unit mass per bin at
// h = 0.35 (8.3e-8 at 0.33, 1.2e-8 at 0.25; maximum over the halo position, checked in
// float64 against the exact Gaussian integral), inside the absolute contract of the
// per-edge tails (1.6e-7).  A lane group whose widths are all <= kEmH2 skips the z^5 term:
// one packed FMA per edge pair per halo less (~6 of ~78 VALU per halo).  The headline
// populations sit at h = 0.2 .. 0.32.
constexpr float kEmH2 = 0.35f;

__device__ __forceinline__ EmLane em_lane2(float inv, float delta) {
  constexpr float ik = 1.0f / kWScale;
  EmLane L;
  L.inv = inv;
  const float dw = delta * inv;
  L.dw4 = -4.0f * dw;
  const float h = dw * ik;
  const float h2 = h * h, h4 = h2 * h2;
  L.a1 = (h2 * (1.0f / 12.0f) + h4 * (3.0f / 720.0f)) * ik;
  L.a3 = -(h4 * (1.0f / 720.0f)) * (ik * ik * ik);
  L.a5 = 0.0f;
  return L;
}

// One halo (nm = -(x + a) inv): F, Wa, E accumulate the UNSCALED sums of edge pairs (the
// pair layout of EdgePairs; an odd last edge in the .x half of the extra pair).  The lane
// constants come as scalars, not as the EmLane struct: splats of adjacent struct fields were
// widened into 8-byte loads that kept (a1, a3, a5) in private memory, a scratch store and two
// scratch loads at every group start of the headline kernel.
template <int NB, bool RESID, bool A7 = false, bool A5 = true>
__device__ __forceinline__ void em_halo(float nm, float inv, float dw4, float a1, float a3,
                                        float a5, const SmfBins& b,
                                        v2f (&F)[EdgePairs<NB>::NV], v2f (&Wa)[EdgePairs<NB>::NV],
                                        v2f (&E)[EdgePairs<NB>::NV], float a7 = 0.0f) {
  using EP = EdgePairs<NB>;
  constexpr int M = EP::NP / 2;
  // sentinel / masked halos (x = -1e30 or -inf): f = 0, and w^4 stays finite so 0 * E = 0
  nm = __builtin_amdgcn_fmed3f(nm, -1e6f, 1e6f);
  // w of the seed pair from the edges; the other pairs step by 2 dw (two lane constants
  // instead of one per pair, which the compiler would otherwise keep in registers)
  const float dw2 = -0.5f * dw4;
  v2f wm;
  {
    v2f e2;
    e2.x = b.edge[2 * M];
    e2.y = b.edge[2 * M + 1];
    wm = e2 * inv + nm;
  }
  auto wpair = [&](int i) { return wm + (float)(i - M) * dw2; };
  auto accum = [&](int i, v2f p, v2f w) {
    const v2f pw = p * w;
    F[i] = F[i] + p;
    if constexpr (RESID) Wa[i] = Wa[i] + pw;
    const v2f w2 = w * w;
    v2f t;
    if constexpr (A7) {
      t = w2 * a7 + a5;
      t = t * w2 + a3;
      t = t * w2 + a1;
    } else if constexpr (A5) {
      t = w2 * a5 + a3;
      t = t * w2 + a1;
    } else {
      t = w2 * a3 + a1;
    }
    E[i] = pw * t + E[i];
  };
  const v2f ws = wpair(M);
  const v2f q = -ws * ws;
  v2f p0;
  p0.x = fast_exp2(q.x);
  p0.y = fast_exp2(q.y);
  const float R = fast_exp2(__builtin_amdgcn_fmed3f(dw4 * ws.y, -126.0f, 126.0f));
  accum(M, p0, ws);
  v2f p = p0;
#pragma unroll
  for (int i = M + 1; i < EP::NP; ++i) {
    p = p * R;
    accum(i, p, wpair(i));
  }
  if constexpr (EP::NX) {  // odd last edge: scalar (a packed op costs two scalar issues anyway)
    const float pz = p.x * R;
    const float wz = fmaf((float)(EP::NP - M), dw2, wm.x);
    const float pw = pz * wz;
    F[EP::NP].x += pz;
    if constexpr (RESID) Wa[EP::NP].x += pw;
    const float w2 = wz * wz;
    const float t = A7 ? fmaf(fmaf(fmaf(w2, a7, a5), w2, a3), w2, a1)
                       : (A5 ? fmaf(fmaf(w2, a5, a3), w2, a1) : fmaf(w2, a3, a1));
    E[EP::NP].x = fmaf(pw, t, E[EP::NP].x);
  }
  if constexpr (M > 0) {
    const float Ri = fast_rcp(R);
    p = p0;
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
      p = p * Ri;
      accum(i, p, wpair(i));
    }
  }
}

// Per-edge evaluation of ONE halo (absolute contract, scalar) into the edge-pair
// accumulators: the fallback of the Euler-Maclaurin kernels for groups outside kEmHMax.
// It is deliberately lean in registers (one halo, one edge at a time): with the packed
// two-halo path as the fallback the pipelined-update kernel spilled 33 VGPRs and ran 12%
// slower even though no group took the fallback (profiles/em_forward/).
template <int NB, bool RESID>
__device__ __forceinline__ void lane_halo_exact1(float x, float ninv, float mua, const SmfBins& b,
                                                 v2f (&acc)[EdgePairs<NB>::NV], int (&cnt)[NB + 1],
                                                 v2f (&G)[EdgePairs<NB>::NV],
                                                 v2f (&W)[EdgePairs<NB>::NV]) {
  const float mu = fmaf(x, -ninv, mua);
#pragma unroll
  for (int e = 0; e <= NB; ++e) {
    const float n = fmaf(b.edge[e], ninv, mu);
    float p, g;
    normal_tail_parts_w<false>(n, p, g);
    const float v = p * __builtin_copysignf(g, n);
    cnt[e] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(n < 0.0f));
    const int i = e >> 1;
    if (e & 1) {
      acc[i].y += v;
      if constexpr (RESID) {
        G[i].y += g;
        W[i].y = fmaf(-g, n, W[i].y);
      }
    } else {
      acc[i].x += v;
      if constexpr (RESID) {
        G[i].x += g;
        W[i].x = fmaf(-g, n, W[i].x);
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
}

// End of a group: apply the lane constants Q_j to the pair sums (F, Wa become the true
// residuals G, W), and add the lane's cumulative bin masses C_e (C_{k+1} - C_k = mass_k) to
// the per-edge accumulators of the edge-pair path.
template <int NB, class LaneT>
__device__ __forceinline__ void em_group_end(const LaneT& L, v2f (&F)[EdgePairs<NB>::NV],
                                             v2f (&Wa)[EdgePairs<NB>::NV],
                                             v2f (&E)[EdgePairs<NB>::NV],
                                             v2f (&accp)[EdgePairs<NB>::NV]) {
  using EP = EdgePairs<NB>;
  constexpr int M = EP::NP / 2;
  const float l4 = 0.25f * L.dw4 * L.dw4;  // 4 dw^2 ... as -(dw4^2)/4 = -4 dw^2 below
#pragma unroll
  for (int i = 0; i < EP::NV; ++i) {
    const int j = i - M;
    v2f Q;
    Q.x = (j * (j - 1) == 0) ? 1.0f : fast_exp2(-l4 * (float)(j * (j - 1)));
    Q.y = (i == EP::NP) ? Q.x : ((j * j == 0) ? 1.0f : fast_exp2(-l4 * (float)(j * j)));
    F[i] = F[i] * Q;
    Wa[i] = Wa[i] * Q;
    E[i] = E[i] * Q;
  }
  // trapezoid weight h/2 and the normalisation, in w units: h = dw / kWScale
  const float hh = (-0.125f / kWScale) * L.dw4;  // dw / (2 kWScale)
  float T = 0.0f, fprev = 0.0f;
#pragma unroll
  for (int e = 0; e <= NB; ++e) {
    const int i = e >> 1;
    float fe, ee;
    if (i < EP::NP) {
      fe = (e & 1) ? F[i].y : F[i].x;
      ee = (e & 1) ? E[i].y : E[i].x;
    } else {
      fe = F[i].x + F[i].y;
      ee = E[i].x + E[i].y;
    }
    if (e > 0) T = fmaf(hh, fprev + fe, T);
    fprev = fe;
    const float C = kInvSqrt2Pi * (T + ee);
    if (i < EP::NP) {
      if (e & 1) accp[i].y += C;
      else accp[i].x += C;
    } else {
      accp[i].x += C;
    }
  }
}

// s_waitcnt vmcnt(0) (expcnt / lgkmcnt left alone): global_load_lds writes LDS behind the
// compiler's back, so its completion is waited for explicitly before the LDS is read.
__device__ __forceinline__ void vmem_wait_all() { __builtin_amdgcn_s_waitcnt(0x0F70); }

template <int N>
__device__ __forceinline__ void vmem_wait_n() {  // s_waitcnt vmcnt(N), expcnt / lgkmcnt untouched
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0x0F70);
  asm volatile("" ::: "memory");
}

// Wave-wide copy of a contiguous block of NR rows x 64 floats into LDS (global_load_lds:
// no VGPRs): 1 KB per dwordx4 instruction, then single rows.  One LDS base (M0) per 4 KB,
// the immediate offset moving both the global and the LDS address.
template <int I>
__device__ __forceinline__ void lds_stage_chunk(const float* src, float* dst, int lane) {
  constexpr int base = (I / 4) * 1024;  // floats
  __builtin_amdgcn_global_load_lds(src + base + lane * 4, dst + base, 16, (I % 4) * 1024, 0);
}
template <int R>
__device__ __forceinline__ void lds_stage_row(const float* src, float* dst, int lane) {
  constexpr int base = (R * kWave / 1024) * 1024;
  __builtin_amdgcn_global_load_lds(src + base + lane, dst + base, 4, (R * kWave - base) * 4, 0);
}
template <int NR, int... I, int... R>
__device__ __forceinline__ void lds_stage_seq(const float* src, float* dst, int lane,
                                              std::integer_sequence<int, I...>,
                                              std::integer_sequence<int, R...>) {
  (lds_stage_chunk<I>(src, dst, lane), ...);
  (lds_stage_row<(NR / 4) * 4 + R>(src, dst, lane), ...);
}
template <int NR>
__device__ __forceinline__ void lds_stage_block(const float* src, float* dst, int lane) {
  lds_stage_seq<NR>(src, dst, lane, std::make_integer_sequence<int, NR / 4>{},
                    std::make_integer_sequence<int, NR % 4>{});
}

}  // namespace mg
