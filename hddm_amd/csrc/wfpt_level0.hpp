// wfpt_level0.hpp — the level-0 passes of the device density: the reference's
// prologue + root aux node of every adaptive Simpson a trial runs, one trial
// per lane. The engine's form (eng_level0_t, on the call's z grid, any single
// t node on its own), the per-node / per-trial-parameter form on the trial's
// own grid (fast_level0) and the direct family's (direct_level0). Trees that
// refine continue in the wave that owns the trial (engine_kernel,
// wfpt_engine.hip: tree_node / tree_value over the dyadic points).
// Device code (DirectArgs / direct_args: host + device).
// Compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "wfpt_grid.hpp"
#include "wfpt_math.hpp"
#include "wfpt_quad.hpp"
#include "wfpt_series.hpp"
#include "wfpt_types.hpp"
#include "wfpt_zgrid.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// Root interval of the adaptive tree: over t for kAdaptT / kAdaptTZ, over z
// for kAdaptZ.
template <int MODE>
__device__ inline void tree_root(const Trial& tr, const Params& P, double& lb, double& ub) {
  if (MODE == kAdaptZ) {
    lb = tr.z - tr.sz / 2.;
    ub = tr.z + tr.sz / 2.;
  } else {
    lb = P.t - tr.st / 2.;
    ub = P.t + tr.st / 2.;
  }
}

// The engine's level 0 (kAdaptT / kAdaptTZ): the same operations as
// fast_level0, factored so that any single t node j of a trial's root
// interval can be evaluated on its own (a split chunk's level-0 task) with
// exactly the bits the per-lane loop produces. The z grid is the call's table
// (EngTables), shared by both.
struct L0Hints {
  // q of t node j is q0 R^j (formed per node: two registers instead of five
  // held across the node loop; the products are the ones a table would hold)
  double q0, R;
  double ia2;  // 1 / a^2
  Decision D0, D4;
  bool ok0, ok4, shared;
  __device__ double qh(int j) const {
    if (q0 < 0.0) return -1.0;
    const double R2 = R * R;
    const double Rj = j == 1 ? R : j == 2 ? R2 : j == 3 ? R2 * R : R2 * R2;
    return j == 0 ? q0 : q0 * Rj;
  }
};
__device__ inline L0Hints l0_hints(double x, double lb, double ub, double a, double err) {
  L0Hints H;
  H.q0 = -1.0;
  H.R = 0.0;
  H.D0 = Decision{0, 0, 0};
  H.D4 = Decision{0, 0, 0};
  H.ok0 = H.ok4 = H.shared = false;
  const double a2 = a * a;
  const double ia2 = 1.0 / a2;
  H.ia2 = ia2;
  // values only (the fp32 decision estimates below have a 1e-5 guard band)
  const double q0 = exp_node((-kPi2 * ((x - lb) * ia2)) * 0.5);
  const double R = exp_node((kPi2 * (ub - lb)) * (0.125 * ia2));
  if (q0 > 1e-280 && R < 1e10 && x - lb > 0) {
    H.q0 = q0;
    H.R = R;
  }
  if (x - ub > 0) {
    float args0, args4;
    H.ok0 = decide32((x - lb) * ia2, err, H.D0, args0);
    H.ok4 = decide32((x - ub) * ia2, err, H.D4, args4);
    H.shared = H.ok0 && H.ok4 && args0 < 0.5f && H.D0.small == H.D4.small && H.D0.K == H.D4.K;
  }
  return H;
}
// t node j (0..4: lb, d, c, e, ub) of the trial's root t interval: its value
// (kAdaptT: pdf_sv / st; kAdaptTZ: the z integral's root estimate / st),
// kFlagExact in flags for an ambiguous decision or a near-tie, pend = the z
// integral asks for refinement.
template <int MODE>
__device__ inline double l0_node(const Trial& tr, const Params& P, const Knobs& K, double lb,
                                 double ub, const L0Hints& H, int j, const ZGrid& G, int& flags,
                                 bool& pend, long long& ne, const double* stab = nullptr) {
  const double a = P.a, sv = P.sv, err = K.err;
  const double x = tr.x, v = tr.v, z = tr.z;
  const double iw = 1.0 / (ub - lb);
  const double c = (ub + lb) / 2.;
  const double d = (lb + c) / 2., e = (c + ub) / 2.;
  const double tc = j == 0 ? lb : j == 1 ? d : j == 2 ? c : j == 3 ? e : ub;
  const double qh = H.qh(j);
  const bool known = j == 0 ? H.ok0 : (j == 4 ? H.ok4 : H.shared);
  const TNode T = tnode_setup_r(x - tc, v, sv, a, H.ia2, err, qh, known, j == 4 ? H.D4 : H.D0);
  pend = false;
  if (T.amb) {
    flags |= kFlagExact;
    return 0.0;
  }
  if (MODE == kAdaptTZ) {
    const double iZz = 1.0 / ((z + tr.sz / 2.) - (z - tr.sz / 2.));
    return inner_root(T, G, iZz, v, sv, a, K, flags, ne, pend, stab) * iw;
  }
  ne += 1;
  return tnode_pdf_sv(T, z, v, sv, a) * iw;
}

// The engine's level 0 of one trial (as fast_level0, on the table's z grid):
// kFinal (p), kTree (f[], pend) or kExact.
// KEEP_F = false (the lean pass, which never reads f[]): the root Simpson
// sums are accumulated as the t nodes complete, in the reference's
// expression order (three registers across the node loop instead of five).
// UNROLL: the t-node loop fully unrolled (node positions, q hints and
// accumulators without per-node selects or loop-carried copies; 5x the code).
// The lean pass unrolls its boundary-uniform call site: 127 VGPRs = 4
// waves/SIMD instead of 168 = 3, and C3's level 0 -13%. So do the per-node and
// per-trial-parameter level-0 passes (fast_level0: no scratch, node kernel
// -18%); the engine's level 0 keeps the loop (measured: the unrolled copy
// slows its stress set 4%).
// Overflowed drift factors (tnode_pdf_sv_grid5): kAdaptTZ's t-node root
// grids hand them to z walks in every pass (inner_root); kAdaptZ's root grid
// takes the literal form when LITERAL (the engine's own level 0, not
// unrolled), otherwise (the unrolled level-0-only passes: lean, small,
// per-node / per-trial fast) the trial returns kTree, i.e. it is handed to the
// engine — every call sequence gives it the same bits.
template <int MODE, bool KEEP_F = true, bool UNROLL = false, bool LITERAL = !UNROLL>
__device__ inline int eng_level0_t(const Trial& tr, const Params& P, const Knobs& K,
                                   const ZGrid& G, double& p, double (&f)[5], long long& ne,
                                   unsigned& pend, const double* stab = nullptr) {
  p = 0.0;
  pend = 0u;
  if (!tr.valid) return kFinal;
  double lb, ub;
  tree_root<MODE>(tr, P, lb, ub);
  // formed here: a one-bit mask across the node loop instead of a double
  const bool structural = (MODE == kAdaptZ) ? tr.x - P.t <= 0 : tr.x - lb <= 0;
  int flags = 0;
  if (MODE == kAdaptZ) {
    const double iw = 1.0 / (ub - lb);
    const TNode T = tnode_setup(tr.x - P.t, tr.v, P.sv, P.a, K.err);
    if (T.amb) return kExact;
    // (kAdaptZ: the root grid's values are the tree's; an overflow hands a
    // level-0-only pass's trial to the engine, which uses the literal values)
    if (!tnode_pdf_sv_grid5<LITERAL>(T, G, tr.v, P.sv, P.a, f, stab) && !LITERAL) return kTree;
#pragma unroll
    for (int i = 0; i < 5; ++i) f[i] = f[i] * iw;
    ne += 5;
  } else {
    const L0Hints H = l0_hints(tr.x, lb, ub, P.a, K.err);
    if (!KEEP_F) {
      // X, Y, Z after node j:  0: f0 | 1: f0, f0+4f1 | 2: f2, f0+4f2, Sl |
      // 3: f2+4f3, f0+4f2, Sl | 4: -> S = h6((f0+4f2)+f4), Sr = h12((f2+4f3)+f4)
      const double h = ub - lb;
      double X = 0.0, Y = 0.0, Z = 0.0, y4 = 0.0;
#define WFPT_L0_ACC_NODE(j)                                                      \
  {                                                                              \
    bool pj;                                                                     \
    const double y = l0_node<MODE>(tr, P, K, lb, ub, H, j, G, flags, pj, ne, stab);  \
    if (flags & kFlagExact) return kExact;                                       \
    if (pj) pend |= 1u << ((j) * (kTreeW / 4));                                  \
    const double x4 = X + (4 * y);                                               \
    if ((j) == 2) Z = (h / 12) * (Y + y);                                        \
    Y = ((j) == 1 || (j) == 2) ? x4 : Y;                                         \
    X = ((j) == 0 || (j) == 2) ? y : ((j) == 3 ? x4 : X);                        \
    y4 = y;                                                                      \
  }
      if constexpr (UNROLL) {
#pragma unroll
        for (int j = 0; j < 5; ++j) WFPT_L0_ACC_NODE(j)
      } else {
#pragma unroll 1
        for (int j = 0; j < 5; ++j) WFPT_L0_ACC_NODE(j)
      }
#undef WFPT_L0_ACC_NODE
      if (pend) return kTree;
      Simp s;
      s.S = (h / 6) * (Y + y4);
      s.Sl = Z;
      s.Sr = (h / 12) * (X + y4);
      s.S2 = s.Sl + s.Sr;
      const int bottom = K.n_st;
      const bool refine = simpson_refine(s.S, s.S2, K.simps_err, bottom, flags);
      if (flags & kFlagExact) return kExact;
      if (refine) return kTree;
      p = s.S2 + (s.S2 - s.S) / 15;
      if (p > kExactBelow || structural) return kFinal;
      if (!tiny_absorbed(p, P.p_outlier, K.w_outlier)) return kExact;
      p = 0.0;
      return kFinal;
    }
#define WFPT_L0_F_NODE(j)                                                        \
  {                                                                              \
    bool pj;                                                                     \
    const double y = l0_node<MODE>(tr, P, K, lb, ub, H, j, G, flags, pj, ne, stab);  \
    if (flags & kFlagExact) return kExact;                                       \
    if (pj) pend |= 1u << ((j) * (kTreeW / 4));                                  \
    if ((j) == 0) f[0] = y;                                                      \
    else if ((j) == 1) f[1] = y;                                                 \
    else if ((j) == 2) f[2] = y;                                                 \
    else if ((j) == 3) f[3] = y;                                                 \
    else f[4] = y;                                                               \
  }
    if constexpr (UNROLL) {
#pragma unroll
      for (int j = 0; j < 5; ++j) WFPT_L0_F_NODE(j)
    } else {
#pragma unroll 1
      for (int j = 0; j < 5; ++j) WFPT_L0_F_NODE(j)
    }
#undef WFPT_L0_F_NODE
  }
  if (pend) return kTree;
  const Simp s = simp5(ub - lb, f[0], f[1], f[2], f[3], f[4]);
  const int bottom = (MODE == kAdaptZ) ? K.n_sz : K.n_st;
  const bool refine = simpson_refine(s.S, s.S2, K.simps_err, bottom, flags);
  if (flags & kFlagExact) return kExact;
  if (refine) return kTree;
  p = s.S2 + (s.S2 - s.S) / 15;
  if (p > kExactBelow || structural) return kFinal;
  if (!tiny_absorbed(p, P.p_outlier, K.w_outlier)) return kExact;
  p = 0.0;
  return kFinal;
}
template <int MODE, bool UNROLL = false>
__device__ inline int eng_level0(double x0, const Params& P, const Knobs& K, const ZGrid& G,
                                 double& p, double (&f)[5], long long& ne, unsigned& pend) {
  return eng_level0_t<MODE, true, UNROLL>(trial_setup(x0, P), P, K, G, p, f, ne, pend);
}

// Level-0 pass of one trial for an adaptive (or direct) MODE, one trial per
// lane (the direct family and the per-node path): the reference's prologue +
// root aux node of every adaptive Simpson it runs (1, 5, 5 or 25 pdf_sv
// evaluations).
//   kFinal: p is the trial density (0 for invalid parameters);
//   kTree:  the root stop test asks for refinement, or (kAdaptTZ) some t
//           node's z integral needs refinement (bit k of `pend`: tree point
//           k * kTreeW / 4); f[] = the root interval's values at lb, d, c, e, ub;
//   kExact: the value hinges on last-bit rounding (recomputed exactly).
template <int MODE>
__device__ inline int fast_level0(double x0, const Params& P, const Knobs& K, double& p,
                                  double (&f)[5], long long& ne, int& flags, unsigned& pend) {
  const Trial tr = trial_setup(x0, P);
  p = 0.0;
  pend = 0u;
  if (!tr.valid) return kFinal;
  const double a = P.a, sv = P.sv, t = P.t, err = K.err;
  const double x = tr.x, v = tr.v, z = tr.z;
  if (MODE == kDirect) {
    ne += 1;
    p = pdf_sv(x - t, v, sv, a, z, err, flags);
    if (flags & kFlagExact) return kExact;
    if (p > kExactBelow || x - t <= 0) return kFinal;
    if (!tiny_absorbed(p, P.p_outlier, K.w_outlier)) return kExact;
    p = 0.0;
    return kFinal;
  }
  // adaptive families: the engine's level 0 (eng_level0, defined above) on
  // this trial's own root z grid
  ZGrid G{};
  if (MODE == kAdaptZ || MODE == kAdaptTZ)
    G = zgrid_setup(z - tr.sz / 2., z + tr.sz / 2., v, sv, a);
  (void)t;
  (void)x;
  return eng_level0<MODE, true>(x0, P, K, G, p, f, ne, pend);
}

// Per-call constants of the direct family (simple DDM: one pdf_sv per trial,
// pdf.pxi:74-102 at w = z) for both boundaries, computed once on the host with
// the device's operations (bit-identical): the flipped v and w (pdf.pxi:
// 116-118), sin(pi w) and 2 cos(pi w) of the large-time series (tnode_ftt),
// the drift exponent's trial-independent part (-v) a w, and 1 / a^2
// (tnode_setup). `ok`: trial_setup's validity tests that do not involve x.
struct DirectArgs {
  double v[2], w[2], s1[2], tc[2], dn[2];
  double ia2;
  int ok;
};
__host__ __device__ inline void direct_args(const Params& P, DirectArgs& D) {
  for (int b = 0; b < 2; ++b) {
    const double v = b ? -P.v : P.v, w = b ? 1. - P.z : P.z;
    D.v[b] = v;
    D.w[b] = w;
    double s1, c1;
    sincospi01(w, s1, c1);
    D.s1[b] = s1;
    D.tc[b] = c1 + c1;
    D.dn[b] = ((-v) * P.a) * w;
  }
  D.ia2 = 1.0 / (P.a * P.a);
  const double a = P.a, sv = P.sv, t = P.t, st0 = P.st, sz0 = P.sz;
  D.ok = !((P.z < 0) || (P.z > 1) || (a < 0) || (t < 0) || (st0 < 0) || (sv < 0) ||
           (sz0 < 0) || (sz0 > 1) || (P.z + sz0 / 2. > 1) || (P.z - sz0 / 2. < 0) ||
           (t - st0 / 2. < 0));
}

// fast_level0<kDirect> of a trial on boundary b with the call's DirectArgs:
// the same operations (trial_setup's validity, tnode_setup, tnode_pdf_sv, the
// settlement), with the trial-independent parts read from D.
__device__ inline int direct_level0(double x0, const Params& P, const Knobs& K,
                                    const DirectArgs& D, int b, double& p, long long& ne,
                                    int& flags) {
  p = 0.0;
  const double x = fabs(x0);
  if (!(D.ok && !((x - (P.t - P.st / 2.)) < 0))) return kFinal;
  const double a = P.a, sv = P.sv, t = P.t;
  const double v = D.v[b], w = D.w[b];
  ne += 1;
  const TNode T = tnode_setup_r(x - t, v, sv, a, D.ia2, K.err);
  if (T.amb) flags |= kFlagExact;
  if (T.pos) {
    const double f = tnode_ftt_sc(T, w, D.s1[b], D.tc[b]);
    if (sv == 0) {
      const double ex = exp_node(D.dn[b] - (T.vvx * 0.5));
      p = (f * ex) * T.sc;
    } else {
      p = tnode_pdf_sv(T, w, v, sv, a);  // (sv > 0: the general form)
    }
  }
  if (flags & kFlagExact) return kExact;
  if (p > kExactBelow || x - t <= 0) return kFinal;
  if (!tiny_absorbed(p, P.p_outlier, K.w_outlier)) return kExact;
  p = 0.0;
  return kFinal;
}

}  // namespace wfpt
