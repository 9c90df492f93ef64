// wfpt_lean.hpp — the wave-level device code of the lean pass's uniform waves.
//
// Uniform waves of the lean pass (lean_kernel<kAdaptTZ>). A resident dataset
// is ordered by boundary, then |rt|, so the 64 trials of a wave almost always
// share the series decision (small, K; pdf.pxi:36-60) of each of their five
// t nodes. Such a wave keeps the five decisions in scalar registers and runs
// lean_uniform_level0: per lane the same floating-point operations on the
// same operands in the same order as eng_level0_t<kAdaptTZ, false, true>, but
// everything that depends on (grid, K) alone is read from a host table
// (UniformTab) with scalar loads, both series loops are scalar-counted, and
// small_grid2d's per-node range guard is replaced by one per-trial bound
// (uniform_guard). Any other wave runs eng_level0_t unchanged.
// The tables and their proofs are wfpt_lean_tables.hpp's.
// Device code. Compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "wfpt_grid.hpp"
#include "wfpt_lean_tables.hpp"
#include "wfpt_level0.hpp"
#include "wfpt_math.hpp"
#include "wfpt_quad.hpp"
#include "wfpt_series.hpp"
#include "wfpt_types.hpp"
#include "wfpt_zgrid.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// The five decisions of a one-boundary wave from the table. Every lane of the
// wave is active; lane l holds edge[l]. xs: the lane's |rt|. The wave's own
// lanes are a prefix (own = ballot of them, lane 0 is one); if their |rt| is
// nondecreasing across lanes (checked here, never assumed), tt_j = (x - tc_j)
// * ia2 is nondecreasing too (a rounded subtraction and a product with ia2 >
// 0 are monotone), so the tt of the first and the last own lane bracket every
// own lane's at each node: both inside the same piece means every lane's is.
// True: kpack / smask hold the codes (wave-uniform). False: no answer.
__device__ inline bool table_decisions(const DecisionTab& D, double xs, double lb, double ub,
                                       double ia2, unsigned long long own, int lane,
                                       unsigned& kpack, unsigned& smask) {
  kpack = 0u;
  smask = 0u;
  const double prev = __shfl_up(xs, 1);
  const bool mine = ((own >> lane) & 1ull) != 0ull;
  if (__ballot(mine && !(prev <= xs)) != 0ull) return false;
  const int last = __popcll(own) - 1;
  const double xmin = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(xs), 0),
                                       __builtin_amdgcn_readlane(__double2loint(xs), 0));
  const double xmax = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(xs), last),
                                       __builtin_amdgcn_readlane(__double2loint(xs), last));
  const double e = D.edge[lane];
  const double c = (ub + lb) / 2.;
  const double d = (lb + c) / 2., f = (c + ub) / 2.;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const double tc = j == 0 ? lb : j == 1 ? d : j == 2 ? c : j == 3 ? f : ub;
    const int n0 = __popcll(__ballot(e <= (xmin - tc) * ia2));
    const int n1 = __popcll(__ballot(e <= (xmax - tc) * ia2));
    const unsigned code = D.code[(n0 >> 1) & (kDecPieces - 1)];
    ok = ok && n0 == n1 && (n0 & 1) != 0 && code != 0u;
    kpack |= (code & 15u) << (4 * j);
    smask |= ((code >> 4) & 1u) << j;
  }
  return ok;
}

// For a wave table_decisions did not settle: true if the table nevertheless
// proves it non-uniform. The own lanes' |rt| are nondecreasing, both extremes
// lie inside a piece the table holds at every node, and at some node in two
// different pieces with different codes: there the first and the last own
// lane have different reference decisions, so no vote over the lanes' own
// decisions (l0_decisions) can pass and the per-lane pre-pass is wasted work.
// The same lookups as table_decisions, redone here (a handful of waves per
// launch) so that the settled waves' path stays as it is.
__device__ inline bool table_split(const DecisionTab& D, double xs, double lb, double ub,
                                   double ia2, unsigned long long own, int lane) {
  const double prev = __shfl_up(xs, 1);
  const bool mine = ((own >> lane) & 1ull) != 0ull;
  if (__ballot(mine && !(prev <= xs)) != 0ull) return false;
  const int last = __popcll(own) - 1;
  const double xmin = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(xs), 0),
                                       __builtin_amdgcn_readlane(__double2loint(xs), 0));
  const double xmax = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(xs), last),
                                       __builtin_amdgcn_readlane(__double2loint(xs), last));
  const double e = D.edge[lane];
  const double c = (ub + lb) / 2.;
  const double d = (lb + c) / 2., f = (c + ub) / 2.;
  bool inside = true, differ = false;
#pragma unroll 1
  for (int j = 0; j < 5; ++j) {
    const double tc = j == 0 ? lb : j == 1 ? d : j == 2 ? c : j == 3 ? f : ub;
    const int n0 = __popcll(__ballot(e <= (xmin - tc) * ia2));
    const int n1 = __popcll(__ballot(e <= (xmax - tc) * ia2));
    const unsigned c0 = D.code[(n0 >> 1) & (kDecPieces - 1)];
    const unsigned c1 = D.code[(n1 >> 1) & (kDecPieces - 1)];
    inside = inside && (n0 & 1) != 0 && (n1 & 1) != 0 && c0 != 0u && c1 != 0u;
    differ = differ || (n0 != n1 && c0 != c1);
  }
  return inside && differ;
}

// Each lane's own five decisions, by today's operations: l0_hints for t nodes
// 0 and 4 and its `shared` rule, decide32 for nodes 1..3 otherwise. False
// (the lane's wave takes eng_level0_t) for invalid parameters, a node with
// x - t_node <= 0, no recurrence hint q0, an fp32 estimate that asks for the
// fp64 decision (within 1e-5 of a threshold), or a K beyond the tables. On
// true: kpack = K_j << 4j, smask bit j = small_j, H = the trial's hints.
__device__ inline bool l0_decisions(const Trial& tr, const Params& P, const Knobs& K, L0Hints& H,
                                    unsigned& kpack, unsigned& smask) {
  kpack = 0u;
  smask = 0u;
  double lb, ub;
  tree_root<kAdaptTZ>(tr, P, lb, ub);
  H = l0_hints(tr.x, lb, ub, P.a, K.err);
  bool ok = tr.valid && (tr.x - ub > 0) && H.q0 >= 0.0 && H.ok0 && H.ok4;
  if (!ok) return false;
  const double c = (ub + lb) / 2.;
  const double d = (lb + c) / 2., e = (c + ub) / 2.;
  auto put = [&](int j, const Decision& D) {
    ok = ok && D.amb == 0 && D.K >= 1 && D.K <= (D.small ? kUniK : kSinK);
    kpack |= (unsigned)(D.K & 15) << (4 * j);
    smask |= (D.small ? 1u : 0u) << j;
  };
  put(0, H.D0);
  put(4, H.D4);
  if (H.shared) {
    put(1, H.D0);
    put(2, H.D0);
    put(3, H.D0);
  } else {
#pragma unroll 1
    for (int j = 1; j < 4; ++j) {
      const double tc = j == 1 ? d : j == 2 ? c : e;
      Decision D{0, 0, 0};
      float args;
      ok = decide32((tr.x - tc) * H.ia2, K.err, D, args) && ok;
      put(j, D);
    }
  }
  return ok;
}

// small_grid2d with wave-uniform K, past its guard (uniform_guard passed):
// the same exponents, exponentials and products per lane, the (grid, K)
// operands from the table. c: the drift exponents of z nodes 0..2. smin: the
// running minimum of the series values (lean_uniform_level0's clean test).
__device__ inline void small_grid2d_u(double m, double f, double c0, double c1, double c2,
                                      const UniformTab& U, int K, double (&out)[5], double& smin) {
  const UniformK& C = U.k[K];
  const int lower = -((K - 1) >> 1), upper = K >> 1;  // -floor((K-1)/2.), ceil((K-1)/2.)
  const double d1 = c1 - c0;
  const double d2 = (c2 - c1) - d1;
  const double a00 = m * C.u0u0 + c0;
  const double aR = m * C.hh2 + d1;
  const double aQj = (2.0 * m) * C.hh + d2;
  const double aP = (4.0 * m) * C.u0p1;
  const double aQk = 8.0 * m;
  const double aQjk = (4.0 * m) * C.h;
  const double ax[6] = {a00, aR, aP, aQj, aQk, aQjk};
  double ey[6];
  exp_val_n<6>(ax, ey);
  double E0 = ey[0], R0 = ey[1], P = ey[2];
  const double Qj = ey[3], Qk = ey[4], Qjk = ey[5];
  double s[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) s[i] = 0.0;
#pragma unroll 1
  for (int k = lower; k <= upper; ++k) {
    const double* u = U.u[k + 4];
    double E = E0, R = R0;
    s[0] = madd(u[0], E, s[0]);
#pragma unroll
    for (int i = 1; i < 5; ++i) {
      E = E * R;
      if (i < 4) R = R * Qj;
      s[i] = madd(u[i], E, s[i]);
    }
    E0 = E0 * P;
    P = P * Qk;
    R0 = R0 * Qjk;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    out[i] = s[i] * f;
    smin = min_raw(smin, s[i]);
  }
}

// eng_level0_t<kAdaptTZ, false, true> of one trial of a uniform wave: kpack,
// smask (wave-uniform: l0_decisions of every lane agree), H the lane's own
// hints, uniform_guard passed. bail: a node may not have been clean (a
// non-positive series value, an infinite product), which the fix-up code of
// tnode_pdf_sv_grid5 handles: the caller reruns the whole wave on
// eng_level0_t and discards this result.
//
// The clean test. eng_level0_t's node is clean when each of its five series
// values is > 0 and none of the five products f_i is infinite. Here the 25
// series values feed one running fmin (smin) and the products are not tested
// at all: bail = !(smin > 0) || the root's S2 is not finite. That bails
// whenever some node is not clean (and possibly more often, never less; a
// bail only reruns the wave on the generic site, whose bits are the
// contract, so a superset is safe and a subset would not be):
//   * a series value <= 0 makes smin <= 0 or NaN (v_min_f64 passes over a NaN
//     operand or returns it, never a larger value);
//   * a NaN series value makes its product f_i NaN, an infinite product is
//     non-finite already, and non-finiteness survives every later operation
//     on the way to the root's S2: a sum with a non-finite addend and a
//     product with a non-finite factor are non-finite (inf - inf and inf * 0
//     give NaN). f_i is a factor of f_i * iZz, that an addend of the node's
//     Sl or Sr (simp5p), those the addends of its S2, S2 an addend of
//     simp_value, that a factor of y, and each of the five y an addend of
//     the root's Sl or Sr, whose sum is the root's S2.
__device__ inline int lean_uniform_level0(const Trial& tr, const Params& P, const Knobs& K,
                                          const ZGrid& G, const UniformTab& U, const double* stab,
                                          const L0Hints& H, unsigned kpack, unsigned smask,
                                          double& p, long long& ne, unsigned& pend, bool& bail) {
  p = 0.0;
  pend = 0u;
  double lb, ub;
  tree_root<kAdaptTZ>(tr, P, lb, ub);
  const double sv = P.sv, v = tr.v, x = tr.x;
  const double iw = 1.0 / (ub - lb);
  const double tcc = (ub + lb) / 2.;
  const double tcd = (lb + tcc) / 2., tce = (tcc + ub) / 2.;
  const double iZz = 1.0 / ((tr.z + tr.sz / 2.) - (tr.z - tr.sz / 2.));
  const double h = ub - lb;
  int flags = 0;
  double smin = __builtin_inf();
  double X = 0.0, Y = 0.0, Z = 0.0, y4 = 0.0;
  // unrolled like eng_level0_t's node loop (a rolled loop measured 3% slower):
  // tc, qh(j) and the Simpson bookkeeping fold per node
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int Kj = (int)((kpack >> (4 * j)) & 15u);
    const bool small = ((smask >> j) & 1u) != 0u;
    const double tc = j == 0 ? lb : j == 1 ? tcd : j == 2 ? tcc : j == 3 ? tce : ub;
    // tnode_setup_r with the known decision
    const double xx = x - tc;
    const double tt = xx * H.ia2;
    double sc = H.ia2, cden = 0.0;
    if (sv != 0) {
      const double r = rsqrt(((sv * sv) * xx) + 1.0);
      cden = (0.5 * r) * r;
      sc = sc * r;
    }
    const double vvx = (v * v) * xx;
    const double dv = (sv == 0) ? vvx * 0.5 : vvx, dm = (sv == 0) ? 1.0 : cden;
    const double c0 = (G.A[0] - dv) * dm, c1 = (G.A[1] - dv) * dm, c2 = (G.A[2] - dv) * dm;
    double f[5];
    if (small) {
      const double r = rsqrt(tt), r2 = r * r;
      const double rn = kInvSqrt2Pi * (r2 * r);
      const double m = -0.5 * r2;
      small_grid2d_u(m, rn * sc, c0, c1, c2, U, Kj, f, smin);
    } else {
      // (H.q0 >= 0: the recurrence's q, as tnode_setup_r takes it from qh(j))
      const double m = H.qh(j);
      const double q2 = m * m;
      double pp[5];
      double e = m, r = m * q2;
#pragma unroll
      for (int i = 0; i < 5; ++i) pp[i] = m * stab[5 + i];
#pragma unroll 1
      for (int k = 2; k <= Kj; ++k) {
        e = e * r;
        r = r * q2;
        const double ke = (double)k * e;
#pragma unroll
        for (int i = 0; i < 5; ++i) pp[i] = madd(ke, stab[5 * k + i], pp[i]);
      }
#pragma unroll
      for (int i = 0; i < 5; ++i) pp[i] = pp[i] * kPi;
      // the drift factors (|c| < 600 by uniform_guard: the `moderate` form)
      const double d1 = c1 - c0;
      const double d2 = (c2 - c1) - d1;
      const double dx[3] = {c0, d1, d2};
      double dy[3];
      exp_val_n<3>(dx, dy);
      double ex = dy[0];
      double rr = dy[1];
      const double qd = dy[2];
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        f[i] = (pp[i] * ex) * sc;
        smin = min_raw(smin, pp[i]);
        ex = ex * rr;
        rr = rr * qd;
      }
    }
    // inner_root
#pragma unroll
    for (int i = 0; i < 5; ++i) f[i] = f[i] * iZz;
    ne += 5;
    const Simp s = simp5p(G.h6, G.h12, f[0], f[1], f[2], f[3], f[4]);
    if (simpson_refine(s.S, s.S2, K.simps_err, K.n_sz, flags)) pend |= 1u << (j * (kTreeW / 4));
    const double y = simp_value(s) * iw;
    // the root Simpson sums, as eng_level0_t (KEEP_F = false)
    const double x4 = X + (4 * y);
    if (j == 2) Z = (h / 12) * (Y + y);
    Y = (j == 1 || j == 2) ? x4 : Y;
    X = (j == 0 || j == 2) ? y : (j == 3 ? x4 : X);
    y4 = y;
  }
  Simp s;
  s.S = (h / 6) * (Y + y4);
  s.Sl = Z;
  s.Sr = (h / 12) * (X + y4);
  s.S2 = s.Sl + s.Sr;
  bail = !(smin > 0) || !__builtin_isfinite(s.S2);
  if (flags & kFlagExact) return kExact;
  if (pend) return kTree;
  const bool refine = simpson_refine(s.S, s.S2, K.simps_err, K.n_st, flags);
  if (flags & kFlagExact) return kExact;
  if (refine) return kTree;
  p = s.S2 + (s.S2 - s.S) / 15;
  if (p > kExactBelow) return kFinal;  // (x - lb > 0: never structural)
  if (!tiny_absorbed(p, P.p_outlier, K.w_outlier)) return kExact;
  p = 0.0;
  return kFinal;
}

}  // namespace wfpt
