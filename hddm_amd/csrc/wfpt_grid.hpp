// wfpt_grid.hpp — the device density on a z grid: pdf_sv at the five equally
// spaced z nodes of one t node (tnode_pdf_sv_grid5, small_grid2d), the
// reference's Simpson estimates of an interval, a t node's root z integral
// (inner_root), the in-wave tree over the dyadic points (tree17) and the
// engine's per-call tables. The grids themselves are wfpt_zgrid.hpp's.
// Compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "wfpt_math.hpp"
#include "wfpt_quad.hpp"
#include "wfpt_series.hpp"
#include "wfpt_types.hpp"
#include "wfpt_zgrid.hpp"

#pragma clang fp contract(off)

namespace wfpt {

__device__ inline ZGrid zgrid_setup(double lb, double ub, double v, double sv, double a) {
  ZGrid G;
  const double c = (ub + lb) / 2.;
  G.g[0] = lb;
  G.g[1] = (lb + c) / 2.;
  G.g[2] = c;
  G.g[3] = (c + ub) / 2.;
  G.g[4] = ub;
  sincospi01(G.g[0], G.s0, G.c0);
  sincospi01(G.g[4], G.s4, G.c4);
  sincospi01((G.g[4] - G.g[0]) * 0.25, G.sd, G.cd);
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    if (sv == 0) {
      G.A[i] = ((-v) * a) * G.g[i];
    } else {
      const double azsv = (a * G.g[i]) * sv;
      G.A[i] = (azsv * azsv) - (((2.0 * a) * v) * G.g[i]);
    }
  }
  G.h6 = (G.g[4] - G.g[0]) / 6;
  G.h12 = (G.g[4] - G.g[0]) / 12;
  return G;
}

// Small-time series and drift factor of a grid in one 2-D recurrence.
// Every term of pdf.pxi:55-57 times the drift factor of
// pdf.pxi:95-101 is exp(phi(j, k)) with
//   phi(j, k) = m (g_j + 2k)^2 + c_j,   j = 0..4 (z node), k = lower..upper,
// a quadratic in (j, k) on the equally spaced grid: its second differences
// are constants (8m in k, 2 m h^2 + d2 in j, 4 m h mixed), so the whole
// 5 x K table follows from six exponentials by products (the 1-D form below
// takes 2 per term k plus 3 for the drift). Values only, like the 1-D
// recurrences: ~K^2/2 + K + 4 chained roundings (< 40 ulp at K <= 8), far
// inside kTieBand. Returns false, and the caller evaluates the grid the 1-D
// way, when a term or an intermediate ratio could leave the normal range
// (every exponent is affine or quadratic over the table: its corners bound
// it) or a node's series is not positive (the fix-up path's semantics).
__device__ inline bool small_grid2d(const TNode& T, const ZGrid& G, double sv, double (&out)[5]) {
  const int K = T.K;
  if (K > 8) return false;
  const int lower = (int)(-floor((K - 1) / 2.));
  const int upper = (int)ceil((K - 1) / 2.);
  const double m = T.m;
  // the drift exponent (A_i - vvx / 2 for sv = 0, (A_i - vvx) cden otherwise)
  // as one expression: the multiplier 1 is exact, so no per-node select
  const double dv = (sv == 0) ? T.vvx * 0.5 : T.vvx, dm = (sv == 0) ? 1.0 : T.cden;
  double c[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) c[i] = (G.A[i] - dv) * dm;
  const double lo2 = (double)(2 * lower);
  const double u0 = G.g[0] + lo2, u4 = G.g[4] + (double)(2 * upper);
  const double h = G.g[1] - G.g[0];
  const double d1 = c[1] - c[0];
  const double d2 = (c[2] - c[1]) - d1;
  const double a00 = m * (u0 * u0) + c[0];  // phi(0, lower)
  const double aR = m * (h * (2.0 * u0 + h)) + d1;  // phi(1, lower) - phi(0, lower)
  const double aQj = (2.0 * m) * (h * h) + d2;
  const double aP = (4.0 * m) * (u0 + 1.0);  // phi(0, lower + 1) - phi(0, lower)
  const double aQk = 8.0 * m;
  const double aQjk = (4.0 * m) * h;
  const double cmax = fmax(fmax(fmax(c[0], c[1]), fmax(c[2], c[3])), c[4]);
  const double cmin = fmin(fmin(fmin(c[0], c[1]), fmin(c[2], c[3])), c[4]);
  const double U = fmax(fabs(u0), fabs(u4));
  const double km1 = (double)(K - 1);
  // j-ratios at the table's corners (j = 0..3, k = lower..upper), k-ratios at
  // k = lower and upper - 1
  const double rmax = fmax(fmax(fabs(aR), fabs(aR + 3.0 * aQj)),
                           fmax(fabs(aR + km1 * aQjk), fabs((aR + 3.0 * aQj) + km1 * aQjk)));
  const double pmax = fmax(fabs(aP), fabs(aP + (km1 - 1.0) * aQk));
  const double qmax = fmax(fmax(fabs(aQj), fabs(aQk)), fabs(aQjk));
  constexpr double B = 640.0;
  const bool safe = (cmax < B) & (m * (U * U) + cmin > -B) & (fmax(fmax(rmax, pmax), qmax) < B);
  if (!safe) return false;
  double E0 = exp_val(a00), R0 = exp_val(aR), P = exp_val(aP);
  const double Qj = exp_val(aQj), Qk = exp_val(aQk), Qjk = exp_val(aQjk);
  double s[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) s[i] = 0.0;
  double k2 = lo2;
  for (int k = lower; k <= upper; ++k) {
    double E = E0, R = R0;
    s[0] = madd(G.g[0] + k2, E, s[0]);
#pragma unroll
    for (int i = 1; i < 5; ++i) {
      E = E * R;
      if (i < 4) R = R * Qj;
      s[i] = madd(G.g[i] + k2, E, s[i]);
    }
    E0 = E0 * P;
    P = P * Qk;
    R0 = R0 * Qjk;
    k2 = k2 + 2.0;
  }
  const double f = T.rn * T.sc;
  bool clean = true;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    out[i] = s[i] * f;
    clean = clean & (s[i] > 0) & !__builtin_isinf(out[i]);
  }
  return clean;
}

// pdf_sv at the 5 root-level z nodes of one t node (the values of
// tnode_pdf_sv at each node to a few ulp):
//   * small-t series: the exponents (g_j + 2k)^2 m are quadratic in j on the
//     equally spaced grid, so per term k two exponentials (j = 0 and the first
//     ratio) and one shared second-difference factor replace five; exponents
//     below -600 (subnormal territory) take the direct exps;
//   * large-t series: the Chebyshev recurrence in k from the rotated sin/cos;
//   * the drift factor exp(c_j): three exponentials and the second-difference
//     recurrence (direct exps when |c| > 600).
// stab (nullable): the grid's large-time sine table sin(k pi g_i), row k at
// stab + 5 k (k = 1..kSinK; SinTable); null: the Chebyshev recurrence in
// registers.
// Returns false when a node's drift factor overflowed with a positive series
// value (exp(c) = inf): then LITERAL fills that node with the reference's
// literal form (below); LITERAL = false (the level-0-only passes, whose
// register budget the rare form would take) leaves it inf. Either way the
// caller decides: a t node's root z grid (kAdaptTZ) hands such a node's z
// integral to a z walk, whose grids take the literal values.
template <bool LITERAL = true>
__device__ inline bool tnode_pdf_sv_grid5(const TNode& T, const ZGrid& G, double v, double sv,
                                          double a, double (&out)[5],
                                          const double* stab = nullptr) {
  double p[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) p[i] = 0.0;
  if (!T.pos) {
#pragma unroll
    for (int i = 0; i < 5; ++i) out[i] = 0.0;
    return true;
  }
  const int K = T.K;
  if (T.small && small_grid2d(T, G, sv, out)) return true;
  if (T.small) {
    const int lower = (int)(-floor((K - 1) / 2.));
    const int upper = (int)ceil((K - 1) / 2.);
    for (int k = lower; k <= upper; ++k) {
      const double k2 = (double)(2 * k);
      // the 2-D table above takes every grid it can, so this branch only sees
      // the rare ones (an end exponent in subnormal territory): one node per
      // trip, so the hot path's register allocation does not carry five
      // interleaved exponentials
#pragma unroll 1
      for (int i = 0; i < 5; ++i) {
        const double wi = pick5(G.g, i) + k2;
        put5(p, i, madd(wi, exp_sat((wi * wi) * T.m), pick5(p, i)));
      }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) p[i] = p[i] * T.rn;
  } else if (stab) {
    // the sines of the (wave-uniform) grid from the call's table: the same
    // values the recurrence below produces (sin_table), read with scalar
    // loads instead of carried in 15 vector registers per lane
    double e = T.m, r = T.m * T.q2;
    if (K >= 1) {
#pragma unroll
      for (int i = 0; i < 5; ++i) p[i] = T.m * stab[5 + i];
    }
    if (K <= kSinK) {
      for (int k = 2; k <= K; ++k) {
        e = e * r;
        r = r * T.q2;
        const double ke = (double)k * e;
#pragma unroll
        for (int i = 0; i < 5; ++i) p[i] = madd(ke, stab[5 * k + i], p[i]);
      }
    } else {
      // beyond the table (err far below 1e-10): the recurrence one node at
      // a time (few live registers)
#pragma unroll 1
      for (int i = 0; i < 5; ++i) {
        const double s1 = stab[5 + i];
        const double tci = sin_tc(G, i);
        double e1 = T.m, r1 = T.m * T.q2, sk = s1, skm1 = 0.0, pi = T.m * s1;
        for (int k = 2; k <= K; ++k) {
          e1 = e1 * r1;
          r1 = r1 * T.q2;
          const double sn = msub(tci, sk, skm1);
          skm1 = sk;
          sk = sn;
          pi = madd((double)k * e1, sk, pi);
        }
        put5(p, i, pi);
      }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) p[i] = p[i] * kPi;
  } else {
    double sj[5], cj[5];
    sj[0] = G.s0;
    cj[0] = G.c0;
    sj[4] = G.s4;
    cj[4] = G.c4;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      sj[j] = fma(sj[j - 1], G.cd, cj[j - 1] * G.sd);
      cj[j] = fma(cj[j - 1], G.cd, -(sj[j - 1] * G.sd));
    }
    double tc[5], sk[5], skm1[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      tc[i] = cj[i] + cj[i];
      sk[i] = sj[i];
      skm1[i] = 0.0;
      if (K >= 1) p[i] = T.m * sj[i];
    }
    // two terms per trip, the two sin registers swapping roles (no moves)
    double e = T.m, r = T.m * T.q2;
    int k = 2;
    for (; k + 1 <= K; k += 2) {
      e = e * r;
      r = r * T.q2;
      const double ke = (double)k * e;
      e = e * r;
      r = r * T.q2;
      const double ke1 = (double)(k + 1) * e;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        skm1[i] = msub(tc[i], sk[i], skm1[i]);  // sin(k pi w)
        p[i] = madd(ke, skm1[i], p[i]);
        sk[i] = msub(tc[i], skm1[i], sk[i]);    // sin((k+1) pi w)
        p[i] = madd(ke1, sk[i], p[i]);
      }
    }
    if (k <= K) {
      e = e * r;
      const double ke = (double)k * e;
#pragma unroll
      for (int i = 0; i < 5; ++i) p[i] = madd(ke, msub(tc[i], sk[i], skm1[i]), p[i]);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) p[i] = p[i] * kPi;
  }
  // exponent of the drift factor at each node (quadratic in g), formed where
  // it is used: A_i - vvx / 2 for sv = 0, (A_i - vvx) cden otherwise, as one
  // expression (the multiplier 1 is exact: no per-node select)
  const double dv = (sv == 0) ? T.vvx * 0.5 : T.vvx, dm = (sv == 0) ? 1.0 : T.cden;
  auto cexp = [&](int i) -> double { return (G.A[i] - dv) * dm; };
  double ex[5];
  const double c0 = cexp(0), c2 = cexp(2), c4 = cexp(4);
  const bool moderate = fabs(c0) < 600.0 && fabs(c2) < 600.0 && fabs(c4) < 600.0;
  if (moderate) {
    // c_j = c0 + j d1 + j(j-1)/2 d2  ->  E_j = E_{j-1} * R * Q^(j-1)
    const double c1 = cexp(1);
    const double d1 = c1 - c0;
    const double d2 = (c2 - c1) - d1;
    ex[0] = exp_val(c0);
    double rr = exp_val(d1);
    const double qd = exp_val(d2);
#pragma unroll
    for (int j = 1; j < 5; ++j) {
      ex[j] = ex[j - 1] * rr;
      rr = rr * qd;
    }
  } else {  // rare: one node per trip (register allocation as above)
#pragma unroll 1
    for (int i = 0; i < 5; ++i) {
      const double Ai = pick5(G.A, i);
      put5(ex, i, exp_sat((Ai - dv) * dm));
    }
  }
  // the common case: every series value positive and every product finite;
  // the rare fix-ups below run only on lanes that need one (same values)
  bool clean = true;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    out[i] = (p[i] * ex[i]) * T.sc;
    clean = clean & (p[i] > 0) & !__builtin_isinf(out[i]);
  }
  if (__builtin_expect(clean, 1)) return true;
  if (!LITERAL) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      double r2 = out[i];
      if (sv != 0 && p[i] < 0) r2 = __builtin_nan("");
      if (p[i] == 0) r2 = 0.0 * T.sc;
      ok = ok & !(__builtin_isinf(r2) && p[i] > 0);
      out[i] = r2;
    }
    return ok;
  }
  bool ok = true;
#pragma unroll 1
  for (int i = 0; i < 5; ++i) {
    double r2 = pick5(out, i);
    const double pi = pick5(p, i);
    if (sv != 0 && pi < 0) r2 = __builtin_nan("");  // log(p < 0) in the reference
    // exp(log 0 + c) = 0 even if e^c = inf; 0 * sc keeps the reference's
    // 0 / (a*a) = NaN at a == 0
    if (pi == 0) r2 = 0.0 * T.sc;
    // exp(c) overflow with a finite true value (sv > 0): the reference's
    // literal form exp(log p + c) / sqrt(sv^2 x + 1) / a^2 (pdf.pxi:102), a
    // value like the others (the stop tests keep their tie band). sv = 0: the
    // reference's p exp(c) / a^2 (pdf.pxi:85) overflows to inf as well.
    const bool ovf = __builtin_isinf(r2) && pi > 0;
    ok = ok & !ovf;
    if (ovf && sv != 0) {
      const double w = pick5(G.g, i);
      const double azsv = (a * w) * sv;
      r2 = (exp(log(pi) + (((azsv * azsv) - (((2.0 * a) * v) * w)) - T.vvx) /
                              (((2.0 * (sv * sv)) * T.xx) + 2.0)) /
            sqrt(((sv * sv) * T.xx) + 1.0)) /
           (a * a);
    }
    put5(out, i, r2);
  }
  return ok;
}

// The reference's Simpson estimates of one interval from its 5 values.
struct Simp {
  double S, Sl, Sr, S2;
};
__host__ __device__ inline Simp simp5(double h, double fb, double fd, double fm, double fe,
                                     double fu) {
  Simp s;
  s.S = (h / 6) * ((fb + (4 * fm)) + fu);
  s.Sl = (h / 12) * ((fb + (4 * fd)) + fm);
  s.Sr = (h / 12) * ((fm + (4 * fe)) + fu);
  s.S2 = s.Sl + s.Sr;
  return s;
}

// simp5 with the interval's weights h/6, h/12 precomputed (the same IEEE
// divisions of the same h: bit-identical).
__device__ inline Simp simp5p(double h6, double h12, double fb, double fd, double fm, double fe,
                              double fu) {
  Simp s;
  s.S = h6 * ((fb + (4 * fm)) + fu);
  s.Sl = h12 * ((fb + (4 * fd)) + fm);
  s.Sr = h12 * ((fm + (4 * fe)) + fu);
  s.S2 = s.Sl + s.Sr;
  return s;
}
// The leaf value S2 + (S2 - S) / 15 of an interval that stops refining
// (integrate.pxi:106,171), with 1/15 as a product: a value, never a decision
// input at its own level (the stop test reads S and S2), within an ulp of the
// quotient. Every site that must produce the same bits for a t node's root z
// integral (inner_root, the engine's task completion) uses this.
constexpr double kInv15 = 1.0 / 15.0;
__device__ inline double simp_value(const Simp& s) { return s.S2 + (s.S2 - s.S) * kInv15; }

// The z integral at one t node (adaptiveSimpsons_1D over z, integrate.pxi:
// 114-141), root level only: the root's 5 evaluations 5-wide on the grid and
// its stop test. repair = the test asks for refinement (the value is then the
// root estimate; the caller defers the trial).
__device__ inline double inner_root(const TNode& T, const ZGrid& G, double iZz, double v,
                                    double sv, double a, const Knobs& K, int& flags,
                                    long long& ne, bool& repair,
                                    const double* stab = nullptr) {
  double f[5];
  // an overflowed drift factor marks the z integral as refining: in every
  // call sequence the t node's value then comes from a z walk, whose grids
  // take the literal form (its values here are not used; their stop test
  // raises no flag)
  const bool ovf = !tnode_pdf_sv_grid5<false>(T, G, v, sv, a, f, stab);
#pragma unroll
  for (int i = 0; i < 5; ++i) f[i] = f[i] * iZz;
  ne += 5;
  const Simp s = simp5p(G.h6, G.h12, f[0], f[1], f[2], f[3], f[4]);
  int fl = 0;
  repair = simpson_refine(s.S, s.S2, K.simps_err, K.n_sz, fl) || ovf;
  flags |= ovf ? 0 : fl;
  return simp_value(s);
}

// The reference's recursion (adaptiveSimpsonsAux, integrate.pxi:94-112 /
// 159-178) over a tree of depth <= kTreeDepth whose values f[k] at the dyadic
// points P[k] of the root interval are in registers, in straight-line form:
// prologue S of the root, then per visited interval its S2 from its 5 values,
// the stop test (bottom = depth - level, eps halved per level) and either the
// leaf value S2 + (S2 - S) / 15 or left + right. lv: the deepest level whose
// values are known. Returns the integral when no visited interval asks for
// values below lv; otherwise need = the refining intervals of level lv
// (bit m: interval m of that level), and for lv == kTreeDepth those mean a
// deeper tree. flags gets kFlagExact for a stop test inside kTieBand; nref =
// visited refined intervals (2 new nodes x 2 evaluations each). used
// (optional): bit k set for every point f[k] the recursion read (the points
// the reference evaluates).
__host__ __device__ inline double tree17(const double (&f)[kTreePoints],
                                         const double (&P)[kTreePoints], double err, int depth,
                                         int lv, int& flags, unsigned& need, int& nref,
                                         unsigned* used = nullptr) {
  need = 0u;
  nref = 0;
  if (used) *used = 0x11111u;  // points 0, 4, 8, 12, 16
  const double h0 = P[kTreeW] - P[0];
  const double S0 = (h0 / 6) * ((f[0] + (4 * f[8])) + f[16]);
  const Simp r = simp5(h0, f[0], f[4], f[8], f[12], f[16]);
  if (!simpson_refine(S0, r.S2, err, depth, flags)) return r.S2 + (r.S2 - S0) / 15;
  nref = 1;
  if (lv == 0) {
    need = 1u;
    return 0.0;
  }
  double vh[2];
  if (used) *used |= 0x4444u;  // the halves' aux points 2, 6, 10, 14
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int lo = 8 * m;
    const double S = m ? r.Sr : r.Sl;
    const Simp s = simp5(P[lo + 8] - P[lo], f[lo], f[lo + 2], f[lo + 4], f[lo + 6], f[lo + 8]);
    if (!simpson_refine(S, s.S2, err / 2, depth - 1, flags)) {
      vh[m] = s.S2 + (s.S2 - S) / 15;
      continue;
    }
    ++nref;
    if (lv == 1) {
      need |= 1u << m;
      vh[m] = 0.0;
      continue;
    }
    if (used) *used |= 0xAAu << lo;  // the half's quarter aux points lo + 1, 3, 5, 7
    double vq[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int l2 = lo + 4 * q;
      const double Sq = q ? s.Sr : s.Sl;
      const Simp u = simp5(P[l2 + 4] - P[l2], f[l2], f[l2 + 1], f[l2 + 2], f[l2 + 3], f[l2 + 4]);
      if (simpson_refine(Sq, u.S2, (err / 2) / 2, depth - 2, flags)) need |= 1u << (2 * m + q);
      vq[q] = u.S2 + (u.S2 - Sq) / 15;
    }
    vh[m] = vq[0] + vq[1];
  }
  return need ? 0.0 : vh[0] + vh[1];
}

// Per-call tables of the engine (host-computed from the call's parameters,
// passed by value): the z grids of both boundaries (trial_setup's flip x > 0:
// v = -v, z = 1 - z), the dyadic points of the t tree and of both z trees.
struct EngTables {
  ZGrid G[2][4];
  double tP[kTreePoints];
  double zP[2][kTreePoints];
  double iz[2];  // 1 / (ub_z - lb_z) per boundary
};

__host__ __device__ inline void eng_tables(const Params& P, EngTables& T) {
  for (int k = 0; k < kTreePoints; ++k) T.tP[k] = dyadic_point(P.t - P.st / 2., P.t + P.st / 2., k);
  for (int flip = 0; flip < 2; ++flip) {
    const double zf = flip ? 1. - P.z : P.z, vf = flip ? -P.v : P.v;
    const double zl = zf - P.sz / 2., zu = zf + P.sz / 2.;
    for (int sel = 0; sel < 4; ++sel) T.G[flip][sel] = zgrid_of(zl, zu, sel, vf, P.sv, P.a);
    for (int k = 0; k < kTreePoints; ++k) T.zP[flip][k] = dyadic_point(zl, zu, k);
    T.iz[flip] = 1.0 / (zu - zl);
  }
}

}  // namespace wfpt
