// wfpt_series.hpp — the per-t-node series of the device density (ftt_01w and
// pdf_sv, src/pdf.pxi:28-102) for one-trial-per-lane execution:
//   * every *decision* (series branch, term count K) is computed with the same
//     IEEE operations in the same order as the reference; a decision within
//     1e-12 of a threshold sends the trial to the exact path (wfpt_exact.hpp);
//   * work that depends only on the non-decision time node t (the series
//     branch and K, sqrt/log terms, sv normalisers) is hoisted out of the z
//     integral: one `TNode` per t node serves all z nodes.
// Device code. Compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "wfpt_exact.hpp"
#include "wfpt_math.hpp"
#include "wfpt_types.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// ---------------------------------------------------------------------------
// Per-t-node quantities of ftt_01w / pdf_sv that do not depend on w (= z).
//
// Decisions (pos, small/large branch, K) are computed with the reference's
// exact operations. Values use cheaper equivalent forms whose rounding differs
// by a few ulp (trials whose value hinges on last-bit rounding are sent to the
// exact path, wfpt_exact.hpp):
//   * exp(-k^2 pi^2 tt/2) = q^(k^2), q = exp(-pi^2 tt/2), by two products per k;
//   * sin(k pi w) by the Chebyshev recurrence from one sincospi(w);
//   * exp(log p + c) = p * exp(c)  (overflow of exp(c) falls back to the
//     literal form; p < 0 keeps the reference's NaN from log);
//   * divisions by per-node constants become multiplications by reciprocals.
constexpr double kInvSqrt2Pi = 0.398942280401432677939946059934;  // 1 / sqrt(2 pi)

struct TNode {
  double xx;    // x - t_node: the `x` argument of pdf_sv
  double tt;    // xx / a^2 (pdf.pxi:98)
  double m;     // small-t: -1/(2 tt) exponent multiplier; large-t: q = exp(-pi^2 tt / 2)
  double q2;    // large-t: q^2
  double rn;    // small-t: 1 / sqrt(2 pi tt^3)  (pdf.pxi:57)
  double sc;    // 1/a^2, times 1/sqrt(sv^2 xx + 1) when sv > 0
  double cden;  // sv: 1 / (2 sv^2 xx + 2)
  double vvx;   // v^2 * xx
  int K;        // number of series terms (pdf.pxi:52, 60)
  int small;    // 1 => small-time series
  int pos;      // xx > 0 (else density 0, pdf.pxi:92)
  int amb;      // the decision sits within 1e-12 of a threshold: exact path
};

// Series branch and term count of one t node (pdf.pxi:36-60): small-time
// series iff ks < kl, K = ceil(min). kl and ks feed ONLY these two decisions.
struct Decision {
  int small, K, amb;
};

// fp32 estimate of the decision (~1e-7 relative). Returns false — the caller
// must then run the reference's fp64 operations — when any decision is within
// 1e-5 (relative) of flipping or an fp32 argument is out of range. args_out:
// the small-time log argument 2 sqrt(2 pi tt) err (for the monotonicity test
// of shared decisions).
__device__ inline bool decide32(double tt, double err, Decision& D, float& args_out) {
  args_out = 2.0f;
  if (!(tt > 1e-30 && tt < 1e30 && err > 1e-30 && err < 1e30)) return false;
  const float ttf = (float)tt, errf = (float)err;
  const float sqtf = sqrt32(ttf);
  const float ipsf = rcp32((float)kPi * sqtf);
  const float argl = ((float)kPi * ttf) * errf;
  const float args = (2.0f * sqrt32((2.0f * (float)kPi) * ttf)) * errf;
  args_out = args;
  const bool use_l = argl < 1.0f;
  const bool use_s = args < 1.0f;
  const float tol = 1e-5f;
  // |dL| <~ 1e-7 |L| from fp32 rounding + the hardware log; the relative error
  // it induces in kl/ks is <= |dL| / (2|L|) ~ 1e-7, 100x inside tol (and |L| >=
  // 0.1 is still required below, as for the correctly rounded logf).
  const bool rng = (use_l && !(argl > 1e-30f)) || (use_s && !(args > 1e-30f));
  if (rng) return false;
  const float Ll = use_l ? log32(argl) : -1.0f;
  const float Ls = use_s ? log32(args) : -1.0f;
  float klf = use_l ? sqrt32((-2.0f * Ll) * rcp32((float)kPi2 * ttf)) : ipsf;
  float ksf = use_s ? 2.0f + sqrt32((-2.0f * ttf) * Ls) : 2.0f;
  const float b2 = sqtf + 1.0f;
  const bool amb_t = fabsf(argl - 1.0f) <= tol || fabsf(args - 1.0f) <= tol;
  const bool amb_l = use_l && fabsf(klf - ipsf) <= tol * klf;
  const bool amb_s = use_s && fabsf(ksf - b2) <= tol * ksf;
  if (use_l) klf = (klf < ipsf) ? ipsf : klf;
  if (use_s) ksf = (ksf < b2) ? b2 : ksf;
  const float kk = (ksf < klf) ? ksf : klf;
  const bool amb_b = fabsf(ksf - klf) <= tol * klf;
  const bool amb_k = fabsf(kk - rintf(kk)) <= tol * kk;
  if (Ll > -0.1f || Ls > -0.1f || amb_t || amb_l || amb_s || amb_b || amb_k) return false;
  if (!(kk < 1e6f)) return false;  // huge / non-finite K: decide64's conversion
  D.small = ksf < klf;
  D.K = (int)ceilf(kk);
  D.amb = 0;
  return true;
}

// The reference's fp64 operations (pdf.pxi:36-60), reached when the fp32
// estimate is within 1e-5 of a threshold. OCML's log differs from glibc's by
// <= 1 ulp, so a decision within 1e-12 (relative) of a threshold is marked
// ambiguous and the trial goes to the exact path (glibc-equal log).
__device__ inline Decision decide64(double tt, double err) {
  double kl, ks;
  const double sqt = sqrt(tt);
  const double inv_pi_sqt = 1. / (kPi * sqt);
  const double arg_l = (kPi * tt) * err;
  const double arg_s = (2.0 * sqrt((2.0 * kPi) * tt)) * err;
  if (arg_l < 1.0) {
    kl = sqrt((-2.0 * log(arg_l)) / (kPi2 * tt));
    kl = (kl < inv_pi_sqt) ? inv_pi_sqt : kl;
  } else {
    kl = inv_pi_sqt;
  }
  if (arg_s < 1.0) {
    ks = 2.0 + sqrt((-2.0 * tt) * log(arg_s));
    const double b = sqt + 1.0;
    ks = (ks < b) ? b : ks;
  } else {
    ks = 2.0;
  }
  Decision D;
  D.small = ks < kl;
  const double kk = D.small ? ks : kl;
  D.K = wfpt_x::ref_int(ceil(kk));  // the reference's x86 conversion
  constexpr double tol = 1e-12;
  D.amb = fabs(arg_l - 1.0) <= tol || fabs(arg_s - 1.0) <= tol || fabs(ks - kl) <= tol * kl ||
          fabs(kk - rint(kk)) <= tol * kk;
  return D;
}

// qhint >= 0: exp(-pi^2 tt / 2) of this node computed by the caller (a
// recurrence over the t grid); < 0: computed here. has_known: `known` is the
// node's decision, established by the caller (shared over a trial's t grid).
// ia2: 1 / a^2 of the call, computed once by the caller. tt comes from a
// product: it feeds the fp32 decision estimate (1e-5 guard band) and values
// only; the fp64 decision, reached near a threshold, divides exactly as
// pdf.pxi:98.
__device__ inline TNode tnode_setup_r(double xx, double v, double sv, double a, double ia2,
                                      double err, double qhint = -1.0, bool has_known = false,
                                      Decision known = Decision{0, 0, 0}) {
  TNode T;
  T.xx = xx;
  T.pos = xx > 0;
  T.tt = 0.0;
  T.m = 0.0;
  T.q2 = 0.0;
  T.rn = 0.0;
  T.sc = 0.0;
  T.cden = 0.0;
  T.vvx = 0.0;
  T.K = 0;
  T.small = 0;
  T.amb = 0;
  if (!T.pos) return T;
  const double a2 = a * a;
  const double tt = xx * ia2;
  T.tt = tt;
  Decision D;
  float args;
  if (has_known) D = known;
  else if (!decide32(tt, err, D, args)) D = decide64(xx / a2, err);
  T.amb = D.amb;
  if (D.small) {
    T.small = 1;
    T.K = D.K;
    // values only: 1/sqrt(2 pi tt^3) and -1/(2 tt) from one rsqrt
    const double r = rsqrt(tt), r2 = r * r;
    T.rn = kInvSqrt2Pi * (r2 * r);
    T.m = -0.5 * r2;
  } else {
    T.small = 0;
    T.K = D.K;
    T.m = qhint >= 0.0 ? qhint : exp((-kPi2 * tt) / 2.0);
    T.q2 = T.m * T.m;
  }
  // values only: 1/(2u) and 1/(a^2 sqrt(u)), u = sv^2 xx + 1, from one rsqrt
  T.sc = ia2;
  if (sv != 0) {
    const double r = rsqrt(((sv * sv) * xx) + 1.0);
    T.cden = (0.5 * r) * r;
    T.sc = T.sc * r;
  }
  T.vvx = (v * v) * xx;
  return T;
}
__device__ inline TNode tnode_setup(double xx, double v, double sv, double a, double err,
                                    double qhint = -1.0, bool has_known = false,
                                    Decision known = Decision{0, 0, 0}) {
  return tnode_setup_r(xx, v, sv, a, 1.0 / (a * a), err, qhint, has_known, known);
}

// f(t|0,1,w) from a prepared t node (pdf.pxi:49-65).
__device__ inline double tnode_ftt(const TNode& T, double w) {
  double p = 0.0;
  const int K = T.K;
  if (T.small) {
    const int lower = (int)(-floor((K - 1) / 2.));
    const int upper = (int)ceil((K - 1) / 2.);
    for (int k = lower; k <= upper; ++k) {
      const double wk = w + (double)(2 * k);
      p = madd(wk, exp_node((wk * wk) * T.m), p);
    }
    p = p * T.rn;
  } else {
    double s1, c1;
    sincospi01(w, s1, c1);
    const double tc = c1 + c1;
    double sk = s1, skm1 = 0.0;          // sin(k pi w), sin((k-1) pi w)
    double e = T.m, r = T.m * T.q2;      // q^(k^2), q^(2k+1)
    if (K >= 1) p = e * s1;
    for (int k = 2; k <= K; ++k) {
      const double sn = msub(tc, sk, skm1);
      skm1 = sk;
      sk = sn;
      e = e * r;
      r = r * T.q2;
      p = madd((double)k * e, sk, p);
    }
    p = p * kPi;
  }
  return p;
}

// tnode_ftt with the large-time sines given (DirectArgs): the same operations.
__device__ inline double tnode_ftt_sc(const TNode& T, double w, double s1, double tc) {
  double p = 0.0;
  const int K = T.K;
  if (T.small) {
    const int lower = (int)(-floor((K - 1) / 2.));
    const int upper = (int)ceil((K - 1) / 2.);
    for (int k = lower; k <= upper; ++k) {
      const double wk = w + (double)(2 * k);
      p = madd(wk, exp_node((wk * wk) * T.m), p);
    }
    p = p * T.rn;
  } else {
    double sk = s1, skm1 = 0.0;
    double e = T.m, r = T.m * T.q2;
    if (K >= 1) p = e * s1;
    for (int k = 2; k <= K; ++k) {
      const double sn = msub(tc, sk, skm1);
      skm1 = sk;
      sk = sn;
      e = e * r;
      r = r * T.q2;
      p = madd((double)k * e, sk, p);
    }
    p = p * kPi;
  }
  return p;
}

// pdf_sv(xx, v, sv, a, w, err) (pdf.pxi:74-102) from a prepared t node.
__device__ inline double tnode_pdf_sv(const TNode& T, double w, double v, double sv, double a) {
  if (!T.pos) return 0.0;
  const double p = tnode_ftt(T, w);
  if (sv == 0) {
    const double ex = exp_node((((-v) * a) * w) - (T.vvx * 0.5));
    return (p * ex) * T.sc;
  }
  if (p < 0) return __builtin_nan("");  // log(p < 0) in the reference
  const double azsv = (a * w) * sv;
  const double c = (((azsv * azsv) - (((2.0 * a) * v) * w)) - T.vvx) * T.cden;
  const double ec = exp_node(c);
  const double r = (p * ec) * T.sc;
  if (__builtin_isinf(ec))  // exp(c) overflow: the literal form
    return (exp(log(p) + (((azsv * azsv) - (((2.0 * a) * v) * w)) - T.vvx) /
                             (((2.0 * (sv * sv)) * T.xx) + 2.0)) /
            sqrt(((sv * sv) * T.xx) + 1.0)) /
           (a * a);
  return r;
}

__device__ inline double pdf_sv(double xx, double v, double sv, double a, double w, double err,
                                int& flags) {
  const TNode T = tnode_setup(xx, v, sv, a, err);
  if (T.amb) flags |= kFlagExact;
  return tnode_pdf_sv(T, w, v, sv, a);
}

}  // namespace wfpt
