// wfpt_quad.hpp — the per-lane quadrature and the trial-level entry points of
// the device density (src/integrate.pxi:12-206, full_pdf of src/pdf.pxi:
// 104-146): the reference's adaptive Simpson as an iterative walk with an
// explicit stack, the fixed Simpson variants, a trial's prologue, the exact
// path and the settlement of a trial density. Every stop test is the
// reference's, so the quadrature tree is identical; one decided within
// kTieBand of its threshold, and a density that hinges on subnormal rounding,
// send the trial to the exact path (wfpt_exact.hpp). Trees deeper than the
// in-wave levels (kTreeDepth) continue here (adaptive_walk).
// Device code. Compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/wfpt_amd.h"
#include "wfpt_exact.hpp"
#include "wfpt_series.hpp"
#include "wfpt_types.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// ---------------------------------------------------------------------------
// The reference's stop test of adaptiveSimpsonsAux (integrate.pxi:105 / 170):
// true = refine. Marks kFlagExact when the test is decided inside kTieBand.
__host__ __device__ inline bool simpson_refine(double S, double S2, double err, int bottom,
                                               int& flags) {
  if (bottom <= 0) return false;
  const double d = fabs(S2 - S), thr = 15 * err;
  if (fabs(d - thr) <= kTieBand * ((fabs(S) + fabs(S2)) + thr)) flags |= kFlagExact;
  return !(d <= thr);
}

// ---------------------------------------------------------------------------
// Adaptive Simpson (integrate.pxi:72-141, 143-206) as an iterative walk.
struct Frame {
  double lb, ub, S, fb, fe, fm, err, left, hs;
};

// Tie resolution inside a per-lane walk. A stop test decided within kTieBand
// is re-decided from the interval's 5 points evaluated on the exact path
// (literal expressions, glibc-equal libm): the reference's own S and S2, so
// only that decision pays exact evaluations (deep trees run ~1e5 tests per
// trial, where whole-trial exact recomputation would dominate). NoResolve
// instead abandons the trial (kFlagExact: the caller recomputes it exactly).
struct NoResolve {
  static constexpr bool kResolves = false;
  __device__ bool operator()(double, double, double, bool, double, int) const { return false; }
};
template <class GX>
struct XResolve {
  static constexpr bool kResolves = true;
  GX gx;  // exact f(u), the reference's integrand value (divided by its width)
  // [lb, ub]: the interval; its S came from (hs / 6) (root prologue) or
  // (hs / 12) (a parent's Sleft / Sright, hs = the parent's width), each over
  // (f(lb) + 4 f(c)) + f(ub) (integrate.pxi:133-134, 105-107).
  __device__ bool operator()(double lb, double ub, double hs, bool root, double err,
                             int bottom) const {
    const double c = (ub + lb) / 2.;
    const double d = (lb + c) / 2., e = (c + ub) / 2.;
    const double fb = gx(lb), fd = gx(d), fm = gx(c), fe = gx(e), fu = gx(ub);
    const double S = root ? (hs / 6) * ((fb + (4 * fm)) + fu) : (hs / 12) * ((fb + (4 * fm)) + fu);
    const double h = ub - lb;
    const double S2 = ((h / 12) * ((fb + (4 * fd)) + fm)) + ((h / 12) * ((fm + (4 * fe)) + fu));
    return !(bottom <= 0 || fabs(S2 - S) <= 15 * err);
  }
};
template <class GX>
__device__ inline XResolve<GX> make_xresolve(GX gx) {
  return XResolve<GX>{gx};
}

// Depth <= N frames held in registers: every access is a compile-time index
// after unrolling, so the array is scalarised (no scratch).
template <int N>
struct RegStack {
  static constexpr int kCap = N;
  Frame f[N];
  __device__ inline Frame get(int i) const {
    Frame r = f[0];
#pragma unroll
    for (int k = 1; k < N; ++k)
      if (i == k) r = f[k];
    return r;
  }
  __device__ inline double left(int i) const {
    double r = f[0].left;
#pragma unroll
    for (int k = 1; k < N; ++k)
      if (i == k) r = f[k].left;
    return r;
  }
  __device__ inline void set(int i, const Frame& x) {
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (i == k) f[k] = x;
  }
  __device__ inline void set_left(int i, double v) {
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (i == k) f[k].left = v;
  }
};

// Arbitrary depth (up to N): plain private array (scratch memory).
template <int N>
struct MemStack {
  static constexpr int kCap = N;
  Frame f[N];
  __device__ inline Frame get(int i) const { return f[i]; }
  __device__ inline double left(int i) const { return f[i].left; }
  __device__ inline void set(int i, const Frame& x) { f[i] = x; }
  __device__ inline void set_left(int i, double v) { f[i].left = v; }
};

constexpr long long kEvalBudget = 1ll << 24;

// Integrates g over [lb0, ub0] exactly like adaptiveSimpsons_1D/_2D followed by
// adaptiveSimpsonsAux(_2D): g(c) must already include the division by ZT (or
// st). Every lane walks its own tree; each loop trip evaluates g at the 3
// prologue nodes or the 2 new nodes of one interval from ONE call site. A
// near-tie stop test is re-decided by `resolve` (XResolve) or abandons the
// trial (NoResolve); depth past the stack or the evaluation budget abandon it
// too (flags set, NaN returned): no input keeps a wave busy without bound.
template <class Stack, class G, class R = NoResolve>
__device__ inline double adaptive_walk(G&& g, double lb0, double ub0, double err0, int depth,
                                       int& flags, const long long& ne, const R& resolve = R()) {
  Stack stk;
  double lb = lb0, ub = ub0, err = err0;
  double S = 0.0, fb = 0.0, fe = 0.0, fm = 0.0;
  double hs = 0.0;    // width the current S was computed with
  bool sroot = true;  // S from the prologue (hs / 6) rather than a parent (hs / 12)
  bool init = true;
  int bottom = depth, sp = 0;
  unsigned right_mask = 0u;  // bit i: frame i has finished its left child
  double result = 0.0;
  for (;;) {
    const double c = (ub + lb) / 2.;
    const double p0 = init ? lb : (lb + c) / 2.;
    const double p1 = init ? ub : (c + ub) / 2.;
    const int n = init ? 3 : 2;
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
      const double p = (i == 0) ? p0 : ((i == 1) ? p1 : c);
      const double y = g(p);
      if (i == 0) y0 = y;
      else if (i == 1) y1 = y;
      else y2 = y;
    }
    if (ne > kEvalBudget) flags |= kFlagBudget;
    if (flags & (kFlagErrors | kFlagExact)) {
      result = __builtin_nan("");
      break;
    }
    const double h = ub - lb;
    if (init) {  // adaptiveSimpsons_1D / _2D prologue
      fb = y0;
      fe = y1;
      fm = y2;
      S = (h / 6) * ((fb + (4 * fm)) + fe);
      hs = h;
      sroot = true;
      init = false;
      continue;
    }
    // adaptiveSimpsonsAux body (integrate.pxi:105-112 / 170-178)
    const double fd = y0, fee = y1;
    const double Sl = (h / 12) * ((fb + (4 * fd)) + fm);
    const double Sr = (h / 12) * ((fm + (4 * fee)) + fe);
    const double S2 = Sl + Sr;
    bool refine = simpson_refine(S, S2, err, bottom, flags);
    if (flags & kFlagExact) {
      if (!R::kResolves) {
        result = __builtin_nan("");
        break;
      }
      flags &= ~kFlagExact;
      refine = resolve(lb, ub, hs, sroot, err, bottom);
    }
    if (refine && sp >= Stack::kCap) {
      flags |= kFlagDepth;
      result = __builtin_nan("");
      break;
    }
    if (refine) {
      Frame fr;
      fr.lb = c;
      fr.ub = ub;
      fr.S = Sr;
      fr.fb = fm;
      fr.fe = fe;
      fr.fm = fee;
      fr.err = err / 2;
      fr.left = 0.0;
      fr.hs = h;
      stk.set(sp, fr);
      ++sp;
      ub = c;
      err = err / 2;
      S = Sl;
      hs = h;
      sroot = false;
      fe = fm;
      fm = fd;
      bottom -= 1;
      continue;
    }
    double val = S2 + (S2 - S) / 15;
    bool done = false;
    for (;;) {  // return up the tree: left + right in reference order
      if (sp == 0) {
        result = val;
        done = true;
        break;
      }
      const int top = sp - 1;
      if (!((right_mask >> top) & 1u)) {
        const Frame fr = stk.get(top);
        stk.set_left(top, val);
        right_mask |= (1u << top);
        lb = fr.lb;
        ub = fr.ub;
        S = fr.S;
        fb = fr.fb;
        fe = fr.fe;
        fm = fr.fm;
        err = fr.err;
        hs = fr.hs;
        sroot = false;
        bottom = depth - sp;
        break;
      }
      val = stk.left(top) + val;
      right_mask &= ~(1u << top);
      --sp;
    }
    if (done) break;
  }
  return result;
}

// Fixed composite Simpson, integrate.pxi:12-45. Returns the integral; the
// reference leaves `y` uninitialised when n == 0 (0 here).
__device__ inline double simpson_1d(double x, double v, double sv, double a, double z, double t,
                                    double err, double lb_z, double ub_z, int n_sz, double lb_t,
                                    double ub_t, int n_st, long long& ne, int& flags) {
  double ht, hz;
  const int n = (n_st < n_sz) ? n_sz : n_st;
  if (n_st == 0) {
    hz = (ub_z - lb_z) / n;
    ht = 0;
    lb_t = t;
    ub_t = t;
  } else {
    hz = 0;
    ht = (ub_t - lb_t) / n;
    lb_z = z;
    ub_z = z;
  }
  ++ne;
  double S = pdf_sv(x - lb_t, v, sv, a, lb_z, err, flags);
  double y = 0.0;
  for (int i = 1; i <= n; ++i) {
    const double z_tag = lb_z + hz * i;
    const double t_tag = lb_t + ht * i;
    ++ne;
    y = pdf_sv(x - t_tag, v, sv, a, z_tag, err, flags);
    if (i & 1) S += (4 * y);
    else S += (2 * y);
  }
  S = S - y;
  S = S / ((ub_t - lb_t) + (ub_z - lb_z));
  return ((ht + hz) * S) / 3;
}

__device__ inline double simpson_2d(double x, double v, double sv, double a, double z, double t,
                                    double err, double lb_z, double ub_z, int n_sz, double lb_t,
                                    double ub_t, int n_st, long long& ne, int& flags) {
  const double ht = (ub_t - lb_t) / n_st;
  double S = simpson_1d(x, v, sv, a, z, lb_t, err, lb_z, ub_z, n_sz, 0, 0, 0, ne, flags);
  double y = 0.0;
  for (int i_t = 1; i_t <= n_st; ++i_t) {
    const double t_tag = lb_t + ht * i_t;
    y = simpson_1d(x, v, sv, a, z, t_tag, err, lb_z, ub_z, n_sz, 0, 0, 0, ne, flags);
    if (i_t & 1) S += (4 * y);
    else S += (2 * y);
  }
  S = S - y;
  S = S / (ub_t - lb_t);
  return (ht * S) / 3;
}

// full_pdf's prologue (pdf.pxi:111-125): validity, boundary flip, |x|, the
// st / sz < 1e-3 zeroing. valid == 0: density 0 (pdf.pxi:111-113).
struct Trial {
  double x, v, z, sz, st;
  int valid;
};

__device__ inline Trial trial_setup(double x, const Params& P) {
  Trial T;
  double v = P.v, z = P.z, st = P.st, sz = P.sz;
  const double a = P.a, sv = P.sv, t = P.t;
  T.valid = !((z < 0) || (z > 1) || (a < 0) || (t < 0) || (st < 0) || (sv < 0) || (sz < 0) ||
              (sz > 1) || ((fabs(x) - (t - st / 2.)) < 0) || (z + sz / 2. > 1) ||
              (z - sz / 2. < 0) || (t - st / 2. < 0));
  if (x > 0) {
    v = -v;
    z = 1. - z;
  }
  T.x = fabs(x);
  if (st < 1e-3) st = 0;
  if (sz < 1e-3) sz = 0;
  T.v = v;
  T.z = z;
  T.st = st;
  T.sz = sz;
  return T;
}

// trial_setup for a trial whose boundary is known to the caller (flip ==
// (x > 0)): the same values, but v and z come from `flip` alone, so inside a
// pass over one boundary (flip wave-uniform) they are wave-uniform too.
__device__ inline Trial trial_setup_b(double x, const Params& P, bool flip) {
  Trial T;
  const double a = P.a, sv = P.sv, t = P.t, st0 = P.st, sz0 = P.sz;
  T.valid = !((P.z < 0) || (P.z > 1) || (a < 0) || (t < 0) || (st0 < 0) || (sv < 0) ||
              (sz0 < 0) || (sz0 > 1) || ((fabs(x) - (t - st0 / 2.)) < 0) ||
              (P.z + sz0 / 2. > 1) || (P.z - sz0 / 2. < 0) || (t - st0 / 2. < 0));
  T.v = flip ? -P.v : P.v;
  T.z = flip ? 1. - P.z : P.z;
  T.x = fabs(x);
  T.st = (st0 < 1e-3) ? 0.0 : st0;
  T.sz = (sz0 < 1e-3) ? 0.0 : sz0;
  return T;
}

// full_pdf (pdf.pxi:104-146) for one trial: the general per-lane walk (the
// fallback for trees deeper than the breadth-first levels, fixed Simpson,
// per-trial parameters). MODE is the integration family (kRuntime: per lane).
template <int MODE, class Stack>
__device__ inline double full_pdf(double x0, const Params& P, const Knobs& K, long long& ne,
                                  int& flags) {
  const Trial tr = trial_setup(x0, P);
  if (!tr.valid) return 0.0;
  const double a = P.a, sv = P.sv, t = P.t;
  const double x = tr.x, v = tr.v, z = tr.z, st = tr.st, sz = tr.sz;
  const int mode = (MODE == kRuntime) ? select_mode(sz, st, K.use_adaptive) : MODE;
  const double err = K.err;

  if (mode == kDirect) {
    ++ne;
    return pdf_sv(x - t, v, sv, a, z, err, flags);
  }
  if (mode == kAdaptZ) {
    // adaptiveSimpsons_1D over z at fixed t: one t node for every evaluation
    const double lb_z = z - sz / 2., ub_z = z + sz / 2.;
    const double iZT = 1.0 / (ub_z - lb_z);
    const TNode T = tnode_setup(x - t, v, sv, a, err);
    if (T.amb) flags |= kFlagExact;
    auto g = [&](double zc) -> double {
      ++ne;
      return tnode_pdf_sv(T, zc, v, sv, a) * iZT;
    };
    const double ZT = ub_z - lb_z;
    auto rz = make_xresolve([=](double zc) { return wfpt_x::pdf_sv(x - t, v, sv, a, zc, err) / ZT; });
    return adaptive_walk<Stack>(g, lb_z, ub_z, K.simps_err, K.n_sz, flags, ne, rz);
  }
  if (mode == kAdaptT) {
    const double lb_t = t - st / 2., ub_t = t + st / 2.;
    const double iZT = 1.0 / (ub_t - lb_t);
    auto g = [&](double tc) -> double {
      ++ne;
      return pdf_sv(x - tc, v, sv, a, z, err, flags) * iZT;
    };
    const double ZT = ub_t - lb_t;
    auto rt = make_xresolve([=](double tc) { return wfpt_x::pdf_sv(x - tc, v, sv, a, z, err) / ZT; });
    return adaptive_walk<Stack>(g, lb_t, ub_t, K.simps_err, K.n_st, flags, ne, rt);
  }
  if (mode == kAdaptTZ) {
    const double lb_z = z - sz / 2., ub_z = z + sz / 2.;
    const double lb_t = t - st / 2., ub_t = t + st / 2.;
    const double iZT = 1.0 / (ub_z - lb_z), istw = 1.0 / (ub_t - lb_t);
    const double ZT = ub_z - lb_z, stw = ub_t - lb_t;
    const double se = K.simps_err;
    const int nsz = K.n_sz;
    auto outer = [&](double tc) -> double {
      const TNode T = tnode_setup(x - tc, v, sv, a, err);
      if (T.amb) flags |= kFlagExact;
      auto inner = [&](double zc) -> double {
        ++ne;
        return tnode_pdf_sv(T, zc, v, sv, a) * iZT;
      };
      auto rz = make_xresolve([=](double zc) { return wfpt_x::pdf_sv(x - tc, v, sv, a, zc, err) / ZT; });
      return adaptive_walk<Stack>(inner, lb_z, ub_z, se, nsz, flags, ne, rz) * istw;
    };
    // exact outer values: the reference's z integral at tc (its own walk)
    auto rt = make_xresolve([=](double tc) {
      wfpt_x::Ctx C;
      auto inner_x = [&](double zc) { return wfpt_x::pdf_sv(x - tc, v, sv, a, zc, err) / ZT; };
      return wfpt_x::adaptive(inner_x, lb_z, ub_z, se, nsz, C) / stw;
    });
    return adaptive_walk<Stack>(outer, lb_t, ub_t, K.simps_err, K.n_st, flags, ne, rt);
  }
  if (mode == kFixedT)
    return simpson_1d(x, v, sv, a, z, t, err, z, z, 0, t - st / 2., t + st / 2., K.n_st, ne,
                      flags);
  if (mode == kFixedZ)
    return simpson_1d(x, v, sv, a, z, t, err, z - sz / 2., z + sz / 2., K.n_sz, t, t, 0, ne,
                      flags);
  return simpson_2d(x, v, sv, a, z, t, err, z - sz / 2., z + sz / 2., K.n_sz, t - st / 2.,
                    t + st / 2., K.n_st, ne, flags);
}

// The exact path for one trial (wfpt_exact.hpp), out of line: the kernels call
// it only for the rare trials routed there, and it must not add to their
// register allocation. Returns the density; flags gets kFlagDepth/Budget.
__device__ __noinline__ double exact_pdf(double x, Params P, Knobs K, long long* ne, int* flags) {
  wfpt_x::Ctx C;
  const double p = wfpt_x::full_pdf(x, P.v, P.sv, P.a, P.z, P.sz, P.t, P.st, K.err, K.n_st,
                                    K.n_sz, K.use_adaptive, K.simps_err, C);
  *ne += C.ne;
  *flags |= C.ovf;
  return p;
}

// The general per-lane walk, out of line (trees deeper than the breadth-first
// levels); a near-tie on it goes to the exact path.
template <int MODE>
__device__ __noinline__ double fallback_pdf(double x, Params P, Knobs K, long long* ne,
                                            int* flags) {
  long long n = 0;
  int f = 0;
  double p = full_pdf<MODE, MemStack<WFPT_MAX_DEPTH>>(x, P, K, n, f);
  if (f & kFlagExact) {
    n = 0;
    f = 0;
    p = exact_pdf(x, P, K, &n, &f);
  }
  *ne += n;
  *flags |= f;
  return p;
}

// Settles a trial density: a value that hinges on last-bit rounding (zero,
// negative, NaN, below kExactBelow, or kFlagExact raised on the way: a
// near-tie or an ambiguous series decision) is recomputed on the exact path,
// unless it is a structural zero (invalid parameters, or no evaluation point
// with x - t_node > 0: no arithmetic produced it).
__device__ inline double settle(double p, double x, const Params& P, const Knobs& K, bool structural,
                                long long& ne, int& flags) {
  if (!(flags & kFlagExact) && (p > kExactBelow || structural)) return p;
  flags &= ~kFlagExact;
  long long n = 0;
  const double q = exact_pdf(x, P, K, &n, &flags);
  ne = n;
  return q;
}

// P(hit upper boundary), pdf.pxi:67-72
__device__ inline double prob_ub(double v, double a, double z) {
  if (v == 0) return z;
  return (exp(((-2.0 * a) * z) * v) - 1.0) / (exp((-2.0 * a) * v) - 1.0);
}

}  // namespace wfpt
