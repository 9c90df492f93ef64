// wfpt_types.hpp — what the host and the device share by value: a call's
// parameters and knobs, the integration families, the trial flags and
// outcomes, the routing constants of the exact path and the depth of the
// in-wave trees. Host + device, no device-only code.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace wfpt {

constexpr double kPi = 3.14159265358979323846;  // M_PI
constexpr double kPi2 = kPi * kPi;             // M_PI**2 (pdf.pxi:37, 62)

struct Params {
  double v, sv, a, z, sz, t, st, p_outlier;
};
struct Knobs {
  double err;
  int n_st, n_sz, use_adaptive;
  double simps_err, w_outlier;
};

enum Mode : int {
  kDirect = 0,   // sz = st = 0: one pdf_sv (pdf.pxi:129)
  kAdaptT = 1,   // st only, adaptive (pdf.pxi:132)
  kAdaptZ = 2,   // sz only, adaptive (pdf.pxi:139)
  kAdaptTZ = 3,  // sz and st, adaptive 2-D (pdf.pxi:144)
  kFixedT = 4,   // fixed Simpson variants (pdf.pxi:134, 141, 146)
  kFixedZ = 5,
  kFixedTZ = 6,
  kRuntime = 7,  // per-trial parameters: mode decided per lane
};

// Host+device: mode after full_pdf's st/sz < 1e-3 zeroing (pdf.pxi:122-146).
// A NaN is not below the threshold: the reference leaves it and integrates
// over a NaN interval (NaN), as trial_setup does, so its family integrates.
__host__ __device__ inline int select_mode(double sz, double st, int use_adaptive) {
  const bool zst = st < 1e-3, zsz = sz < 1e-3;
  if (zsz) {
    if (zst) return kDirect;
    return use_adaptive > 0 ? kAdaptT : kFixedT;
  }
  if (zst) return use_adaptive ? kAdaptZ : kFixedZ;
  return use_adaptive ? kAdaptTZ : kFixedTZ;
}

// ---------------------------------------------------------------------------
// Routing of trials whose value hinges on last-bit rounding (wfpt_exact.hpp).
//
// kExactBelow: a trial density below it (or zero, negative, NaN) is recomputed
// on the exact path: there intermediate values can be subnormal, where one
// rounding is up to 1e-5 relative, and a zero / negative / NaN outcome is a
// decision, not a rounding.
// kTieBand: an adaptive stop test |S2 - S| <= 15 err decided within this
// relative band of its threshold sends the trial to the exact path (the fast
// path's node values carry ~1e-14 relative error; the band is 1000x wider).
constexpr double kExactBelow = 1e-290;
constexpr double kTieBand = 1e-11;

// A settled density 0 < p <= kExactBelow (its tree decided with the
// reference's operations, no near-tie flagged) when the call's outlier mixture
// adds w_outlier p_outlier >= kMixAbsorb: any value within the fast path's
// error of p (< 1e-289) satisfies p' (1 - p_outlier) < w_outlier p_outlier
// 2^-54, so the reference's mixture p' (1 - p_outlier) + w_outlier p_outlier
// (wfpt.pyx:44, :70) rounds to w_outlier p_outlier exactly and the trial's
// output does not depend on p: it is settled as 0 (the same mixture bits)
// instead of being recomputed on the exact path. Without the mixture
// (full_pdf, p_outlier = 0) such a density still takes the exact path.
constexpr double kMixAbsorb = 1e-250;
__host__ __device__ inline bool tiny_absorbed(double p, double p_outlier, double w_outlier) {
  return p > 0.0 && p <= kExactBelow && w_outlier * p_outlier >= kMixAbsorb;
}

enum Flag : int {
  kFlagDepth = 1,     // refinement deeper than the stack (WFPT_MAX_DEPTH)
  kFlagBudget = 2,    // more than kEvalBudget pdf_sv evaluations in one trial
  kFlagExact = 4,     // recompute on the exact path
  kFlagFallback = 8,  // tree deeper than the breadth-first levels: per-lane walk
};
constexpr int kFlagErrors = kFlagDepth | kFlagBudget;

// ---------------------------------------------------------------------------
// Adaptive trees (the reference's adaptiveSimpsonsAux recursion) over the
// dyadic points of the root interval.
//
// Node order used below: lb, d, c, e, ub of an interval (integrate.pxi:114-141
// prologue nodes lb, c, ub + the root aux nodes d, e). The level-0 engine
// (wfpt_engine.hip: engine_kernel) completes trees of up to kTreeDepth
// refinement levels per axis in-wave (HDDM's n_st = n_sz = 2 default); deeper
// trees continue on the per-lane walk (kFlagFallback). A tree's values live at
// the kTreePoints dyadic points P_0..P_kTreeW of its root interval.
constexpr int kTreeDepth = 2;
constexpr int kTreeW = 4 << kTreeDepth;
constexpr int kTreePoints = kTreeW + 1;

enum Outcome : int { kFinal = 0, kTree = 1, kExact = 2 };

}  // namespace wfpt
