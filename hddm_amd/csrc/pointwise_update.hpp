// pointwise_update.hpp — the per-trial accumulator of the model-comparison
// pass, stated once for the device kernels
// (pointwise_kernels.hip) and for a host build (tests/c/pointwise_host.cpp).
//
// One state per trial, fed one log term per kept sweep, in rising sweep order:
// a streaming log-sum-exp {m, r} (lppd), Welford's {mean, M2} (the WAIC
// penalty) and two counts. The rule below is the contract: every operation is
// rounded once, exp and log are the correctly rounded ones of wfpt_crlibm.hpp,
// and no product is fused into an FMA, so the device result equals a g++ build
// of this header bit for bit.
#pragma once
#include <stdint.h>

#include "wfpt_crlibm.hpp"

#pragma clang fp contract(off)

namespace wfpt_pw {

struct State {
  double m;       // running maximum of the finite terms
  double r;       // sum of exp(term - m)
  double mean;    // Welford's running mean ...
  double M2;      // ... and sum of squared deviations
  int32_t k;      // finite (or NaN) terms seen
  int32_t n_inf;  // terms equal to -inf (zero densities)
};

// The empty asm keeps a product out of any fused multiply-add on the device
// whatever the contraction setting (rl_update.hpp); a host build is compiled
// with contraction off.
WFPT_HD double keep_product(double p) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(p));
#endif
  return p;
}

// A NaN term needs no case of its own: it fails both comparisons, takes the
// last branch and leaves r, mean and M2 NaN for good.
WFPT_HD void update(State& s, double l) {
  if (l == -INFINITY) {
    s.n_inf += 1;
    return;
  }
  s.k += 1;
  if (s.k == 1) {
    s.m = l;
    s.r = 1.0;
  } else if (l <= s.m) {
    s.r = s.r + wfpt_cr::cr_exp(l - s.m);
  } else {
    s.r = keep_product(s.r * wfpt_cr::cr_exp(s.m - l)) + 1.0;
    s.m = l;
  }
  const double d = l - s.mean;
  s.mean = s.mean + d / (double)s.k;
  s.M2 = s.M2 + keep_product(d * (l - s.mean));
}

struct Result {
  double lppd, p_waic, mean;
};

// S counts every sweep, the -inf ones too: a zero density is a term exp(-inf)
// = 0 of the mean density.
WFPT_HD Result finish(const State& s, int64_t S) {
  Result R;
  if (s.k == 0) {
    R.lppd = -INFINITY;
    R.mean = -INFINITY;
    R.p_waic = __builtin_nan("");
    return R;
  }
  R.lppd = s.m + wfpt_cr::cr_log(s.r) - wfpt_cr::cr_log((double)S);
  R.p_waic = s.k >= 2 ? s.M2 / (double)(s.k - 1) : 0.0;
  R.mean = s.mean;
  return R;
}

}  // namespace wfpt_pw
