// rl_update.hpp — the Q-learning arithmetic of the RL family, stated once: the
// update for the likelihood's scan (rl_kernels.hip) and the closed-loop
// simulator (rl_sim_kernels.hip), device code only, and the learning rate of a
// regressed alpha (rl_reg_kernels.hip), host and device: tests/c/rl_rate_host.cpp
// compiles it with g++.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "wfpt_crlibm.hpp"

#pragma clang fp contract(off)

namespace wfpt {

#if defined(__HIPCC__)
// q + rate * (f - q) as three separately rounded operations (wfpt.pyx:147-153,
// generate.py:503-509): the empty asm keeps the product out of any fused
// multiply-add whatever the contraction setting. A one-ulp difference in q
// could flip the next feedback > q comparison and change every later trial.
__device__ __forceinline__ double rl_q_update(double q, double rate, double f) {
  double prod = rate * (f - q);
  asm volatile("" : "+v"(prod));
  return q + prod;
}
#endif

// The learning rate of the unbounded alpha, 2.718281828459**alpha / (1 +
// 2.718281828459**alpha) (wfpt.pyx:123-125, :317), with the power correctly
// rounded (wfpt_cr::cr_pow_rlbase) and the sum and the quotient each rounded
// once: the same bits on the host and on the device. The reference's libm pow
// is misrounded by one ulp in a small share of calls, so this
// rate can differ from capi::rl_rate's there. A very large alpha gives inf /
// inf = NaN, as in the reference.
WFPT_HD double rl_rate(double alpha) {
  const double e = wfpt_cr::cr_pow_rlbase(alpha);
  const double den = 1.0 + e;
  return e / den;
}

}  // namespace wfpt
