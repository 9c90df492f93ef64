// rl_update.hpp — the Q-learning update of the RL family, stated once for the
// likelihood's scan (rl_kernels.hip) and the closed-loop simulator
// (rl_sim_kernels.hip). Device code only.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace wfpt {

// q + rate * (f - q) as three separately rounded operations (wfpt.pyx:147-153,
// generate.py:503-509): the empty asm keeps the product out of any fused
// multiply-add whatever the contraction setting. A one-ulp difference in q
// could flip the next feedback > q comparison and change every later trial.
__device__ __forceinline__ double rl_q_update(double q, double rate, double f) {
  double prod = rate * (f - q);
  asm volatile("" : "+v"(prod));
  return q + prod;
}

}  // namespace wfpt
