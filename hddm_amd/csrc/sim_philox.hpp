// sim_philox.hpp — the simulators' counter-based random numbers and the walk's
// step threshold, shared by sim_kernels.hip and rl_sim_kernels.hip. Device
// code only. Every value is a function of (seed, row, draw, stream): neither
// the lane nor the launch shape enters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace wfpt {

// Philox4x32-10 (Salmon et al. 2011), counter c, key k.
struct Philox {
  uint32_t w[4];
};
__device__ inline Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                       uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox{{c0, c1, c2, c3}};
}

// A uniform in [0, 1) with 53 random bits from the first two output words.
__device__ inline double philox_uniform(uint64_t seed, uint64_t draw, uint32_t row,
                                        uint32_t stream) {
  const Philox o = philox4x32_10((uint32_t)draw, (uint32_t)(draw >> 32), row, stream,
                                 (uint32_t)seed, (uint32_t)(seed >> 32));
  return ((double)(o.w[0] >> 5) * 67108864.0 + (double)(o.w[1] >> 6)) * (1.0 / 9007199254740992.0);
}

// 53-bit uniform from two Philox words, as philox_uniform forms it.
__device__ inline double drift_uniform(uint32_t hi, uint32_t lo) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) * (1.0 / 9007199254740992.0);
}

// Box-Muller: u1 from words 0 and 1, u2 from words 2 and 3 of one Philox call.
__device__ inline double philox_normal(uint64_t seed, uint64_t draw, uint32_t row,
                                       uint32_t stream) {
  const Philox o = philox4x32_10((uint32_t)draw, (uint32_t)(draw >> 32), row, stream,
                                 (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u1 = drift_uniform(o.w[0], o.w[1]), u2 = drift_uniform(o.w[2], o.w[3]);
  return sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
}

// The step goes up iff (double)w * 2^-32 < prob_up (generate.py:287 with a
// 32-bit uniform). Both sides scaled by 2^32 are exact, and for an integer w,
// w < x iff w < ceil(x): the loop compares integers. prob_up <= 0 or NaN never
// goes up, prob_up >= 1 always does.
__device__ inline uint64_t drift_threshold(double prob_up) {
  if (!(prob_up > 0.0)) return 0;
  if (prob_up >= 1.0) return (uint64_t)1 << 32;
  return (uint64_t)ceil(prob_up * 4294967296.0);
}

}  // namespace wfpt
