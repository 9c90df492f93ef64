// Host build of the learning rate of a regressed alpha
// (hddm_amd/csrc/rl_update.hpp over wfpt_crlibm.hpp's cr_pow_rlbase) for
// tests/test_rl_rate.py and tests/test_rl_reg.py, with the libm route the
// non-regressed paths keep (capi_rl.cpp: rl_rate) next to it.
#include <math.h>
#include <stdint.h>
#include "../../hddm_amd/csrc/rl_update.hpp"
extern "C" void cr_pow_rlbase_array(const double* x, int64_t n, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = wfpt_cr::cr_pow_rlbase(x[i]);
}
extern "C" void rl_rate_array(const double* x, int64_t n, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = wfpt::rl_rate(x[i]);
}
extern "C" void libm_pow_rlbase_array(const double* x, int64_t n, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = pow(2.718281828459, x[i]);
}
extern "C" void libm_rl_rate_array(const double* x, int64_t n, double* out) {
  for (int64_t i = 0; i < n; ++i) {
    const double e = pow(2.718281828459, x[i]);
    out[i] = e / (1 + e);
  }
}
