// reg_predict.hpp — one regression term's predicted parameter of one trial,
// link(design row . coefficients), shared by reg_fill_kernel (reg_kernels.hip)
// and reg_sim_kernel (reg_sim_kernels.hip) so that the likelihood and the
// posterior predictive form the same bits. Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reg_internal.h"
#include "wfpt_crlibm.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// x: the trial's element of design column 0 (column c is x[c * n]); b: the
// trial's coefficient row. The order of the predictor is part of the contract
// (reg_internal.h): one product, one sum per column, left to right. The empty
// asm keeps each product out of a fused multiply-add whatever the contraction
// setting, as rl_scan_kernel guards its update.
__device__ inline double reg_predict(const RegTerm& T, const double* x, int64_t n,
                                     const double* b) {
  const double* col = x + (int64_t)T.col0 * n;
  double eta = col[0] * b[T.col0];
  asm volatile("" : "+v"(eta));
  for (int c = 1; c < T.ncol; ++c) {
    double prod = col[(int64_t)c * n] * b[T.col0 + c];
    asm volatile("" : "+v"(prod));
    eta = eta + prod;
  }
  double y = eta;
  if (T.link == kRegExp) {
    y = wfpt_cr::cr_exp(eta);
  } else if (T.link == kRegInvLogit) {
    const double e = wfpt_cr::cr_exp(-eta);
    const double den = 1.0 + e;
    y = 1.0 / den;
  }
  return y;
}

}  // namespace wfpt
