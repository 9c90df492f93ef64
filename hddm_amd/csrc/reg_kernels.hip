// reg_kernels.hip — the regression front end on gfx950 (HDDMRegressor's
// wiener_multi_like, hddm/models/hddm_regression.py:26-36: trial-wise
// parameters link(design matrix . coefficients) into wfpt.wiener_like_multi).
//
//   reg_fill_kernel   one trial per lane: every regression term's linear
//                     predictor and link, and the group rows of the
//                     non-regressed parameters, into per-trial arrays
//
// The densities are not computed here: the arrays go into the per-trial-
// parameter pass (multi_fast_kernel / multi_kernel through
// launch_multi_fast / launch_multi), the per-group sums come from
// rl_kernels.hip's launch_rl_node_sum.
#include <hip/hip_runtime.h>

#include "reg_internal.h"
#include "reg_predict.hpp"
#include "wfpt_types.hpp"

#pragma clang fp contract(off)

namespace wfpt {
namespace {

constexpr int kRegBlock = 256;

// The predictor (its order is part of the contract, reg_internal.h) is
// reg_predict.hpp's, shared with the posterior predictive's kernel. A column
// is contiguous over trials, so a wave reads 512 consecutive bytes per column;
// the coefficient row is the same address for every lane of a group.
__global__ __launch_bounds__(kRegBlock) void reg_fill_kernel(RegFill F) {
  const int64_t i = (int64_t)blockIdx.x * kRegBlock + threadIdx.x;
  if (i >= F.n) return;
  const int32_t g = F.group ? F.group[i] : 0;
  const double* b = F.coef + (int64_t)g * F.C;
  const int64_t ci = F.pred_in ? (F.caller ? F.caller[i] : i) : 0;
#pragma unroll 1
  for (int k = 0; k < F.n_terms; ++k) {
    const double y = reg_predict(F.term[k], F.X + i, F.n, b);
    F.arr[(int64_t)k * F.n + i] = y;
    if (F.pred_in) F.pred_in[(int64_t)k * F.n + ci] = y;
  }
  if (F.expand) {
    const double* row = reinterpret_cast<const double*>(F.P + g);
    int slot = F.n_terms;
#pragma unroll
    for (int f = 0; f < 7; ++f) {
      if (F.expand & (1 << f)) {
        F.arr[(int64_t)slot * F.n + i] = row[f];
        ++slot;
      }
    }
  }
}

}  // namespace

void launch_reg_fill(const RegFill& F, hipStream_t s) {
  const int64_t nb = (F.n + kRegBlock - 1) / kRegBlock;
  if (nb == 0 || (F.n_terms == 0 && F.expand == 0)) return;
  hipLaunchKernelGGL(reg_fill_kernel, dim3(nb), dim3(kRegBlock), 0, s, F);
}

}  // namespace wfpt
