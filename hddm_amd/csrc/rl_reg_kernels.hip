// rl_reg_kernels.hip — the RL regression front end on gfx950 (HDDMrlRegressor's
// wienerRL_multi_like, hddm/models/hddm_rl_regression.py:25-38: trial-wise
// parameters link(design matrix . coefficients), alpha among them, into
// wfpt.wiener_like_multi_rlddm, src/wfpt.pyx:277-320).
//
//   rl_reg_fill_kernel  one trial per lane: every regression term's linear
//                       predictor and link, the learning rate of a regressed
//                       alpha, and the group rows of the non-regressed
//                       parameters, into per-trial arrays
//
// The learning rate is formed here, spread over n lanes, and not in the Q
// recurrence: the scan (rl_kernels.hip: rl_scan_kernel) is one lane per
// segment and latency-bound, and a double-double power per step would
// multiply its length. The scan reads vmul / rate, writes the drifts into the
// v slot, and the densities come from the per-trial-parameter pass.
#include <hip/hip_runtime.h>

#include "reg_predict.hpp"
#include "rl_reg_internal.h"
#include "rl_update.hpp"
#include "wfpt_types.hpp"

#pragma clang fp contract(off)

namespace wfpt {
namespace {

constexpr int kRlRegBlock = 256;

__global__ __launch_bounds__(kRlRegBlock) void rl_reg_fill_kernel(RlRegFill F) {
  const int64_t i = (int64_t)blockIdx.x * kRlRegBlock + threadIdx.x;
  if (i >= F.n) return;
  const int32_t g = F.group ? F.group[i] : 0;
  const double* b = F.coef + (int64_t)g * F.C;
  const int64_t ci = F.caller ? F.caller[i] : i;
#pragma unroll 1
  for (int k = 0; k < F.n_terms; ++k) {
    const RegTerm T = F.term[k];
    const double y = reg_predict(T, F.X + i, F.n, b);
    if (F.pred_in) F.pred_in[(int64_t)k * F.n + ci] = y;
    if (T.param == kRlRegAlpha) {
      const double r = rl_rate(y);
      F.rate[i] = r;
      if (F.rate_in) F.rate_in[ci] = r;
    } else if (T.param == 0) {
      F.vmul[i] = y;
    } else {
      F.arr[(int64_t)T.param * F.n + i] = y;
    }
  }
  const double* row = reinterpret_cast<const double*>(F.P + g);
#pragma unroll
  for (int f = 1; f < 7; ++f)
    if (F.expand & (1 << f)) F.arr[(int64_t)f * F.n + i] = row[f];
}

}  // namespace

void launch_rl_reg_fill(const RlRegFill& F, hipStream_t s) {
  const int64_t nb = (F.n + kRlRegBlock - 1) / kRlRegBlock;
  if (nb == 0 || (F.n_terms == 0 && F.expand == 0)) return;
  hipLaunchKernelGGL(rl_reg_fill_kernel, dim3(nb), dim3(kRlRegBlock), 0, s, F);
}

}  // namespace wfpt
