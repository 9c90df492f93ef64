// pointwise_internal.h — launcher interface between the C ABI (capi_*.cpp) and
// the model-comparison pass (pointwise_kernels.hip). Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wfpt {

// The per-trial accumulator state of wfpt_pw::State (pointwise_update.hpp), one
// array per field, `len` entries each. All zero bytes is the empty state.
struct PointwiseState {
  double* m;
  double* r;
  double* mean;
  double* M2;
  int32_t* k;
  int32_t* n_inf;
};

// T sweeps of per-trial log terms, sweep t's trial i at lp[t * len + i], into
// the state: one lane per trial, the sweeps in rising t.
void launch_pointwise_accumulate(const double* lp, int64_t T, int64_t len, const PointwiseState& st,
                                 hipStream_t s);
// out[0 * len + i] = lppd, [1 * len + i] = p_waic, [2 * len + i] = mean and
// [3 * len + i] = n_inf (as a double) of trial i after S sweeps.
void launch_pointwise_finish(const PointwiseState& st, int64_t len, int64_t S, double* out,
                             hipStream_t s);

}  // namespace wfpt
