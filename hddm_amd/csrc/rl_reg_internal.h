// rl_reg_internal.h — launcher interface between the C ABI (capi_rl_reg.cpp)
// and the RL regression front end (rl_reg_kernels.hip). Not part of the public
// ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reg_internal.h"

namespace wfpt {

constexpr int kRlRegAlpha = 7;     // wfpt_reg_term.param of the learning rate's alpha
constexpr int kRlRegMaxTerms = 8;  // one term per parameter (v .. st, alpha) at the most

// One fill launch of the RL regression likelihood. Trials are
// in stored order (group-major). Field f (0..6 = v .. st, wfpt_params order)
// of a trial goes to arr[f * n + i]: a regressed field from its term
// (reg_predict), the fields of `expand` from the trial's group row P[group[i]];
// the others are not written. The v slot is NOT written here: the drift of the
// Q recurrence goes there (launch_rl_scan), and a regressed v, the trial's
// drift scaling, goes to vmul[i]. A regressed alpha goes to rate[i] as the
// learning rate rl_rate(link(eta)) (rl_update.hpp).
struct RlRegFill {
  int64_t n;
  int32_t C;
  int32_t n_terms;
  const double* X;        // [C * n] column-major: column c is X + c * n
  const int32_t* group;   // [n] group of a stored trial (null: one group)
  const double* coef;     // [G * C] coefficient rows, read through the trial's group
  const Params* P;        // [G] parameter rows
  int expand;             // bits 1, 2, 3, 5 (sv, a, z, t) of the non-regressed fields
  double* arr;            // [7 * n]
  double* vmul;           // [n] (null unless v is regressed)
  double* rate;           // [n] (null unless alpha is regressed)
  double* pred_in;        // nullable [n_terms * n]: the predictions in the caller's order
                          // (the alpha term: after the link, before squashing)
  double* rate_in;        // nullable [n]: the learning rates in the caller's order
  const int64_t* caller;  // [n] the caller's index of a stored trial (null: identity)
  RegTerm term[kRlRegMaxTerms];
};
void launch_rl_reg_fill(const RlRegFill& F, hipStream_t s);

}  // namespace wfpt
