// reg_internal.h — launcher interface between the C ABI (capi_*.cpp) and the
// regression front end (reg_kernels.hip). Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wfpt {
struct Params;


constexpr int kRegMaxTerms = 7;  // one term per parameter (v .. st) at the most
constexpr int kRegIdentity = 0, kRegExp = 1, kRegInvLogit = 2;  // WFPT_LINK_*

// One regression term (wfpt_reg_term): the parameter it predicts (0..6 = v,
// sv, a, z, sz, t, st), the link, and its columns [col0, col0 + ncol) of X.
struct RegTerm {
  int32_t param, link, col0, ncol;
};

// One fill launch. Trials are in stored order (group-major).
// Term k's predicted parameter goes to arr[k * n + i]; the fields of `expand`
// (bit f = field f of the wfpt_params order, non-regressed parameters of the
// groups call) follow from slot n_terms on, in rising field order, copied from
// the trial's group row P[group[i]].
struct RegFill {
  int64_t n;
  int32_t C;
  int32_t n_terms;
  const double* X;       // [C * n] column-major: column c is X + c * n
  const int32_t* group;  // [n] group of a stored trial (null: one group)
  const double* coef;    // [G * C] coefficient rows, read through the trial's group
  const Params* P;       // [G] parameter rows (null with expand == 0)
  int expand;
  double* arr;           // [(n_terms + popcount(expand)) * n]
  double* pred_in;       // nullable [n_terms * n]: the predictions in the caller's order
  const int64_t* caller; // [n] the caller's index of a stored trial (null: identity)
  RegTerm term[kRegMaxTerms];
};

// The linear predictor of term k is formed left to right, every product and
// every sum rounded separately:
//   eta = X[i, col0] * b[col0]; eta = eta + X[i, col0 + 1] * b[col0 + 1]; ...
// then IDENTITY: eta; EXP: cr_exp(eta) (correctly rounded, wfpt_crlibm.hpp);
// INVLOGIT: 1 / (1 + cr_exp(-eta)), each operation rounded once.
void launch_reg_fill(const RegFill& F, hipStream_t s);
}  // namespace wfpt
