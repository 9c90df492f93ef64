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

// One launch of the regressor's posterior predictive (reg_sim_kernels.hip;
// hddm_regression.py:39-56 over generate.py:208-319): one
// simulated diffusion path per (sweep, trial) of a tile of sweeps. Element e
// of the tile is sweep s0 + e / n and stored trial p = e % n; its parameters
// are formed when a lane picks it up: the fields of P[(e / n) * G + group[p]],
// the regressed ones replaced by reg_predict over X[., p] and the coefficient
// row coef[((e / n) * G + group[p]) * C ..]. The walk is sim_drift_kernel's
// (DriftCall: step, scale, max_steps, wave_draws) without the in-trial switch,
// its random words Philox4x32-10 at counter (sweep lo, sweep hi, caller[p],
// stream), streams 1, 2, 3 and 16 + step / 4 as there. A trial whose formed
// parameters cannot be walked (walk_row_ok's rule, capi_sim.cpp) is NaN and
// counted in counts[0]; a walk cut at max_steps is NaN and counted in counts[1].
struct RegSimCall {
  int64_t n;             // trials per sweep, < 2^31
  int32_t C, G;          // design columns, groups
  int32_t n_terms;
  int32_t wave_draws;    // elements handed to one wave, a multiple of 64
  const double* X;       // [C * n] column-major, stored order
  const int32_t* group;  // [n] (null: one group)
  const int64_t* caller; // [n] the caller's index of a stored trial (null: identity)
  const double* coef;    // the tile's [sweeps * G * C] coefficient rows
  const Params* P;       // the tile's [sweeps * G] parameter rows
  int64_t s0;            // the tile's first sweep: the draw index of its element 0
  int64_t total;         // sweeps * n elements
  double dt, step, scale;
  uint32_t max_steps;    // 1 .. 2^31
  uint64_t seed;
  double* out;           // [total]
  double* par;           // nullable [7 * total]: field f of element e at par[f * total + e]
  double* y0;            // nullable, per element, NaN for an invalid trial
  double* delay;
  double* drift;
  int64_t* n_steps;      // nullable: steps taken, 0 for an invalid trial
  int64_t* wave_steps;   // nullable [ceil(total / wave_draws)]
  unsigned long long* counts;  // [2] invalid trials, cut walks: one atomic per wave each
  RegTerm term[kRegMaxTerms];
};
// The caller checks that the wave count fits a grid's x dimension.
void launch_reg_sim(const RegSimCall& C, hipStream_t s);
}  // namespace wfpt
