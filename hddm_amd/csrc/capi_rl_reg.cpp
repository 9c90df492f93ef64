// capi_rl_reg.cpp — the RL regression likelihood of the C ABI
// (hddm/models/hddm_rl_regression.py:25-38 into wiener_like_multi_rlddm,
// wfpt.pyx:277-320; rl_reg_kernels.hip): the regression data
// set's design matrix and the RL data set's run segments, resident together.
#include "capi_internal.hpp"
#include "capi_layout.hpp"
#include "rl_internal.h"
#include "rl_reg_internal.h"

using namespace wfpt::capi;

// Trials group-major, the caller's order kept inside a group (reg_layout_host);
// segments the runs of equal adjacent split_by inside a group (rl_layout_host,
// by_runs, the groups as nodes), every trial scored: compact == stored order.
#pragma GCC visibility push(hidden)
struct wfpt_rl_reg_ds : DsBase {
  int64_t n = 0;
  int32_t C = 0;
  int32_t n_groups = 1;  // 1 without group ids
  int32_t n_seg = 0;
  DevBuf<double> x;        // [n] signed RTs, stored order
  DevBuf<double> X;        // [C * n] column c at X + c * n, stored order
  DevBuf<int32_t> group;   // [n] group of a stored trial (null without group ids)
  DevBuf<int64_t> off;     // [n_groups + 1] stored range of each group
  DevBuf<int64_t> caller;  // [n] the caller's index of a stored trial (null: identity)
  DevBuf<int64_t> lane_start, lane_len, step_off;  // rl_internal.h: RlLayout
  DevBuf<int32_t> lane_node;                       // null without group ids
  DevBuf<unsigned char> resp_t;
  DevBuf<double> fb_t;
  std::vector<int64_t> off_host;
  std::vector<int64_t> caller_host;  // empty: identity
  int64_t group_max = 0;             // most trials in one group
  void free_device() override {
    release_all(x, X, group, off, caller, lane_start, lane_len, step_off, lane_node, resp_t, fb_t);
  }
};
#pragma GCC visibility pop

namespace {

int rl_reg_check_call(wfpt_ctx* c, const wfpt_rl_reg_ds* d, const wfpt_reg_term* terms,
                      int32_t n_terms) {
  if (d->ctx != c) return fail(WFPT_ERR_ARG, "RL regression dataset belongs to another context");
  for (int32_t k = 0; k < n_terms; ++k)
    if ((int64_t)terms[k].col0 + terms[k].ncol > d->C)
      return fail(WFPT_ERR_ARG,
                  "column range outside [0, C) (term " + std::to_string(k) + ")");
  return WFPT_OK;
}

// Per-trial workspace of a call in c->reg.arr: the seven fields of the scoring
// pass (the v slot holds the scan's drifts), then the drift scalings and the
// learning rates in stored order, then the learning rates in the caller's order.
constexpr int kSlotVmul = 7, kSlotRate = 8, kSlotRateIn = 9, kSlots = 10;

}  // namespace

extern "C" {

int wfpt_rl_reg_dataset_create(wfpt_ctx* c, const double* rt, const int64_t* response,
                               const double* feedback, const int64_t* split_by, int64_t n,
                               const double* X, int32_t C, const int32_t* group_id,
                               int32_t n_groups, wfpt_rl_reg_ds** out) {
  if (!c || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (n < 0) return fail(WFPT_ERR_ARG, "n < 0");
  if (C < 1) return fail(WFPT_ERR_ARG, "the design matrix needs at least one column");
  if (n > 0 && (!rt || !response || !feedback || !split_by || !X))
    return fail(WFPT_ERR_ARG, "null rt / response / feedback / split_by / design matrix");
  if (group_id && n_groups <= 0) return fail(WFPT_ERR_ARG, "group ids need n_groups > 0");
  RegHostLayout H = reg_layout_host(rt, n, X, C, group_id, n_groups);
  if (H.rc) return fail(H.rc, H.msg);
  // the same stable group-major order: stored index == the RL layout's
  RlHostLayout R = rl_layout_host(rt, response, feedback, split_by, n, group_id,
                                  group_id ? n_groups : 0, true);
  if (R.rc) return fail(R.rc, R.msg);
  WFPT_RANGE("wfpt_rl_reg_dataset_create");
  auto* d = new wfpt_rl_reg_ds();
  d->n = n;
  d->C = C;
  d->n_groups = group_id ? n_groups : 1;
  d->n_seg = R.n_seg;
  d->group_max = H.group_max;
  d->off_host = H.off;
  if (!H.identity) d->caller_host = H.caller;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  hipError_t e = hipSuccess;
  auto up = [&](auto& dst, const auto& v, bool wanted = true) {
    if (wanted && e == hipSuccess) e = upload_vec(dst, v);
  };
  up(d->x, H.x), up(d->X, H.X), up(d->group, H.group, group_id != nullptr), up(d->off, H.off);
  up(d->caller, H.caller, !H.identity);
  up(d->lane_start, R.lane_start), up(d->lane_len, R.lane_len), up(d->step_off, R.step_off);
  up(d->lane_node, R.lane_node, group_id != nullptr), up(d->resp_t, R.resp_t), up(d->fb_t, R.fb_t);
  if (e != hipSuccess) {
    delete d;  // frees what was uploaded (the context's device is current)
    return fail(WFPT_ERR_HIP,
                std::string("RL regression dataset upload: ") + hipGetErrorString(e));
  }
  ds_register(c, d);
  *out = d;
  return WFPT_OK;
}

void wfpt_rl_reg_dataset_destroy(wfpt_rl_reg_ds* d) { ds_destroy(d); }

int wfpt_wiener_like_rl_reg_groups_ex(wfpt_ctx* c, const wfpt_rl_reg_ds* d,
                                      const wfpt_reg_term* terms, int32_t n_terms,
                                      const double* coef, const double* q, const double* alpha,
                                      const wfpt_params* per_group, const wfpt_knobs* k,
                                      double* out_logp, double* out_trial, double* out_pred,
                                      double* out_drift, double* out_rate) {
  if (int rc = reg_check_terms(terms, n_terms, wfpt::kRlRegAlpha)) return rc;
  if (!c || !d || !coef || !q || !alpha || !per_group || !k || !out_logp)
    return fail(WFPT_ERR_ARG, "null pointer");
  if (int rc = rl_reg_check_call(c, d, terms, n_terms)) return rc;
  const int32_t G = d->n_groups;
  const int64_t n = d->n;
  if (d->group_max > wfpt::kRlNodeMax)
    return fail(WFPT_ERR_UNSUPPORTED, "a group holds more trials than the per-group sum takes");
  for (int32_t j = 1; j < G; ++j)  // the per-trial-parameter pass takes one p_outlier
    if (per_group[j].p_outlier != per_group[0].p_outlier)
      return fail(WFPT_ERR_UNSUPPORTED, "the groups call needs one p_outlier for all groups");
  const double p_outlier = per_group[0].p_outlier;
  const wfpt::Knobs K = to_knobs(k);
  int term_of[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  for (int32_t t = 0; t < n_terms; ++t) term_of[terms[t].param] = t;
  const bool reg_v = term_of[0] >= 0, reg_alpha = term_of[wfpt::kRlRegAlpha] >= 0;
  // sv, a, z and t per trial from the group rows unless regressed; sz and st
  // stay scalars of the pass unless regressed (wfpt_wiener_like_reg_groups)
  int expand = 0;
  for (int f : {1, 2, 3, 5})
    if (term_of[f] < 0) expand |= 1 << f;
  std::vector<wfpt::Params> par(G);
  std::vector<wfpt::RlRow> rows(G);
  for (int32_t j = 0; j < G; ++j) {
    par[j] = to_params(&per_group[j]);
    rows[j].q = q[j];
    rows[j].alfa = rows[j].pos_alfa = reg_alpha ? 0.0 : rl_rate(alpha[j]);  // host libm pow
    rows[j].v = per_group[j].v;
  }
  WFPT_RANGE("wfpt_wiener_like_rl_reg_groups");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HIP_TRY(c->reg.par.reserve(G));
  HIP_TRY(c->rl.rows.reserve(G));
  HIP_TRY(c->reg.coef.reserve(std::max<int64_t>((int64_t)G * d->C, 1)));
  HIP_TRY(c->reg.arr.reserve(std::max<int64_t>(kSlots * n, 1)));
  if (out_pred) HIP_TRY(c->reg.pred.reserve(std::max<int64_t>((int64_t)n_terms * n, 1)));
  if (out_drift) HIP_TRY(c->rl.drift_in.reserve(std::max<int64_t>(n, 1)));
  HIP_TRY(hipMemcpyAsync(c->reg.par.p, par.data(), G * sizeof(wfpt::Params),
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->rl.rows.p, rows.data(), G * sizeof(wfpt::RlRow),
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->reg.coef.p, coef, (size_t)G * d->C * sizeof(double),
                         hipMemcpyHostToDevice, c->stream));
  if (c->count) HIP_TRY(hipMemsetAsync(c->evals.p, 0, sizeof(unsigned long long), c->stream));
  if (c->profile) HIP_TRY(hipEventRecord(c->ev0, c->stream));
  double* arr = c->reg.arr.p;
  // 1. the trial-parallel fill
  wfpt::RlRegFill F;
  F.n = n;
  F.C = d->C;
  F.n_terms = n_terms;
  F.X = d->X.p;
  F.group = d->group.p;
  F.coef = c->reg.coef.p;
  F.P = c->reg.par.p;
  F.expand = expand;
  F.arr = arr;
  F.vmul = reg_v ? arr + kSlotVmul * n : nullptr;
  F.rate = reg_alpha ? arr + kSlotRate * n : nullptr;
  F.pred_in = out_pred ? c->reg.pred.p : nullptr;
  F.rate_in = out_rate && reg_alpha ? arr + kSlotRateIn * n : nullptr;
  F.caller = d->caller.p;
  for (int t = 0; t < wfpt::kRlRegMaxTerms; ++t)
    F.term[t] = t < n_terms ? wfpt::RegTerm{terms[t].param, terms[t].link, terms[t].col0,
                                            terms[t].ncol}
                            : wfpt::RegTerm{0, 0, 0, 0};
  wfpt::launch_rl_reg_fill(F, c->stream);
  HIP_TRY(hipGetLastError());
  // 2. the Q recurrence, one lane per run, the group's row: drifts into the v slot
  wfpt::RlLayout L;
  L.n_seg = d->n_seg;
  L.lane_start = d->lane_start.p;
  L.lane_out = d->lane_start.p;  // every trial scored: compact == stored
  L.lane_len = d->lane_len.p;
  L.lane_node = d->lane_node.p;
  L.step_off = d->step_off.p;
  L.resp_t = d->resp_t.p;
  L.fb_t = d->fb_t.p;
  L.caller = d->caller.p;
  L.score_first = 1;
  wfpt::launch_rl_scan(L, wfpt::RlRow{}, c->rl.rows.p, F.vmul, F.rate, arr,
                       out_drift ? c->rl.drift_in.p : nullptr, c->stream);
  HIP_TRY(hipGetLastError());
  // 3. the densities and the per-group sums
  double* field[7] = {arr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int f = 1; f < 7; ++f)
    if (term_of[f] >= 0 || (expand & (1 << f))) field[f] = arr + (int64_t)f * n;
  if (int rc = score_runs(c, d->x.p, field, per_group, G, d->off_host.data(), d->off.p,
                          c->reg.npart, K, p_outlier, out_logp))
    return rc;
  if (n == 0) return WFPT_OK;
  const std::vector<int64_t>& perm = d->caller_host;
  if (out_trial) {
    if (perm.empty()) {
      HIP_TRY(hipMemcpy(out_trial, c->lp.p, n * sizeof(double), hipMemcpyDeviceToHost));
    } else {
      std::vector<double> h(n);
      HIP_TRY(hipMemcpy(h.data(), c->lp.p, n * sizeof(double), hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < n; ++i) out_trial[perm[i]] = h[i];
    }
  }
  if (out_pred && n_terms > 0)
    HIP_TRY(hipMemcpy(out_pred, c->reg.pred.p, (size_t)n_terms * n * sizeof(double),
                      hipMemcpyDeviceToHost));
  if (out_drift)
    HIP_TRY(hipMemcpy(out_drift, c->rl.drift_in.p, n * sizeof(double), hipMemcpyDeviceToHost));
  if (out_rate && reg_alpha)
    HIP_TRY(hipMemcpy(out_rate, F.rate_in, n * sizeof(double), hipMemcpyDeviceToHost));
  if (out_rate && !reg_alpha)  // the group's host-squashed rate, every trial of the group
    for (int32_t j = 0; j < G; ++j)
      for (int64_t i = d->off_host[j]; i < d->off_host[j + 1]; ++i)
        out_rate[perm.empty() ? i : perm[i]] = rows[j].alfa;
  return WFPT_OK;
}

int wfpt_wiener_like_rl_reg_groups(wfpt_ctx* c, const wfpt_rl_reg_ds* d,
                                   const wfpt_reg_term* terms, int32_t n_terms,
                                   const double* coef, const double* q, const double* alpha,
                                   const wfpt_params* per_group, const wfpt_knobs* k,
                                   double* out_logp) {
  return wfpt_wiener_like_rl_reg_groups_ex(c, d, terms, n_terms, coef, q, alpha, per_group, k,
                                           out_logp, nullptr, nullptr, nullptr, nullptr);
}

}  // extern "C"
