// capi_reg.cpp — the regression family of the C ABI: the likelihoods
// (hddm/models/hddm_regression.py:26-36 into wfpt.pyx:244-274;
// reg_kernels.hip) and the posterior predictive's trial-wise
// drift sampler (hddm_regression.py:39-56; reg_sim_kernels.hip).
#include "capi_internal.hpp"
#include "capi_layout.hpp"
#include "reg_internal.h"
#include "rl_internal.h"  // kRlNodeMax: the per-group sum is the RL unit's launch_rl_node_sum
#include "stats_internal.h"

using namespace wfpt::capi;

// The fixed inputs of a regression likelihood, resident: signed RTs and the
// design matrix, group-major (reg_layout_host).
#pragma GCC visibility push(hidden)
struct wfpt_reg_ds : DsBase {
  int64_t n = 0;
  int32_t C = 0;
  int32_t n_groups = 1;     // 1 without group ids
  DevBuf<double> x;         // [n] signed RTs, stored order (+-999 kept: a missing response)
  DevBuf<double> X;         // [C * n] column c at X + c * n, stored order
  DevBuf<int32_t> group;    // [n] group of a stored trial (null without group ids)
  DevBuf<int64_t> off;      // [n_groups + 1] stored range of each group
  DevBuf<int64_t> caller;   // [n] the caller's index of a stored trial (null: identity)
  std::vector<int64_t> off_host;
  std::vector<int64_t> caller_host;  // empty: identity
  int64_t group_max = 0;    // most trials in one group
  void free_device() override { release_all(x, X, group, off, caller); }
};
#pragma GCC visibility pop

namespace wfpt {
namespace capi {

RegHostLayout reg_layout_host(const double* rt, int64_t n, const double* X, int32_t C,
                              const int32_t* group_id, int32_t n_groups) {
  RegHostLayout H;
  const int32_t G = group_id ? n_groups : 1;
  for (int64_t i = 0; group_id && i < n; ++i)
    if (group_id[i] < 0 || group_id[i] >= G) {
      H.rc = WFPT_ERR_ARG;
      H.msg = "group id out of range at trial " + std::to_string(i);
      return H;
    }
  std::vector<int64_t>& idx = H.caller;
  idx = std::vector<int64_t>(n);
  for (int64_t i = 0; i < n; ++i) idx[i] = i;
  if (group_id) {
    std::stable_sort(idx.begin(), idx.end(),
                     [&](int64_t a, int64_t b) { return group_id[a] < group_id[b]; });
    for (int64_t i = 0; i < n && H.identity; ++i) H.identity = idx[i] == i;
  }
  H.x = std::vector<double>(n);
  H.X = std::vector<double>((size_t)C * n);
  H.group = std::vector<int32_t>(group_id ? n : 0);
  H.off = std::vector<int64_t>(G + 1, 0);
  for (int64_t j = 0; j < n; ++j) {
    const int64_t src = idx[j];
    H.x[j] = rt[src];
    for (int32_t col = 0; col < C; ++col) H.X[(size_t)col * n + j] = X[(size_t)src * C + col];
    const int32_t g = group_id ? group_id[src] : 0;
    if (group_id) H.group[j] = g;
    H.off[g + 1]++;
  }
  for (int32_t g = 0; g < G; ++g) {
    H.group_max = std::max(H.group_max, H.off[g + 1]);
    H.off[g + 1] += H.off[g];
  }
  return H;
}

// The checks of a term list that need no data set: parameter 0..max_param,
// each named once, a known link, ncol >= 1, col0 >= 0.
int reg_check_terms(const wfpt_reg_term* terms, int32_t n_terms, int max_param) {
  const bool rl = max_param > 6;  // the RL regression entries: 7 = alpha (capi_rl_reg.cpp)
  if (n_terms < 0 || n_terms > max_param + 1)
    return fail(WFPT_ERR_ARG, rl ? "n_terms must be 0..8 (one term per parameter)"
                                 : "n_terms must be 0..7 (one term per parameter)");
  if (n_terms > 0 && !terms) return fail(WFPT_ERR_ARG, "null pointer (terms)");
  unsigned seen = 0;
  for (int32_t k = 0; k < n_terms; ++k) {
    const wfpt_reg_term& T = terms[k];
    const std::string at = " (term " + std::to_string(k) + ")";
    if (T.param < 0 || T.param > max_param)
      return fail(WFPT_ERR_ARG,
                  (rl ? "term parameter outside 0..7 (v, sv, a, z, sz, t, st, alpha)"
                      : "term parameter outside 0..6 (v, sv, a, z, sz, t, st)") + at);
    if (seen & (1u << T.param)) return fail(WFPT_ERR_ARG, "a parameter is named twice" + at);
    seen |= 1u << T.param;
    if (T.link != WFPT_LINK_IDENTITY && T.link != WFPT_LINK_EXP && T.link != WFPT_LINK_INVLOGIT)
      return fail(WFPT_ERR_ARG, "unknown link" + at);
    if (T.ncol < 1) return fail(WFPT_ERR_ARG, "ncol < 1" + at);
    if (T.col0 < 0) return fail(WFPT_ERR_ARG, "column range outside [0, C)" + at);
  }
  return WFPT_OK;
}

}  // namespace capi
}  // namespace wfpt

namespace {

// The rest of an entry's checks, still before any device work.
int reg_check_call(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                   int32_t n_terms) {
  if (d->ctx != c) return fail(WFPT_ERR_ARG, "regression dataset belongs to another context");
  for (int32_t k = 0; k < n_terms; ++k)
    if ((int64_t)terms[k].col0 + terms[k].ncol > d->C)
      return fail(WFPT_ERR_ARG,
                  "column range outside [0, C) (term " + std::to_string(k) + ")");
  return WFPT_OK;
}

// Uploads the call's coefficient rows, opens the profile bracket and launches
// reg_fill_kernel: term k's predictions into c->reg.arr[k n ..], the fields of
// `expand` after them. by_group: coefficients and rows are read through the
// trial's group, else row 0 serves every trial.
int reg_fill(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms, int32_t n_terms,
             const double* coef, int32_t rows, bool by_group, int expand, bool want_pred) {
  int slots = n_terms;
  for (int f = 0; f < 7; ++f) slots += (expand >> f) & 1;
  HIP_TRY(c->reg.arr.reserve(std::max<int64_t>((int64_t)slots * d->n, 1)));
  HIP_TRY(c->reg.coef.reserve(std::max<int64_t>((int64_t)rows * d->C, 1)));
  if (want_pred) HIP_TRY(c->reg.pred.reserve(std::max<int64_t>((int64_t)n_terms * d->n, 1)));
  HIP_TRY(hipMemcpyAsync(c->reg.coef.p, coef, (size_t)rows * d->C * sizeof(double),
                         hipMemcpyHostToDevice, c->stream));
  if (c->count) HIP_TRY(hipMemsetAsync(c->evals.p, 0, sizeof(unsigned long long), c->stream));
  if (c->profile) HIP_TRY(hipEventRecord(c->ev0, c->stream));
  wfpt::RegFill F;
  F.n = d->n;
  F.C = d->C;
  F.n_terms = n_terms;
  F.X = d->X.p;
  F.group = by_group ? d->group.p : nullptr;
  F.coef = c->reg.coef.p;
  F.P = expand ? c->reg.par.p : nullptr;
  F.expand = expand;
  F.arr = c->reg.arr.p;
  F.pred_in = want_pred ? c->reg.pred.p : nullptr;
  F.caller = d->caller.p;
  for (int k = 0; k < wfpt::kRegMaxTerms; ++k)
    F.term[k] = k < n_terms ? wfpt::RegTerm{terms[k].param, terms[k].link, terms[k].col0,
                                            terms[k].ncol}
                            : wfpt::RegTerm{0, 0, 0, 0};
  wfpt::launch_reg_fill(F, c->stream);
  HIP_TRY(hipGetLastError());
  return WFPT_OK;
}

// The _ex outputs of a finished call, in the caller's order.
int reg_outputs(wfpt_ctx* c, const wfpt_reg_ds* d, int32_t n_terms, double* out_trial,
                double* out_pred) {
  if (out_trial && d->n > 0) {
    if (d->caller_host.empty()) {
      HIP_TRY(hipMemcpy(out_trial, c->lp.p, d->n * sizeof(double), hipMemcpyDeviceToHost));
    } else {
      std::vector<double> h(d->n);
      HIP_TRY(hipMemcpy(h.data(), c->lp.p, d->n * sizeof(double), hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < d->n; ++i) out_trial[d->caller_host[i]] = h[i];
    }
  }
  if (out_pred && d->n > 0 && n_terms > 0)
    HIP_TRY(hipMemcpy(out_pred, c->reg.pred.p, (size_t)n_terms * d->n * sizeof(double),
                      hipMemcpyDeviceToHost));
  return WFPT_OK;
}

// The groups call after its checks, the context locked: the G per-group sums
// into out_logp, every trial's term left in c->lp (stored order).
int reg_groups_locked(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                      int32_t n_terms, const double* coef, const wfpt_params* per_group,
                      const wfpt::Knobs& K, double p_outlier, bool want_pred, double* out_logp) {
  const int32_t G = d->n_groups;
  const int64_t n = d->n;
  int term_of[7] = {-1, -1, -1, -1, -1, -1, -1};
  for (int32_t t = 0; t < n_terms; ++t) term_of[terms[t].param] = t;
  // v, sv, a, z and t per trial from the group rows unless regressed; sz and st
  // stay scalars of the pass unless regressed, as in the single call, so a
  // group's trials take the kernel the single call on that group takes
  int expand = 0;
  for (int f : {0, 1, 2, 3, 5})
    if (term_of[f] < 0) expand |= 1 << f;
  std::vector<wfpt::Params> par(G);
  for (int32_t j = 0; j < G; ++j) par[j] = to_params(&per_group[j]);
  HIP_TRY(c->reg.par.reserve(G));
  HIP_TRY(hipMemcpyAsync(c->reg.par.p, par.data(), G * sizeof(wfpt::Params),
                         hipMemcpyHostToDevice, c->stream));
  if (int rc = reg_fill(c, d, terms, n_terms, coef, G, true, expand, want_pred))
    return rc;
  double* field[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int f = 0, slot = n_terms; f < 7; ++f) {
    if (term_of[f] >= 0) field[f] = c->reg.arr.p + (int64_t)term_of[f] * n;
    else if (expand & (1 << f)) field[f] = c->reg.arr.p + (int64_t)slot++ * n;
  }
  if (int rc = score_runs(c, d->x.p, field, per_group, G, d->off_host.data(), d->off.p,
                          c->reg.npart, K, p_outlier, out_logp))
    return rc;
  return WFPT_OK;
}

// ---------------------------------------------------------------------------
// The regressor's posterior predictive (reg_sim_kernel; hddm_regression.py:39-56
// over generate.py:208-319)

struct RegSimDebug {
  double *par, *y0, *delay, *drift;
  int64_t *n_steps, *wave_steps;
};
struct RegStatsReq {
  const double* q;
  int32_t nq;
  double* out;  // [S x G x (8 + 2 nq)]
};

int gen_rts_reg_drift_impl(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                           int32_t n_terms, const double* coef, const wfpt_params* params,
                           int64_t S, double dt, double intra_sv, int64_t max_steps,
                           uint64_t seed, int32_t wave_draws, int64_t workspace_bytes,
                           double* out, int64_t* n_unfinished, int64_t* n_invalid,
                           const RegSimDebug& D, const RegStatsReq* sr) {
  const std::string name = sr ? "gen_rts_reg_drift_stats" : "gen_rts_reg_drift";
  if (int rc = reg_check_terms(terms, n_terms)) return rc;
  if (!c || !d || !coef || !params || !n_unfinished || !n_invalid)
    return fail(WFPT_ERR_ARG, "null pointer (context / dataset / coef / params / n_unfinished / "
                              "n_invalid)");
  if (!out && !sr) return fail(WFPT_ERR_ARG, "null pointer (out)");
  if (S < 1) return fail(WFPT_ERR_ARG, name + ": S < 1");
  if (!(dt > 0) || !std::isfinite(dt)) return fail(WFPT_ERR_ARG, name + ": dt <= 0");
  if (!(intra_sv > 0) || !std::isfinite(intra_sv))
    return fail(WFPT_ERR_ARG, name + ": intra_sv <= 0");
  if (max_steps < 1 || max_steps > (int64_t)1 << 31)
    return fail(WFPT_ERR_ARG, name + ": max_steps outside [1, 2^31]");
  if (wave_draws < 0 || wave_draws % 64 != 0)
    return fail(WFPT_ERR_ARG, name + ": wave_draws must be a multiple of 64 (0: default)");
  if (workspace_bytes < 0) return fail(WFPT_ERR_ARG, name + ": negative workspace_bytes");
  const double root = std::sqrt(dt);
  const double step = root * intra_sv, scale = root / intra_sv;  // generate.py:258, 279
  if (!(step > 0) || !std::isfinite(step) || !std::isfinite(scale))
    return fail(WFPT_ERR_ARG, name + ": sqrt(dt) * intra_sv is not a usable step");
  if (sr)
    if (int rc = stats_check_q(name.c_str(), sr->q, sr->nq, sr->out)) return rc;
  if (int rc = reg_check_call(c, d, terms, n_terms)) return rc;
  const int64_t n = d->n;
  const int32_t G = d->n_groups, C = d->C;
  if (n >= (int64_t)1 << 31)
    return fail(WFPT_ERR_ARG, name + ": the data set must hold < 2^31 trials");
  // Sweeps per tile: as many as the workspace holds draws of (the sampler's
  // 1 GiB by default), and few enough for the statistics' 32-bit row index.
  // The counter keying makes the tiling invisible in the result.
  const int64_t ws = workspace_bytes > 0 ? workspace_bytes : (int64_t)1 << 30;
  int64_t spt = std::max<int64_t>(1, ws / 8 / std::max<int64_t>(n, 1));
  spt = std::min(spt, S);
  spt = std::min(spt, std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / G));
  // Elements per wave: one per lane until that gives every SIMD four waves
  // (1024 SIMDs), then up to 16 per lane (gen_rts_drift_nodes' rule, per tile).
  auto wave_of = [&](int64_t tt) {
    return wave_draws > 0 ? (int64_t)wave_draws
                          : 64 * std::min<int64_t>(16, std::max<int64_t>(1, tt / (64 * 4096)));
  };
  const int64_t tt_max = spt * n, waves_max = (tt_max + wave_of(tt_max) - 1) / wave_of(tt_max);
  if (waves_max >= (int64_t)1 << 31)
    return fail(WFPT_ERR_ARG, name + ": too many draws for one launch; lower workspace_bytes");
  if (D.wave_steps && (wave_draws == 0 || spt < S))
    return fail(WFPT_ERR_ARG, name + ": out_wave_steps needs an explicit wave_draws and a "
                                     "workspace that holds every sweep");
  *n_unfinished = 0;
  *n_invalid = 0;
  if (n == 0 && !sr) return WFPT_OK;
  WFPT_RANGE("wfpt_gen_rts_reg_drift");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  std::vector<wfpt::Params> par((size_t)S * G);
  for (int64_t r = 0; r < S * G; ++r) par[r] = to_params(&params[r]);
  const bool dbg = D.par || D.y0 || D.delay || D.drift;
  HIP_TRY(c->reg.coef.reserve(std::max<int64_t>(spt * G * C, 1)));
  HIP_TRY(c->reg.par.reserve(spt * G));
  HIP_TRY(c->sim.out.reserve(std::max<int64_t>(tt_max, 1)));
  HIP_TRY(c->stats.count.reserve(2));
  if (dbg) HIP_TRY(c->sim.u.reserve(std::max<int64_t>(10 * tt_max, 1)));
  if (D.n_steps || D.wave_steps) HIP_TRY(c->sim.idx.reserve(tt_max + waves_max));
  HIP_TRY(hipMemsetAsync(c->stats.count.p, 0, 2 * sizeof(unsigned long long), c->stream));
  if (c->profile)
    for (int k = 0; k < 2; ++k)
      if (!c->sim.ev[k]) HIP_TRY(hipEventCreate(&c->sim.ev[k]));
  const std::vector<int64_t>& perm = d->caller_host;  // empty: the caller's order is the stored one
  std::vector<double> h;
  std::vector<int64_t> hi;
  std::vector<int64_t> goff;
  const int K = wfpt::stats_cols(sr ? sr->nq : 0);
  for (int64_t s0 = 0; s0 < S; s0 += spt) {
    const int64_t st = std::min(spt, S - s0), tt = st * n;
    const int64_t wd = wave_of(tt), waves = (tt + wd - 1) / wd;
    HIP_TRY(hipMemcpyAsync(c->reg.coef.p, coef + s0 * G * C, (size_t)st * G * C * sizeof(double),
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->reg.par.p, par.data() + s0 * G, (size_t)st * G * sizeof(wfpt::Params),
                           hipMemcpyHostToDevice, c->stream));
    wfpt::RegSimCall R;
    R.n = n;
    R.C = C;
    R.G = G;
    R.n_terms = n_terms;
    R.wave_draws = (int32_t)wd;
    R.X = d->X.p;
    R.group = d->group.p;
    R.caller = d->caller.p;
    R.coef = c->reg.coef.p;
    R.P = c->reg.par.p;
    R.s0 = s0;
    R.total = tt;
    R.dt = dt;
    R.step = step;
    R.scale = scale;
    R.max_steps = (uint32_t)max_steps;
    R.seed = seed;
    R.out = c->sim.out.p;
    R.par = D.par ? c->sim.u.p : nullptr;
    R.y0 = D.y0 ? c->sim.u.p + 7 * tt : nullptr;
    R.delay = D.delay ? c->sim.u.p + 8 * tt : nullptr;
    R.drift = D.drift ? c->sim.u.p + 9 * tt : nullptr;
    R.n_steps = D.n_steps ? c->sim.idx.p : nullptr;
    R.wave_steps = D.wave_steps ? c->sim.idx.p + tt : nullptr;
    R.counts = c->stats.count.p;
    for (int k = 0; k < wfpt::kRegMaxTerms; ++k)
      R.term[k] = k < n_terms ? wfpt::RegTerm{terms[k].param, terms[k].link, terms[k].col0,
                                              terms[k].ncol}
                              : wfpt::RegTerm{0, 0, 0, 0};
    if (c->profile) HIP_TRY(hipEventRecord(c->sim.ev[0], c->stream));
    wfpt::launch_reg_sim(R, c->stream);
    HIP_TRY(hipGetLastError());
    if (c->profile) {
      HIP_TRY(hipEventRecord(c->sim.ev[1], c->stream));
      HIP_TRY(hipEventSynchronize(c->sim.ev[1]));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, c->sim.ev[0], c->sim.ev[1]));
      c->k_ms += ms;
      c->launches += 1;
    }
    if (sr) {  // row (s, g) of the tile: the stored range of group g in sweep s
      goff.resize((size_t)st * G + 1);
      for (int64_t s = 0; s < st; ++s)
        for (int32_t j = 0; j < G; ++j) goff[s * G + j] = s * n + d->off_host[j];
      goff[st * G] = tt;
      if (int rc = stats_device_rows(c, name.c_str(), c->sim.out.p, goff.data(), st * G, sr->q,
                                     sr->nq, sr->out + s0 * G * K))
        return rc;
    } else {
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (tt == 0) continue;
    // the tile's per-element arrays, stored order on the device, into the
    // caller's order: element (s, p) is trial perm[p] of sweep s0 + s
    auto fetch = [&](double* dst, const double* dev) -> int {
      if (perm.empty()) {
        HIP_TRY(hipMemcpy(dst, dev, tt * sizeof(double), hipMemcpyDeviceToHost));
        return WFPT_OK;
      }
      h.resize((size_t)tt);
      HIP_TRY(hipMemcpy(h.data(), dev, tt * sizeof(double), hipMemcpyDeviceToHost));
      for (int64_t s = 0; s < st; ++s)
        for (int64_t p = 0; p < n; ++p) dst[s * n + perm[p]] = h[s * n + p];
      return WFPT_OK;
    };
    const std::pair<double*, const double*> copies[] = {
        {out, R.out}, {D.y0, R.y0}, {D.delay, R.delay}, {D.drift, R.drift}};
    for (const auto& cp : copies)
      if (cp.first)
        if (int rc = fetch(cp.first + s0 * n, cp.second)) return rc;
    if (D.par) {  // (S, n, 7) on the host, field-major on the device
      h.resize((size_t)7 * tt);
      HIP_TRY(hipMemcpy(h.data(), R.par, 7 * tt * sizeof(double), hipMemcpyDeviceToHost));
      for (int f = 0; f < 7; ++f)
        for (int64_t s = 0; s < st; ++s)
          for (int64_t p = 0; p < n; ++p)
            D.par[((s0 + s) * n + (perm.empty() ? p : perm[p])) * 7 + f] = h[f * tt + s * n + p];
    }
    if (D.n_steps) {
      hi.resize((size_t)tt);
      HIP_TRY(hipMemcpy(hi.data(), R.n_steps, tt * sizeof(int64_t), hipMemcpyDeviceToHost));
      for (int64_t s = 0; s < st; ++s)
        for (int64_t p = 0; p < n; ++p)
          D.n_steps[(s0 + s) * n + (perm.empty() ? p : perm[p])] = hi[s * n + p];
    }
    if (D.wave_steps)
      HIP_TRY(hipMemcpy(D.wave_steps, R.wave_steps, waves * sizeof(int64_t),
                        hipMemcpyDeviceToHost));
  }
  unsigned long long counts[2] = {0, 0};
  HIP_TRY(hipMemcpy(counts, c->stats.count.p, sizeof(counts), hipMemcpyDeviceToHost));
  *n_invalid = (int64_t)counts[0];
  *n_unfinished = (int64_t)counts[1];
  return WFPT_OK;
}

}  // namespace

extern "C" {

int wfpt_gen_rts_reg_drift_ex(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                              int32_t n_terms, const double* coef, const wfpt_params* params,
                              int64_t S, double dt, double intra_sv, int64_t max_steps,
                              uint64_t seed, int32_t wave_draws, int64_t workspace_bytes,
                              double* out, int64_t* n_unfinished, int64_t* n_invalid,
                              double* out_params, double* out_y0, double* out_delay,
                              double* out_drift, int64_t* out_n_steps, int64_t* out_wave_steps) {
  const RegSimDebug D{out_params, out_y0, out_delay, out_drift, out_n_steps, out_wave_steps};
  return gen_rts_reg_drift_impl(c, d, terms, n_terms, coef, params, S, dt, intra_sv, max_steps,
                                seed, wave_draws, workspace_bytes, out, n_unfinished, n_invalid, D,
                                nullptr);
}

int wfpt_gen_rts_reg_drift(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                           int32_t n_terms, const double* coef, const wfpt_params* params,
                           int64_t S, double dt, double intra_sv, int64_t max_steps, uint64_t seed,
                           double* out, int64_t* n_unfinished, int64_t* n_invalid) {
  return gen_rts_reg_drift_impl(c, d, terms, n_terms, coef, params, S, dt, intra_sv, max_steps,
                                seed, 0, 0, out, n_unfinished, n_invalid, RegSimDebug{}, nullptr);
}

int wfpt_gen_rts_reg_drift_stats(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                                 int32_t n_terms, const double* coef, const wfpt_params* params,
                                 int64_t S, double dt, double intra_sv, int64_t max_steps,
                                 uint64_t seed, int64_t workspace_bytes, double* out,
                                 int64_t* n_unfinished, int64_t* n_invalid, const double* q,
                                 int32_t nq, double* stats_out) {
  const RegStatsReq sr{q, nq, stats_out};
  return gen_rts_reg_drift_impl(c, d, terms, n_terms, coef, params, S, dt, intra_sv, max_steps,
                                seed, 0, workspace_bytes, out, n_unfinished, n_invalid,
                                RegSimDebug{}, &sr);
}

int wfpt_reg_dataset_create(wfpt_ctx* c, const double* rt, int64_t n, const double* X, int32_t C,
                            const int32_t* group_id, int32_t n_groups, wfpt_reg_ds** out) {
  if (!c || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (n < 0) return fail(WFPT_ERR_ARG, "n < 0");
  if (C < 1) return fail(WFPT_ERR_ARG, "the design matrix needs at least one column");
  if (n > 0 && (!rt || !X)) return fail(WFPT_ERR_ARG, "null rt / design matrix");
  if (group_id && n_groups <= 0) return fail(WFPT_ERR_ARG, "group ids need n_groups > 0");
  RegHostLayout H = reg_layout_host(rt, n, X, C, group_id, n_groups);
  if (H.rc) return fail(H.rc, H.msg);
  WFPT_RANGE("wfpt_reg_dataset_create");
  auto* d = new wfpt_reg_ds();
  d->n = n;
  d->C = C;
  d->n_groups = group_id ? n_groups : 1;
  d->group_max = H.group_max;
  d->off_host = H.off;
  if (!H.identity) d->caller_host = H.caller;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  hipError_t e = upload_vec(d->x, H.x);
  if (e == hipSuccess) e = upload_vec(d->X, H.X);
  if (e == hipSuccess && group_id) e = upload_vec(d->group, H.group);
  if (e == hipSuccess) e = upload_vec(d->off, H.off);
  if (e == hipSuccess && !H.identity) e = upload_vec(d->caller, H.caller);
  if (e != hipSuccess) {
    delete d;  // frees what was uploaded (the context's device is current)
    return fail(WFPT_ERR_HIP, std::string("regression dataset upload: ") + hipGetErrorString(e));
  }
  ds_register(c, d);
  *out = d;
  return WFPT_OK;
}

void wfpt_reg_dataset_destroy(wfpt_reg_ds* d) { ds_destroy(d); }

int wfpt_wiener_like_reg_ex(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                            int32_t n_terms, const double* coef, const wfpt_params* p,
                            const wfpt_knobs* k, double* out, double* out_trial,
                            double* out_pred) {
  if (int rc = reg_check_terms(terms, n_terms)) return rc;
  if (!c || !d || !coef || !p || !k || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (int rc = reg_check_call(c, d, terms, n_terms)) return rc;
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_reg");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const int64_t n = d->n;
  if (int rc = reg_fill(c, d, terms, n_terms, coef, 1, false, 0, out_pred != nullptr)) return rc;
  // a regressed parameter is an array of the pass, every other one its scalar,
  // as wiener_like_multi(multi=[the regressed ones]) passes them
  double* dptr[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double scal[7] = {p->v, p->sv, p->a, p->z, p->sz, p->t, p->st};
  for (int32_t t = 0; t < n_terms; ++t) {
    dptr[terms[t].param] = c->reg.arr.p + (int64_t)t * n;
    scal[terms[t].param] = 0.0;
  }
  if (int rc = multi_score(c, d->x.p, n, dptr, scal, K, p->p_outlier)) return rc;
  if (int rc = multi_finish(c, n, out)) return rc;
  return reg_outputs(c, d, n_terms, out_trial, out_pred);
}

int wfpt_wiener_like_reg(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                         int32_t n_terms, const double* coef, const wfpt_params* p,
                         const wfpt_knobs* k, double* out) {
  return wfpt_wiener_like_reg_ex(c, d, terms, n_terms, coef, p, k, out, nullptr, nullptr);
}

int wfpt_wiener_like_reg_groups_ex(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                                   int32_t n_terms, const double* coef,
                                   const wfpt_params* per_group, const wfpt_knobs* k,
                                   double* out_logp, double* out_trial, double* out_pred) {
  if (int rc = reg_check_terms(terms, n_terms)) return rc;
  if (!c || !d || !coef || !per_group || !k || !out_logp)
    return fail(WFPT_ERR_ARG, "null pointer");
  if (int rc = reg_check_call(c, d, terms, n_terms)) return rc;
  const int32_t G = d->n_groups;
  if (d->group_max > wfpt::kRlNodeMax)
    return fail(WFPT_ERR_UNSUPPORTED, "a group holds more trials than the per-group sum takes");
  for (int32_t j = 1; j < G; ++j)  // the per-trial-parameter pass takes one p_outlier
    if (per_group[j].p_outlier != per_group[0].p_outlier)
      return fail(WFPT_ERR_UNSUPPORTED, "the groups call needs one p_outlier for all groups");
  const double p_outlier = per_group[0].p_outlier;
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_reg_groups");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (int rc = reg_groups_locked(c, d, terms, n_terms, coef, per_group, K, p_outlier,
                                 out_pred != nullptr, out_logp))
    return rc;
  return reg_outputs(c, d, n_terms, out_trial, out_pred);
}

int wfpt_pointwise_reg_groups(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                              int32_t n_terms, const double* coef, const wfpt_params* per_group,
                              int64_t S, const wfpt_knobs* k, int64_t max_workspace,
                              double* out_sums, double* out_stats, int64_t* out_ninf_total) {
  if (int rc = reg_check_terms(terms, n_terms)) return rc;
  if (!c || !d || !coef || !per_group || !k || !out_sums || !out_stats || !out_ninf_total)
    return fail(WFPT_ERR_ARG, "null pointer");
  if (S < 1) return fail(WFPT_ERR_ARG, "S < 1");
  if (int rc = reg_check_call(c, d, terms, n_terms)) return rc;
  const int32_t G = d->n_groups;
  if (d->group_max > wfpt::kRlNodeMax)
    return fail(WFPT_ERR_UNSUPPORTED, "a group holds more trials than the per-group sum takes");
  for (int64_t s = 0; s < S; ++s)  // the per-trial-parameter pass takes one p_outlier
    for (int32_t j = 1; j < G; ++j)
      if (per_group[s * G + j].p_outlier != per_group[s * G].p_outlier)
        return fail(WFPT_ERR_UNSUPPORTED, "the groups call needs one p_outlier for all groups");
  const wfpt::Knobs K = to_knobs(k);
  (void)max_workspace;  // the groups call scores one table: a tile is one sweep
  WFPT_RANGE("wfpt_pointwise_reg_groups");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (int rc = pointwise_begin(c, d->n)) return rc;
  for (int64_t s = 0; s < S; ++s) {  // the state stays on the device between sweeps
    if (int rc = reg_groups_locked(c, d, terms, n_terms, coef + s * G * d->C, per_group + s * G, K,
                                   per_group[s * G].p_outlier, false, out_sums + s * G))
      return rc;
    if (int rc = pointwise_add(c, c->lp.p, 1)) return rc;
  }
  return pointwise_finish(c, S, d->caller_host.empty() ? nullptr : d->caller_host.data(),
                          out_stats, out_ninf_total);
}

int wfpt_wiener_like_reg_groups(wfpt_ctx* c, const wfpt_reg_ds* d, const wfpt_reg_term* terms,
                                int32_t n_terms, const double* coef,
                                const wfpt_params* per_group, const wfpt_knobs* k,
                                double* out_logp) {
  return wfpt_wiener_like_reg_groups_ex(c, d, terms, n_terms, coef, per_group, k, out_logp,
                                        nullptr, nullptr);
}

}  // extern "C"
