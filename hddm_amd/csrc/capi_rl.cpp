// capi_rl.cpp — the reinforcement-learning family of the C ABI
// (wfpt.pyx:79-241, 277-320; rl_kernels.hip).
#include "capi_internal.hpp"
#include "capi_layout.hpp"
#include "rl_internal.h"

using namespace wfpt::capi;

// The fixed per-trial inputs of the RL likelihoods, resident: laid out once on
// the host (rl_layout_host; rl_internal.h: RlLayout), uploaded once.
#pragma GCC visibility push(hidden)
struct wfpt_rl_ds : DsBase {
  int64_t n = 0;        // trials
  int64_t m = 0;        // scored trials (all but each segment's first; all when by_runs)
  int32_t n_seg = 0;
  int32_t n_nodes = 0;  // 0: created without node ids
  bool has_rt = false;
  bool by_runs = false;  // wiener_like_multi_rlddm's segments (runs of equal split_by)
  DevBuf<double> x_c;    // [m] RTs of the scored trials, compact
  DevBuf<int64_t> lane_start, lane_out, lane_len;
  DevBuf<int32_t> lane_node;
  DevBuf<int64_t> step_off;
  DevBuf<unsigned char> resp_t;
  DevBuf<double> fb_t;
  DevBuf<int64_t> caller;
  DevBuf<unsigned char> resp_c;  // [m] responses of the scored trials
  DevBuf<int32_t> node_c;        // [m] their nodes
  DevBuf<int64_t> node_off;      // [n_nodes + 1] compact range of each node
  std::vector<int64_t> c2caller;    // host [m]: the caller's index of a compact trial
  std::vector<int64_t> node_off_host;  // host copy of node_off
  int64_t node_max = 0;             // most scored trials in one node
  // the multi-table node batch's view of the scored trials, grown on demand
  // (rl_replicate): x_c and the nodes' compact ranges once per table
  mutable int32_t rep_tables = 0;
  mutable DevBuf<double> x_rep;            // [rep_tables x m]
  mutable DevBuf<int64_t> off_rep;         // [rep_tables x n_nodes + 1]
  mutable std::vector<int64_t> off_rep_host;
  void free_device() override {
    release_all(x_c, lane_start, lane_out, lane_len, lane_node, step_off, resp_t, fb_t, caller,
                resp_c, node_c, node_off, x_rep, off_rep);
    rep_tables = 0;
  }
};
#pragma GCC visibility pop

namespace wfpt {
namespace capi {

RlHostLayout rl_layout_host(const double* rt, const int64_t* response, const double* feedback,
                            const int64_t* split_by, int64_t n, const int32_t* node_id,
                            int32_t n_nodes, bool by_runs) {
  RlHostLayout H;
  auto refuse = [&](const std::string& msg) {
    H.rc = WFPT_ERR_ARG;
    H.msg = msg;
    return H;
  };
  for (int64_t i = 0; i < n; ++i) {
    if (response[i] != 0 && response[i] != 1)
      return refuse("response must be 0 or 1 (trial " + std::to_string(i) + ")");
    if (rt && std::fabs(rt[i]) == 999.)
      return refuse("|rt| == 999 at trial " + std::to_string(i) +
                    ": the RL likelihoods have no missing-response code");
    if (node_id && (node_id[i] < 0 || node_id[i] >= n_nodes))
      return refuse("node id out of range at trial " + std::to_string(i));
  }
  std::vector<int64_t>& idx = H.caller;
  idx = std::vector<int64_t>(n);
  for (int64_t i = 0; i < n; ++i) idx[i] = i;
  if (!by_runs)
    std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) {
      if (node_id && node_id[a] != node_id[b]) return node_id[a] < node_id[b];
      return split_by[a] < split_by[b];
    });
  else if (node_id)  // node-major, the caller's order (and so its runs) kept inside a node
    std::stable_sort(idx.begin(), idx.end(),
                     [&](int64_t a, int64_t b) { return node_id[a] < node_id[b]; });
  std::vector<int64_t> seg_start;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t a = idx[j], b = j ? idx[j - 1] : 0;
    if (j == 0 || split_by[a] != split_by[b] || (node_id && node_id[a] != node_id[b]))
      seg_start.push_back(j);
  }
  if (seg_start.size() > (size_t)INT32_MAX) return refuse("too many segments");
  const int32_t ns = (int32_t)seg_start.size();
  seg_start.push_back(n);
  auto seg_len = [&](int32_t s) { return seg_start[s + 1] - seg_start[s]; };
  const int64_t m = by_runs ? n : n - ns;
  H.m = m;
  H.n_seg = ns;
  // lanes: the segments by falling length
  std::vector<int32_t> lane(ns);
  for (int32_t s = 0; s < ns; ++s) lane[s] = s;
  std::stable_sort(lane.begin(), lane.end(),
                   [&](int32_t a, int32_t b) { return seg_len(a) > seg_len(b); });
  const int64_t lmax = ns ? seg_len(lane[0]) : 0;
  std::vector<int64_t>& step_off = H.step_off;
  step_off = std::vector<int64_t>(lmax + 1, 0);
  for (int32_t s = 0; s < ns; ++s) step_off[seg_len(s)]++;  // histogram of the lengths
  {
    int64_t longer = 0, acc = 0;  // longer: segments with more than k trials
    for (int64_t k = lmax; k >= 0; --k) {
      const int64_t here = step_off[k];
      step_off[k] = longer;
      longer += here;
    }
    for (int64_t k = 0; k <= lmax; ++k) {  // counts -> offsets
      const int64_t cnt = step_off[k];
      step_off[k] = acc;
      acc += cnt;
    }
  }
  H.lane_start = H.lane_out = H.lane_len = std::vector<int64_t>(ns);
  H.lane_node = std::vector<int32_t>(node_id ? ns : 0);
  H.resp_t = std::vector<unsigned char>(n);
  H.fb_t = std::vector<double>(n);
  for (int32_t r = 0; r < ns; ++r) {
    const int32_t s = lane[r];
    H.lane_start[r] = seg_start[s];
    H.lane_out[r] = by_runs ? seg_start[s] : seg_start[s] - s;
    H.lane_len[r] = seg_len(s);
    if (node_id) H.lane_node[r] = node_id[idx[seg_start[s]]];
    for (int64_t k = 0; k < H.lane_len[r]; ++k) {
      const int64_t src = idx[seg_start[s] + k];
      H.resp_t[step_off[k] + r] = (unsigned char)response[src];
      H.fb_t[step_off[k] + r] = feedback[src];
    }
  }
  H.x_c = std::vector<double>(rt ? m : 0);
  H.resp_c = std::vector<unsigned char>(m);
  H.node_c = std::vector<int32_t>(node_id ? m : 0);
  H.node_off = std::vector<int64_t>(node_id ? n_nodes + 1 : 0, 0);
  H.c2caller = std::vector<int64_t>(m);
  {
    int64_t k = 0;
    for (int32_t s = 0; s < ns; ++s)
      for (int64_t j = seg_start[s] + (by_runs ? 0 : 1); j < seg_start[s + 1]; ++j, ++k) {
        const int64_t src = idx[j];
        if (rt) H.x_c[k] = rt[src];
        H.resp_c[k] = (unsigned char)response[src];
        H.c2caller[k] = src;
        if (node_id) {
          H.node_c[k] = node_id[src];
          H.node_off[node_id[src] + 1]++;
        }
      }
  }
  for (int32_t j = 0; node_id && j < n_nodes; ++j) {
    H.node_max = std::max(H.node_max, H.node_off[j + 1]);
    H.node_off[j + 1] += H.node_off[j];
  }
  return H;
}

// (2.718281828459**alpha) / (1 + 2.718281828459**alpha), libm pow (wfpt.pyx:123-125)
double rl_rate(double alpha) {
  constexpr double kRlBase = 2.718281828459;  // the reference's literal (wfpt.pyx:123)
  const double e = std::pow(kRlBase, alpha);
  return e / (1 + e);
}

}  // namespace capi
}  // namespace wfpt

namespace {

// Lays the trials out (rl_layout_host) and uploads them (context locked by the
// caller). The dataset is not registered: a resident one is by its entry point.
int rl_build(wfpt_ctx* c, const double* rt, const int64_t* response, const double* feedback,
             const int64_t* split_by, int64_t n, const int32_t* node_id, int32_t n_nodes,
             bool by_runs, wfpt_rl_ds** out) {
  RlHostLayout H = rl_layout_host(rt, response, feedback, split_by, n, node_id, n_nodes, by_runs);
  if (H.rc) return fail(H.rc, H.msg);
  auto* d = new wfpt_rl_ds();
  d->n = n;
  d->m = H.m;
  d->n_seg = H.n_seg;
  d->n_nodes = node_id ? n_nodes : 0;
  d->has_rt = rt != nullptr;
  d->by_runs = by_runs;
  d->node_max = H.node_max;
  hipError_t e = hipSuccess;
  auto up = [&](auto& dst, const auto& v, bool wanted = true) {
    if (wanted && e == hipSuccess) e = upload_vec(dst, v);
  };
  up(d->x_c, H.x_c), up(d->lane_start, H.lane_start), up(d->lane_out, H.lane_out);
  up(d->lane_len, H.lane_len), up(d->lane_node, H.lane_node, node_id), up(d->step_off, H.step_off);
  up(d->resp_t, H.resp_t), up(d->fb_t, H.fb_t), up(d->caller, H.caller, !by_runs);
  up(d->resp_c, H.resp_c), up(d->node_c, H.node_c, node_id), up(d->node_off, H.node_off, node_id);
  if (e != hipSuccess) {
    delete d;  // frees what was uploaded (the context's device is current)
    return fail(WFPT_ERR_HIP, std::string("RL dataset upload: ") + hipGetErrorString(e));
  }
  d->c2caller = std::move(H.c2caller);
  d->node_off_host = std::move(H.node_off);
  *out = d;
  return WFPT_OK;
}

wfpt::RlLayout rl_layout(const wfpt_rl_ds* d) {
  wfpt::RlLayout L;
  L.n_seg = d->n_seg;
  L.lane_start = d->lane_start.p;
  L.lane_out = d->lane_out.p;
  L.lane_len = d->lane_len.p;
  L.lane_node = d->lane_node.p;
  L.step_off = d->step_off.p;
  L.resp_t = d->resp_t.p;
  L.fb_t = d->fb_t.p;
  L.caller = d->caller.p;
  L.score_first = d->by_runs ? 1 : 0;
  return L;
}

// The scan of one call: drifts into c->rl.drift (compact) and, for an _ex
// call, c->rl.drift_in (every trial, the caller's order). Opens the call's
// profile bracket.
int rl_scan(wfpt_ctx* c, const wfpt_rl_ds* d, const wfpt::RlRow& one, const wfpt::RlRow* rows,
            const double* vmul, const double* rate, bool want_drift, int32_t n_tables = 0) {
  const int64_t T = std::max<int32_t>(n_tables, 1);
  HIP_TRY(c->rl.drift.reserve(std::max<int64_t>(T * d->m, 1)));
  const bool separate = want_drift && !d->by_runs;  // by_runs: compact == the caller's order
  if (separate) HIP_TRY(c->rl.drift_in.reserve(std::max<int64_t>(T * d->n, 1)));
  if (c->count) HIP_TRY(hipMemsetAsync(c->evals.p, 0, sizeof(unsigned long long), c->stream));
  if (c->profile) HIP_TRY(hipEventRecord(c->ev0, c->stream));
  double* drift_in = separate ? c->rl.drift_in.p : nullptr;
  if (n_tables > 0)  // the multi-table node batch: rows holds n_tables x n_nodes rows
    wfpt::launch_rl_scan_multi(rl_layout(d), wfpt::RlTables{n_tables, d->n_nodes, d->m, d->n},
                               rows, c->rl.drift.p, drift_in, c->stream);
  else
    wfpt::launch_rl_scan(rl_layout(d), one, rows, vmul, rate, c->rl.drift.p, drift_in, c->stream);
  HIP_TRY(hipGetLastError());
  return WFPT_OK;
}


// The _ex outputs of a finished call, in the caller's order: out_trial (each
// scored trial's term from c->lp, 0.0 for an unscored first trial), out_drift;
// T tables of a multi-table call one after the other (n values each).
int rl_outputs(wfpt_ctx* c, const wfpt_rl_ds* d, double* out_trial, double* out_drift,
               int64_t T = 1) {
  if (out_trial && d->n > 0) {
    std::vector<double> h(std::max<int64_t>(T * d->m, 1));
    if (d->m > 0)
      HIP_TRY(hipMemcpy(h.data(), c->lp.p, T * d->m * sizeof(double), hipMemcpyDeviceToHost));
    std::fill(out_trial, out_trial + T * d->n, 0.0);
    for (int64_t t = 0; t < T; ++t)
      for (int64_t i = 0; i < d->m; ++i)
        out_trial[t * d->n + d->c2caller[i]] = h[t * d->m + i];
  }
  if (out_drift && d->n > 0)
    HIP_TRY(hipMemcpy(out_drift, d->by_runs ? c->rl.drift.p : c->rl.drift_in.p,
                      T * d->n * sizeof(double), hipMemcpyDeviceToHost));
  return WFPT_OK;
}

// Grows the dataset's replicated view to T tables: x_rep = x_c T times over,
// off_rep[t n_nodes + j] = t m + node_off[j] (the compact range of node j in
// table t; T n_nodes + 1 offsets). The stream is idle here: every call on the
// context ends in its completion wait.
int rl_replicate(wfpt_ctx* c, const wfpt_rl_ds* d, int32_t T) {
  if (T <= d->rep_tables) return WFPT_OK;
  const int64_t m = d->m, nn = d->n_nodes;
  d->rep_tables = 0;
  HIP_TRY(d->x_rep.reserve(std::max<int64_t>(T * m, 1)));
  HIP_TRY(d->off_rep.reserve(T * nn + 1));
  for (int64_t t = 0; t < T && m > 0; ++t)
    HIP_TRY(hipMemcpyAsync(d->x_rep.p + t * m, d->x_c.p, m * sizeof(double),
                           hipMemcpyDeviceToDevice, c->stream));
  d->off_rep_host.resize(T * nn + 1);
  for (int64_t t = 0; t < T; ++t)
    for (int64_t j = 0; j < nn; ++j) d->off_rep_host[t * nn + j] = t * m + d->node_off_host[j];
  d->off_rep_host[T * nn] = T * m;
  HIP_TRY(hipMemcpyAsync(d->off_rep.p, d->off_rep_host.data(), (T * nn + 1) * sizeof(int64_t),
                         hipMemcpyHostToDevice, c->stream));
  d->rep_tables = T;
  return WFPT_OK;
}

int rl_check_ds(wfpt_ctx* c, const wfpt_rl_ds* d, bool need_rt) {
  if (d->ctx != c) return fail(WFPT_ERR_ARG, "RL dataset belongs to another context");
  if (d->by_runs) return fail(WFPT_ERR_ARG, "RL dataset laid out for wiener_like_multi_rlddm");
  if (need_rt && !d->has_rt)
    return fail(WFPT_ERR_ARG, "RL dataset was created without RTs (choice-only model)");
  return WFPT_OK;
}

wfpt::RlRow rl_row(double q, double alpha, double pos_alpha, double v) {
  wfpt::RlRow R;
  R.q = q;
  R.alfa = rl_rate(alpha);
  R.pos_alfa = pos_alpha == 100.00 ? R.alfa : rl_rate(pos_alpha);  // wfpt.pyx:105-108
  R.v = v;
  return R;
}

// The multi-table node batch after its checks, the context locked: the sums of
// the T x n_nodes nodes into out_logp, every scored trial's term left in c->lp
// (table t's compact trial i at t m + i).
int rl_nodes_multi_locked(wfpt_ctx* c, const wfpt_rl_ds* d, const double* rl_tables,
                          const wfpt_params* tables, int32_t n_tables, const wfpt::Knobs& K,
                          double p_outlier, bool want_drift, double* out_logp) {
  const int32_t nn = d->n_nodes;
  const int64_t T = n_tables, G = T * nn, m = d->m;
  std::vector<wfpt::RlRow> rows(G);
  std::vector<wfpt::Params> par(G);
  for (int64_t j = 0; j < G; ++j) {
    rows[j] = rl_row(rl_tables[3 * j], rl_tables[3 * j + 1], rl_tables[3 * j + 2], tables[j].v);
    par[j] = to_params(&tables[j]);
  }
  // one copy each for all tables
  HIP_TRY(c->rl.rows.reserve(G));
  HIP_TRY(c->rl.par.reserve(G));
  HIP_TRY(hipMemcpyAsync(c->rl.rows.p, rows.data(), G * sizeof(wfpt::RlRow),
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->rl.par.p, par.data(), G * sizeof(wfpt::Params),
                         hipMemcpyHostToDevice, c->stream));
  if (int rc = rl_replicate(c, d, n_tables)) return rc;
  // The one-table call's sequence over T x the work: table t's scored trials
  // are trials [t m, (t + 1) m) of every per-trial array, its nodes groups
  // [t n_nodes, (t + 1) n_nodes) of score_runs. The scoring kernels work trial
  // by trial and the per-node sum counts its blocks from the node's first
  // trial, so no bit depends on where a table starts.
  constexpr int mask = 0x2e;  // sv, a, z, t per trial; sz and st scalars of the pass
  const int64_t tm = T * m;
  HIP_TRY(c->rl.arr.reserve(std::max<int64_t>(4 * tm, 1)));
  if (int rc = rl_scan(c, d, wfpt::RlRow{}, c->rl.rows.p, nullptr, nullptr, want_drift,
                       n_tables))
    return rc;
  wfpt::launch_rl_fill_multi(d->node_c.p, wfpt::RlTables{n_tables, nn, m, d->n}, c->rl.par.p, mask,
                             c->rl.arr.p, c->stream);
  HIP_TRY(hipGetLastError());
  double* field[7] = {c->rl.drift.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int f = 1, slot = 0; f < 7; ++f)
    if (mask & (1 << f)) field[f] = c->rl.arr.p + (int64_t)slot++ * tm;
  if (int rc = score_runs(c, d->x_rep.p, field, tables, (int32_t)G, d->off_rep_host.data(),
                          d->off_rep.p, c->rl.npart, K, p_outlier, out_logp))
    return rc;
  return WFPT_OK;
}

}  // namespace

extern "C" {

int wfpt_rl_dataset_create(wfpt_ctx* c, const double* rt, const int64_t* response,
                           const double* feedback, const int64_t* split_by, int64_t n,
                           const int32_t* node_id, int32_t n_nodes, wfpt_rl_ds** out) {
  if (!c || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (n < 0) return fail(WFPT_ERR_ARG, "n < 0");
  if (n > 0 && (!response || !feedback || !split_by))
    return fail(WFPT_ERR_ARG, "null response / feedback / split_by array");
  if (node_id && n_nodes <= 0) return fail(WFPT_ERR_ARG, "node ids need n_nodes > 0");
  WFPT_RANGE("wfpt_rl_dataset_create");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  wfpt_rl_ds* d = nullptr;
  if (int rc = rl_build(c, rt, response, feedback, split_by, n, node_id, n_nodes, false, &d))
    return rc;
  ds_register(c, d);
  *out = d;
  return WFPT_OK;
}

void wfpt_rl_dataset_destroy(wfpt_rl_ds* d) { ds_destroy(d); }

int wfpt_wiener_like_rlddm_ex(wfpt_ctx* c, const wfpt_rl_ds* d, double q, double alpha,
                              double pos_alpha, const wfpt_params* p, const wfpt_knobs* k,
                              double* out, double* out_trial, double* out_drift) {
  if (!c || !d || !p || !k || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (int rc = rl_check_ds(c, d, true)) return rc;
  if (!p_outlier_in_range(p->p_outlier)) {  // wfpt.pyx:102-103
    *out = -INFINITY;
    return WFPT_OK;
  }
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_rlddm");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (int rc = rl_scan(c, d, rl_row(q, alpha, pos_alpha, p->v), nullptr, nullptr, nullptr,
                       out_drift != nullptr))
    return rc;
  double* dptr[7] = {c->rl.drift.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const double scal[7] = {0.0, p->sv, p->a, p->z, p->sz, p->t, p->st};
  if (int rc = multi_score(c, d->x_c.p, d->m, dptr, scal, K, p->p_outlier)) return rc;
  if (int rc = multi_finish(c, d->m, out)) return rc;
  return rl_outputs(c, d, out_trial, out_drift);
}

int wfpt_wiener_like_rlddm(wfpt_ctx* c, const wfpt_rl_ds* d, double q, double alpha,
                           double pos_alpha, const wfpt_params* p, const wfpt_knobs* k,
                           double* out) {
  return wfpt_wiener_like_rlddm_ex(c, d, q, alpha, pos_alpha, p, k, out, nullptr, nullptr);
}

int wfpt_wiener_like_rl_ex(wfpt_ctx* c, const wfpt_rl_ds* d, double q, double alpha,
                           double pos_alpha, double v, double z, double p_outlier,
                           double w_outlier, double* out, double* out_trial,
                           double* out_drift) {
  if (!c || !d || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (int rc = rl_check_ds(c, d, false)) return rc;
  if (!p_outlier_in_range(p_outlier)) {  // wfpt.pyx:178-179
    *out = -INFINITY;
    return WFPT_OK;
  }
  WFPT_RANGE("wfpt_wiener_like_rl");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (int rc = rl_scan(c, d, rl_row(q, alpha, pos_alpha, v), nullptr, nullptr, nullptr,
                       out_drift != nullptr))
    return rc;
  const int64_t nb = wfpt::blocks_for(d->m);
  HIP_TRY(c->part.reserve(std::max<int64_t>(nb, 1)));
  HIP_TRY(c->zero.reserve(std::max<int64_t>(nb, 1)));
  HIP_TRY(c->lp.reserve(std::max<int64_t>(d->m, 1)));
  wfpt::launch_rl_choice(c->rl.drift.p, d->resp_c.p, d->m, z, p_outlier, w_outlier * p_outlier,
                         c->lp.p, c->part.p, c->zero.p, c->stream);
  HIP_TRY(hipGetLastError());
  if (int rc = multi_finish(c, d->m, out)) return rc;
  return rl_outputs(c, d, out_trial, out_drift);
}

int wfpt_wiener_like_rl(wfpt_ctx* c, const wfpt_rl_ds* d, double q, double alpha,
                        double pos_alpha, double v, double z, double p_outlier, double w_outlier,
                        double* out) {
  return wfpt_wiener_like_rl_ex(c, d, q, alpha, pos_alpha, v, z, p_outlier, w_outlier, out,
                                nullptr, nullptr);
}

int wfpt_wiener_like_multi_rlddm_ex(wfpt_ctx* c, const double* x, const int64_t* response,
                                    const double* feedback, const int64_t* split_by, int64_t n,
                                    double q, const double* const arrays[8],
                                    const double scalars[8], const wfpt_knobs* k,
                                    double p_outlier, double* out, double* out_trial,
                                    double* out_drift) {
  if (!c || !arrays || !scalars || !k || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (n < 0) return fail(WFPT_ERR_ARG, "n < 0");
  if (n > 0 && (!x || !response || !feedback || !split_by))
    return fail(WFPT_ERR_ARG, "null x / response / feedback / split_by array");
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_multi_rlddm");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  wfpt_rl_ds* d = nullptr;
  if (int rc = rl_build(c, x, response, feedback, split_by, n, nullptr, 0, true, &d)) return rc;
  // per-trial alpha -> per-trial learning rates (wfpt.pyx:317), on the host
  std::vector<double> rate(arrays[7] ? n : 0);
  for (int64_t i = 0; i < (int64_t)rate.size(); ++i) rate[i] = rl_rate(arrays[7][i]);
  auto run = [&]() -> int {
    double* dev[8];
    if (int rc = upload_multi_arrays(c, arrays, 8, n, rate.data(), dev)) return rc;
    wfpt::RlRow one;
    one.q = q;
    one.alfa = one.pos_alfa = arrays[7] ? 0.0 : rl_rate(scalars[7]);
    one.v = scalars[0];
    if (int rc = rl_scan(c, d, one, nullptr, dev[0], dev[7], out_drift != nullptr)) return rc;
    double* dptr[7] = {c->rl.drift.p, dev[1], dev[2], dev[3], dev[4], dev[5], dev[6]};
    if (int rc = multi_score(c, d->x_c.p, n, dptr, scalars, K, p_outlier)) return rc;
    if (int rc = multi_finish(c, n, out)) return rc;
    return rl_outputs(c, d, out_trial, out_drift);
  };
  const int rc = run();
  if (rc != WFPT_OK) (void)hipStreamSynchronize(c->stream);  // nothing may still read d
  delete d;
  return rc;
}

int wfpt_wiener_like_multi_rlddm(wfpt_ctx* c, const double* x, const int64_t* response,
                                 const double* feedback, const int64_t* split_by, int64_t n,
                                 double q, const double* const arrays[8], const double scalars[8],
                                 const wfpt_knobs* k, double p_outlier, double* out) {
  return wfpt_wiener_like_multi_rlddm_ex(c, x, response, feedback, split_by, n, q, arrays,
                                         scalars, k, p_outlier, out, nullptr, nullptr);
}

int wfpt_wiener_like_rlddm_nodes_ex(wfpt_ctx* c, const wfpt_rl_ds* d, const double* rl_rows,
                                    const wfpt_params* per_node, const wfpt_knobs* k,
                                    double* out_logp, double* out_trial, double* out_drift) {
  if (!c || !d || !rl_rows || !per_node || !k || !out_logp)
    return fail(WFPT_ERR_ARG, "null pointer");
  if (int rc = rl_check_ds(c, d, true)) return rc;
  const int32_t nn = d->n_nodes;
  if (nn <= 0) return fail(WFPT_ERR_ARG, "RL dataset was created without node ids");
  if (d->node_max > wfpt::kRlNodeMax)
    return fail(WFPT_ERR_UNSUPPORTED, "a node holds more scored trials than the per-node sum takes");
  for (int32_t j = 1; j < nn; ++j)  // the per-trial-parameter pass takes one p_outlier
    if (per_node[j].p_outlier != per_node[0].p_outlier)
      return fail(WFPT_ERR_UNSUPPORTED, "the RL node batch needs one p_outlier for all nodes");
  const double p_outlier = per_node[0].p_outlier;
  if (!p_outlier_in_range(p_outlier)) {  // wfpt.pyx:102-103, every node
    for (int32_t j = 0; j < nn; ++j) out_logp[j] = -INFINITY;
    return WFPT_OK;
  }
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_rlddm_nodes");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  std::vector<wfpt::RlRow> rows(nn);
  std::vector<wfpt::Params> par(nn);
  for (int32_t j = 0; j < nn; ++j) {
    rows[j] = rl_row(rl_rows[3 * j], rl_rows[3 * j + 1], rl_rows[3 * j + 2], per_node[j].v);
    par[j] = to_params(&per_node[j]);
  }
  HIP_TRY(c->rl.rows.reserve(nn));
  HIP_TRY(c->rl.par.reserve(nn));
  HIP_TRY(hipMemcpyAsync(c->rl.rows.p, rows.data(), nn * sizeof(wfpt::RlRow),
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->rl.par.p, par.data(), nn * sizeof(wfpt::Params),
                         hipMemcpyHostToDevice, c->stream));
  const int64_t m = d->m;
  // sv, a, z and t per trial (rl_fill_kernel); sz and st stay scalars, so the
  // scoring pass is the one the single-node call takes (the level-0 pass for
  // the adaptive / direct families) and gives the same bits per trial: one
  // launch when the nodes share sz and st (HDDM's default: group-only), else
  // one per run of consecutive nodes that do
  constexpr int mask = 0x2e;
  HIP_TRY(c->rl.arr.reserve(std::max<int64_t>(4 * m, 1)));
  if (int rc = rl_scan(c, d, wfpt::RlRow{}, c->rl.rows.p, nullptr, nullptr, out_drift != nullptr))
    return rc;
  wfpt::launch_rl_fill(d->node_c.p, m, c->rl.par.p, mask, c->rl.arr.p, c->stream);
  HIP_TRY(hipGetLastError());
  double* field[7] = {c->rl.drift.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int f = 1, slot = 0; f < 7; ++f)
    if (mask & (1 << f)) field[f] = c->rl.arr.p + (int64_t)slot++ * m;
  if (int rc = score_runs(c, d->x_c.p, field, per_node, nn, d->node_off_host.data(),
                          d->node_off.p, c->rl.npart, K, p_outlier, out_logp))
    return rc;
  return rl_outputs(c, d, out_trial, out_drift);
}

int wfpt_wiener_like_rlddm_nodes(wfpt_ctx* c, const wfpt_rl_ds* d, const double* rl_rows,
                                 const wfpt_params* per_node, const wfpt_knobs* k,
                                 double* out_logp) {
  return wfpt_wiener_like_rlddm_nodes_ex(c, d, rl_rows, per_node, k, out_logp, nullptr, nullptr);
}

int wfpt_wiener_like_rlddm_nodes_multi_ex(wfpt_ctx* c, const wfpt_rl_ds* d,
                                          const double* rl_tables, const wfpt_params* tables,
                                          int32_t n_tables, const wfpt_knobs* k, double* out_logp,
                                          double* out_trial, double* out_drift) {
  if (!c || !d || !rl_tables || !tables || !k || !out_logp)
    return fail(WFPT_ERR_ARG, "null pointer");
  if (n_tables < 1) return fail(WFPT_ERR_ARG, "n_tables < 1");
  if (int rc = rl_check_ds(c, d, true)) return rc;
  const int32_t nn = d->n_nodes;
  if (nn <= 0) return fail(WFPT_ERR_ARG, "RL dataset was created without node ids");
  if (d->node_max > wfpt::kRlNodeMax)
    return fail(WFPT_ERR_UNSUPPORTED, "a node holds more scored trials than the per-node sum takes");
  // the scan's lanes, the rows and the scoring pass's deferred-record count are ints
  const int64_t T = n_tables, G = T * nn, m = d->m;
  if (T * d->n_seg > INT32_MAX || T * m > INT32_MAX || G > INT32_MAX)
    return fail(WFPT_ERR_UNSUPPORTED,
                "n_tables x segments, scored trials or nodes exceeds the kernels' index range");
  for (int64_t j = 1; j < G; ++j)  // the per-trial-parameter pass takes one p_outlier
    if (tables[j].p_outlier != tables[0].p_outlier)
      return fail(WFPT_ERR_UNSUPPORTED,
                  "the RL node batch needs one p_outlier for all nodes of all tables");
  const double p_outlier = tables[0].p_outlier;
  if (!p_outlier_in_range(p_outlier)) {  // wfpt.pyx:102-103, every node of every table
    for (int64_t j = 0; j < G; ++j) out_logp[j] = -INFINITY;
    return WFPT_OK;
  }
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_rlddm_nodes_multi");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (int rc = rl_nodes_multi_locked(c, d, rl_tables, tables, n_tables, K, p_outlier,
                                     out_drift != nullptr, out_logp))
    return rc;
  return rl_outputs(c, d, out_trial, out_drift, T);
}

int wfpt_pointwise_rlddm_nodes(wfpt_ctx* c, const wfpt_rl_ds* d, const double* rl_tables,
                               const wfpt_params* tables, int64_t S, const wfpt_knobs* k,
                               int64_t max_workspace, double* out_sums, double* out_stats,
                               int64_t* out_index, int64_t* out_ninf_total) {
  if (!c || !d || !rl_tables || !tables || !k || !out_sums || !out_stats || !out_index ||
      !out_ninf_total)
    return fail(WFPT_ERR_ARG, "null pointer");
  if (S < 1) return fail(WFPT_ERR_ARG, "S < 1");
  if (int rc = rl_check_ds(c, d, true)) return rc;
  const int32_t nn = d->n_nodes;
  if (nn <= 0) return fail(WFPT_ERR_ARG, "RL dataset was created without node ids");
  if (d->node_max > wfpt::kRlNodeMax)
    return fail(WFPT_ERR_UNSUPPORTED, "a node holds more scored trials than the per-node sum takes");
  const int64_t m = d->m, G = S * nn;
  for (int64_t j = 1; j < G; ++j)  // the per-trial-parameter pass takes one p_outlier
    if (tables[j].p_outlier != tables[0].p_outlier)
      return fail(WFPT_ERR_UNSUPPORTED,
                  "the RL node batch needs one p_outlier for all nodes of all tables");
  const double p_outlier = tables[0].p_outlier;
  std::copy(d->c2caller.begin(), d->c2caller.end(), out_index);
  if (!p_outlier_in_range(p_outlier)) {  // wfpt.pyx:102-103, every node of every sweep
    for (int64_t j = 0; j < G; ++j) out_sums[j] = -INFINITY;
    pointwise_all_inf(m, S, out_stats, out_ninf_total);
    return WFPT_OK;
  }
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_pointwise_rlddm_nodes");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  // a tile is one multi-table batch: its lanes, rows and records are ints
  const int64_t widest = std::max<int64_t>({(int64_t)nn, m, (int64_t)d->n_seg});
  const int64_t tile = pointwise_tile(max_workspace, m, S, widest);
  if (int rc = pointwise_begin(c, m)) return rc;
  for (int64_t s0 = 0; s0 < S; s0 += tile) {
    const int32_t T = (int32_t)std::min<int64_t>(tile, S - s0);
    if (int rc = rl_nodes_multi_locked(c, d, rl_tables + 3 * s0 * nn, tables + s0 * nn, T, K,
                                       p_outlier, false, out_sums + s0 * nn))
      return rc;
    if (int rc = pointwise_add(c, c->lp.p, T)) return rc;
  }
  return pointwise_finish(c, S, nullptr, out_stats, out_ninf_total);
}

int wfpt_wiener_like_rlddm_nodes_multi(wfpt_ctx* c, const wfpt_rl_ds* d, const double* rl_tables,
                                       const wfpt_params* tables, int32_t n_tables,
                                       const wfpt_knobs* k, double* out_logp) {
  return wfpt_wiener_like_rlddm_nodes_multi_ex(c, d, rl_tables, tables, n_tables, k, out_logp,
                                               nullptr, nullptr);
}

}  // extern "C"
