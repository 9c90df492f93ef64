// capi_sim.cpp — the samplers of the C ABI (include/wfpt_amd.h): the batched
// inverse-CDF RT sampler and the diffusion-path simulator (sim_kernels.hip),
// the closed-loop RLDDM simulator (rl_sim_kernels.hip), and the per-row RT
// statistics (stats_kernels.hip) alone or fused onto any of them.
#include "capi_internal.hpp"
#include "sim_internal.h"
#include "stats_internal.h"

using namespace wfpt::capi;

int wfpt::capi::stats_check_q(const char* name, const double* q, int32_t nq, const double* out) {
  if (nq < 0 || nq > wfpt::kStatsMaxQ)
    return fail(WFPT_ERR_ARG, std::string(name) + ": nq outside 0..16");
  if ((nq > 0 && !q) || !out)
    return fail(WFPT_ERR_ARG, std::string(name) + ": null pointer (q / stats_out)");
  for (int32_t k = 0; k < nq; ++k)
    if (!(q[k] >= 0 && q[k] <= 100))
      return fail(WFPT_ERR_ARG, std::string(name) + ": percentile " + std::to_string(k) +
                                    " outside [0, 100]");
  return WFPT_OK;
}

namespace {

// The statistics a sampler call is asked for on top of its draws.
struct StatsReq {
  const double* q;
  int32_t nq;
  double* out;  // [R x (8 + 2 nq)]
};

// Which kernel scores which row, decided on the host before any device work:
// `list` holds the wave tier's rows, then the block tier's by LDS size, then
// the global tier's. A call whose rows all take the wave tier uploads no list.
struct StatsPlan {
  wfpt::StatsQ Q;
  std::vector<int32_t> list;
  int64_t n_wave = 0, n_global = 0;
  struct Group {
    int64_t P, first, count;
  };
  std::vector<Group> block;
  int64_t global_first = 0, global_P = 0;
  bool identity = false;
};

// off: R + 1 rising offsets. tier 0: by row length; 1 / 2 / 3 force the wave /
// block / global tier, and a row the forced tier cannot hold is WFPT_ERR_ARG.
int stats_plan(const char* name, const int64_t* off, int64_t R, const double* q, int32_t nq,
               int32_t tier, StatsPlan* S) {
  if (tier < 0 || tier > 3) return fail(WFPT_ERR_ARG, std::string(name) + ": tier outside 0..3");
  S->Q.nq = nq;
  for (int k = 0; k < wfpt::kStatsMaxQ; ++k) S->Q.q[k] = k < nq ? q[k] : 0.0;
  std::vector<int32_t> wave, global;
  std::vector<std::vector<int32_t>> block(16);  // by log2 of the padded length
  for (int64_t r = 0; r < R; ++r) {
    const int64_t n = off[r + 1] - off[r];
    const int t = tier ? tier : (n <= wfpt::kStatsWaveMax ? 1 : n <= wfpt::kStatsBlockMax ? 2 : 3);
    if ((t == 1 && n > wfpt::kStatsWaveMax) || (t == 2 && n > wfpt::kStatsBlockMax))
      return fail(WFPT_ERR_ARG, std::string(name) + ": row " + std::to_string(r) + " has " +
                                    std::to_string(n) + " draws, more than the forced tier " +
                                    std::to_string(t) + " holds");
    if (n >= (int64_t)1 << 36)
      return fail(WFPT_ERR_ARG, std::string(name) + ": a row of 2^36 draws or more");
    if (t == 1) wave.push_back((int32_t)r);
    else if (t == 3) global.push_back((int32_t)r);
    else {
      int lg = 1;
      while (((int64_t)1 << lg) < n) ++lg;
      block[lg].push_back((int32_t)r);
    }
    if (t == 3) S->global_P = std::max(S->global_P, wfpt::stats_pow2(n));
  }
  S->identity = (int64_t)wave.size() == R;
  S->n_wave = (int64_t)wave.size();
  S->list = std::move(wave);
  for (int lg = 1; lg < 16; ++lg) {
    if (block[lg].empty()) continue;
    S->block.push_back({(int64_t)1 << lg, (int64_t)S->list.size(), (int64_t)block[lg].size()});
    S->list.insert(S->list.end(), block[lg].begin(), block[lg].end());
  }
  S->global_first = (int64_t)S->list.size();
  S->n_global = (int64_t)global.size();
  S->list.insert(S->list.end(), global.begin(), global.end());
  return WFPT_OK;
}

// The statistics of rows [0, R) of the device draws d_rts (offsets on the
// device and on the host) into c->stats.out, then host_out, on the context's
// stream; returns after the stream has drained. The context is locked.
int stats_run(wfpt_ctx* c, const StatsPlan& S, const double* d_rts, const int64_t* d_off,
              const int64_t* off, int64_t R, double* host_out) {
  const int K = wfpt::stats_cols(S.Q.nq);
  HIP_TRY(c->stats.out.reserve((size_t)R * K));
  if (!S.identity) {
    HIP_TRY(c->stats.list.reserve(S.list.size()));
    HIP_TRY(hipMemcpyAsync(c->stats.list.p, S.list.data(), S.list.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, c->stream));
  }
  if (S.n_global > 0) HIP_TRY(c->stats.ws.reserve((size_t)S.global_P));
  if (c->profile)
    for (int k = 0; k < 2; ++k)
      if (!c->sim.ev[k]) HIP_TRY(hipEventCreate(&c->sim.ev[k]));
  wfpt::StatsCall C;
  C.rts = d_rts;
  C.off = d_off;
  C.out = c->stats.out.p;
  C.Q = S.Q;
  if (c->profile) HIP_TRY(hipEventRecord(c->sim.ev[0], c->stream));
  wfpt::launch_stats_wave(C, S.identity ? nullptr : c->stats.list.p, S.n_wave, c->stream);
  HIP_TRY(hipGetLastError());
  for (const StatsPlan::Group& g : S.block) {
    wfpt::launch_stats_block(C, c->stats.list.p + g.first, g.count, g.P, c->stream);
    HIP_TRY(hipGetLastError());
  }
  for (int64_t k = 0; k < S.n_global; ++k) {
    const int64_t r = S.list[S.global_first + k];
    wfpt::launch_stats_global(C, r, off[r], off[r + 1] - off[r], c->stats.ws.p, c->stream);
    HIP_TRY(hipGetLastError());
  }
  if (c->profile) {
    HIP_TRY(hipEventRecord(c->sim.ev[1], c->stream));
    HIP_TRY(hipEventSynchronize(c->sim.ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->sim.ev[0], c->sim.ev[1]));
    c->k_ms += ms;
    c->launches += 1;
  }
  HIP_TRY(hipMemcpyAsync(host_out, c->stats.out.p, (size_t)R * K * sizeof(double),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // a global-tier workspace grown past 256 MiB is not kept between calls
  if (c->stats.ws.cap * sizeof(double) > ((size_t)256 << 20)) c->stats.ws.release();
  return WFPT_OK;
}

// ---------------------------------------------------------------------------
// RT sampler (sim_kernels.hip; wfpt.pyx:323-354 for R parameter rows)

int gen_rts_nodes_impl(wfpt_ctx* c, const double* grid, int64_t G, const wfpt_params* rows,
                       int64_t R, const int64_t* counts, const double* u_choice,
                       const double* u_delay, uint64_t seed, int64_t workspace_bytes, double* out,
                       double* out_pdf, double* out_cdf, int64_t* out_idx, double* out_u_choice,
                       double* out_u_delay, const StatsReq* sr) {

  if (!grid || !rows || !counts) return fail(WFPT_ERR_ARG, "null pointer (grid / rows / counts)");
  if (G < 2) return fail(WFPT_ERR_ARG, "gen_rts_nodes: G < 2 (the grid needs two points)");
  if (R < 1) return fail(WFPT_ERR_ARG, "gen_rts_nodes: R < 1");
  if (R >= (int64_t)1 << 31) return fail(WFPT_ERR_ARG, "gen_rts_nodes: R must be < 2^31");
  if (workspace_bytes < 0) return fail(WFPT_ERR_ARG, "gen_rts_nodes: negative workspace_bytes");
  std::vector<int64_t> off;
  if (int rc = counts_to_offsets("gen_rts_nodes", counts, R, &off)) return rc;
  bool any_st = false;
  for (int64_t r = 0; r < R; ++r) any_st = any_st || rows[r].st != 0;
  const int64_t total = off[R];
  if ((u_delay && !u_choice) || (u_choice && !u_delay && any_st))
    return fail(WFPT_ERR_ARG,
                "gen_rts_nodes: u_choice and u_delay go together when a row has st != 0");
  if (!out && total > 0 && !sr) return fail(WFPT_ERR_ARG, "null pointer (out)");
  StatsPlan plan;
  if (sr) {
    if (int rc = stats_check_q("gen_rts_nodes_stats", sr->q, sr->nq, sr->out)) return rc;
    if (int rc = stats_plan("gen_rts_nodes_stats", off.data(), R, sr->q, sr->nq, 0, &plan))
      return rc;
  }
  if (!c) return fail(WFPT_ERR_ARG, "null pointer (context)");
  const int64_t m = G - 1;
  const int64_t ws = workspace_bytes > 0 ? workspace_bytes : (int64_t)1 << 30;
  // rows per tile: the workspace's, at most R, and few enough for one launch
  // of 256-point blocks (a grid's x dimension is below 2^31)
  int64_t rpt = std::max<int64_t>(1, ws / 8 / m);
  rpt = std::min(rpt, R);
  rpt = std::min(rpt, std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / ((m + 255) / 256)));
  rpt = std::min<int64_t>(rpt, (int64_t)1 << 30);
  WFPT_RANGE("wfpt_gen_rts_nodes");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  std::vector<wfpt::Params> par((size_t)R);
  for (int64_t r = 0; r < R; ++r) par[r] = to_params(&rows[r]);
  const bool want_u = out_u_choice || out_u_delay;
  HIP_TRY(c->sim.grid.reserve(G));
  HIP_TRY(c->sim.rows.reserve(R));
  HIP_TRY(c->sim.off.reserve(R + 1));
  HIP_TRY(c->sim.tot.reserve(R));
  HIP_TRY(c->sim.ws.reserve((size_t)wfpt::sim_ws_rows(rpt) * m));
  HIP_TRY(c->sim.out.reserve(std::max<int64_t>(total, 1)));
  // [0, total) the choice uniforms, [total, 2 total) the delay uniforms:
  // supplied ones going in, generated ones coming out of a debugging call
  if (u_choice || want_u) HIP_TRY(c->sim.u.reserve(std::max<int64_t>(2 * total, 1)));
  if (out_idx) HIP_TRY(c->sim.idx.reserve(std::max<int64_t>(total, 1)));
  HIP_TRY(hipMemcpyAsync(c->sim.grid.p, grid, G * sizeof(double), hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipMemcpyAsync(c->sim.rows.p, par.data(), R * sizeof(wfpt::Params),
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->sim.off.p, off.data(), (R + 1) * sizeof(int64_t),
                         hipMemcpyHostToDevice, c->stream));
  if (u_choice && total > 0) {
    HIP_TRY(hipMemcpyAsync(c->sim.u.p, u_choice, total * sizeof(double), hipMemcpyHostToDevice,
                           c->stream));
    if (u_delay)
      HIP_TRY(hipMemcpyAsync(c->sim.u.p + total, u_delay, total * sizeof(double),
                             hipMemcpyHostToDevice, c->stream));
  }
  if (c->profile)
    for (hipEvent_t& ev : c->sim.ev)
      if (!ev) HIP_TRY(hipEventCreate(&ev));
  if (int rc = begin_status(c)) return rc;
  wfpt::SimDraw D;
  D.off = c->sim.off.p;
  D.u_choice = u_choice ? c->sim.u.p : nullptr;
  D.u_delay = (u_choice && u_delay) ? c->sim.u.p + total : nullptr;
  D.seed = seed;
  D.out = c->sim.out.p;
  D.idx_out = out_idx ? c->sim.idx.p : nullptr;
  // the uniforms of a supplied-uniform call are the caller's own: returned
  // from the host arrays below
  D.uc_out = (want_u && !u_choice) ? c->sim.u.p : nullptr;
  D.ud_out = (want_u && !u_choice) ? c->sim.u.p + total : nullptr;
  for (int64_t r0 = 0; r0 < R; r0 += rpt) {
    wfpt::SimTile T;
    T.grid = c->sim.grid.p;
    T.m = m;
    T.rows = c->sim.rows.p;
    T.row0 = r0;
    T.nrows = (int32_t)std::min(rpt, R - r0);
    T.W = c->sim.ws.p;
    T.tot = c->sim.tot.p;
    const size_t tile_bytes = (size_t)T.nrows * m * sizeof(double);
    if (c->profile) HIP_TRY(hipEventRecord(c->sim.ev[0], c->stream));
    wfpt::launch_sim_pdf(T, c->status.p, c->stream);
    HIP_TRY(hipGetLastError());
    if (out_pdf)
      HIP_TRY(hipMemcpyAsync(out_pdf + r0 * m, T.W, tile_bytes, hipMemcpyDeviceToHost, c->stream));
    if (c->profile) HIP_TRY(hipEventRecord(c->sim.ev[1], c->stream));
    wfpt::launch_sim_scan(T, c->stream);
    HIP_TRY(hipGetLastError());
    if (c->profile) HIP_TRY(hipEventRecord(c->sim.ev[2], c->stream));
    wfpt::launch_sim_norm(T, c->stream);
    HIP_TRY(hipGetLastError());
    if (out_cdf)
      HIP_TRY(hipMemcpyAsync(out_cdf + r0 * m, T.W, tile_bytes, hipMemcpyDeviceToHost, c->stream));
    if (c->profile) HIP_TRY(hipEventRecord(c->sim.ev[3], c->stream));
    wfpt::launch_sim_draw(T, D, off[r0], off[r0 + T.nrows] - off[r0], c->stream);
    HIP_TRY(hipGetLastError());
    if (c->profile) {
      HIP_TRY(hipEventRecord(c->sim.ev[4], c->stream));
      HIP_TRY(hipEventSynchronize(c->sim.ev[4]));
      for (int k = 0; k < 4; ++k) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->sim.ev[k], c->sim.ev[k + 1]));
        c->sim.ms[k] += ms;
        c->k_ms += ms;
      }
      c->launches += 4;
    }
  }
  std::vector<double> tot((size_t)R);
  HIP_TRY(hipMemcpyAsync(tot.data(), c->sim.tot.p, R * sizeof(double), hipMemcpyDeviceToHost,
                         c->stream));
  if (int rc = fetch_status(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  // a tile workspace grown past 256 MiB is not kept between calls
  if (c->sim.ws.cap * sizeof(double) > ((size_t)256 << 20)) c->sim.ws.release();
  if (int rc = check_status(c)) return rc;
  // wfpt.pyx:338 divides by the row's total: a total that is not finite and
  // positive (invalid parameters: all-zero densities; a == 0: NaN) has no CDF
  for (int64_t r = 0; r < R; ++r)
    if (!(tot[r] > 0) || !std::isfinite(tot[r]))
      return fail(WFPT_ERR_UNSUPPORTED, "gen_rts_nodes: row " + std::to_string(r) +
                                    " has no CDF (the sum of its grid densities is " +
                                    std::to_string(tot[r]) + "); no draws are returned");
  if (sr)
    if (int rc = stats_run(c, plan, c->sim.out.p, c->sim.off.p, off.data(), R, sr->out)) return rc;
  if (total > 0) {
    if (out) HIP_TRY(hipMemcpy(out, c->sim.out.p, total * sizeof(double), hipMemcpyDeviceToHost));
    if (out_idx)
      HIP_TRY(hipMemcpy(out_idx, c->sim.idx.p, total * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (out_u_choice) {
      if (u_choice) std::memcpy(out_u_choice, u_choice, total * sizeof(double));
      else HIP_TRY(hipMemcpy(out_u_choice, c->sim.u.p, total * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (out_u_delay) {
      if (u_choice && u_delay) std::memcpy(out_u_delay, u_delay, total * sizeof(double));
      else if (u_choice) std::memset(out_u_delay, 0, total * sizeof(double));
      else
        HIP_TRY(hipMemcpy(out_u_delay, c->sim.u.p + total, total * sizeof(double),
                          hipMemcpyDeviceToHost));
    }
  }
  return WFPT_OK;
}

// ---------------------------------------------------------------------------
// Diffusion-path simulator (sim_drift_kernel; hddm/generate.py:208-319)

// What a walk needs of a parameter row (generate.py:245-253: the start point
// lies between the boundaries).
bool walk_row_ok(const wfpt_params& P) {
  const bool finite = std::isfinite(P.v) && std::isfinite(P.sv) && std::isfinite(P.a) &&
                      std::isfinite(P.z) && std::isfinite(P.sz) && std::isfinite(P.t) &&
                      std::isfinite(P.st);
  return finite && P.a > 0 && !(P.z - P.sz / 2. < 0) && !(P.z + P.sz / 2. > 1);
}

int gen_rts_drift_nodes_impl(wfpt_ctx* c, const wfpt_params* rows, int64_t R, const double* sw,
                             const int64_t* counts, double dt, double intra_sv,
                             int64_t max_steps, uint64_t seed, int64_t row0, int32_t wave_draws,
                             double* out, int64_t* n_unfinished, double* out_y0,
                             double* out_delay, double* out_drift, double* out_drift_switch,
                             int64_t* out_n_steps, int64_t* out_wave_steps, const StatsReq* sr) {
  if (!rows || !counts || !n_unfinished)
    return fail(WFPT_ERR_ARG, "null pointer (rows / counts / n_unfinished)");
  if (R < 1) return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: R < 1");
  if (R >= (int64_t)1 << 31) return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: R must be < 2^31");
  if (row0 < 0 || row0 >= (int64_t)1 << 31)
    return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: row0 outside [0, 2^31)");
  if (!(dt > 0) || !std::isfinite(dt)) return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: dt <= 0");
  if (!(intra_sv > 0) || !std::isfinite(intra_sv))
    return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: intra_sv <= 0");
  if (max_steps < 1 || max_steps > (int64_t)1 << 31)
    return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: max_steps outside [1, 2^31]");
  if (wave_draws < 0 || wave_draws % 64 != 0)
    return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: wave_draws must be a multiple of 64 (0: default)");
  if (out_wave_steps && wave_draws == 0)
    return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: out_wave_steps needs an explicit wave_draws");
  const double root = std::sqrt(dt);
  const double step = root * intra_sv, scale = root / intra_sv;  // generate.py:258, 279
  if (!(step > 0) || !std::isfinite(step) || !std::isfinite(scale))
    return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: sqrt(dt) * intra_sv is not a usable step");
  std::vector<int64_t> off;
  if (int rc = counts_to_offsets("gen_rts_drift_nodes", counts, R, &off)) return rc;
  const int64_t total = off[R];
  if (!out && total > 0 && !sr) return fail(WFPT_ERR_ARG, "null pointer (out)");
  StatsPlan plan;
  if (sr) {
    if (int rc = stats_check_q("gen_rts_drift_nodes_stats", sr->q, sr->nq, sr->out)) return rc;
    if (int rc = stats_plan("gen_rts_drift_nodes_stats", off.data(), R, sr->q, sr->nq, 0, &plan))
      return rc;
  }
  std::vector<wfpt::DriftRow> tab((size_t)R);
  for (int64_t r = 0; r < R; ++r) {
    const wfpt_params& P = rows[r];
    wfpt::DriftRow& Q = tab[r];
    Q = wfpt::DriftRow{P.v, P.sv, P.a, P.z, P.sz, P.t, P.st, 0.0, 0.0, wfpt::kDriftNoSwitch, 0u};
    if (sw) {
      const double nn = std::nearbyint(sw[3 * r + 2] / dt);  // int(round(t_switch / dt))
      if (!(nn >= 1))
        return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: t_switch / dt rounds below 1 in row " +
                                      std::to_string(r));
      Q.v_switch = sw[3 * r];
      Q.V_switch = sw[3 * r + 1];
      // a switch past the step bound is never reached
      Q.nn = nn < 4294967295.0 ? (uint32_t)nn : wfpt::kDriftNoSwitch - 1;
    }
  }
  if (!c) return fail(WFPT_ERR_ARG, "null pointer (context)");
  for (int64_t r = 0; r < R; ++r) {
    const wfpt::DriftRow& Q = tab[r];
    if (!walk_row_ok(rows[r]) || !std::isfinite(Q.v_switch) || !std::isfinite(Q.V_switch))
      return fail(WFPT_ERR_UNSUPPORTED,
                  "gen_rts_drift_nodes: row " + std::to_string(r) +
                      " cannot be simulated (a non-finite parameter, a <= 0, or a start "
                      "point outside [0, 1]); no draws are returned");
  }
  // Draws per wave: one per lane until that gives every SIMD four waves
  // (1024 SIMDs), then up to 16 per lane, taken in turn as lanes finish
  // (fewer, longer waves idle less but must still fill the chip).
  const int64_t wd = wave_draws > 0 ? wave_draws
                                    : 64 * std::min<int64_t>(16, std::max<int64_t>(1, total / (64 * 4096)));
  const int64_t waves = (total + wd - 1) / wd;
  if (waves >= (int64_t)1 << 31)
    return fail(WFPT_ERR_ARG, "gen_rts_drift_nodes: too many draws for one call");
  *n_unfinished = 0;
  if (total == 0 && !sr) return WFPT_OK;
  WFPT_RANGE("wfpt_gen_rts_drift_nodes");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const bool dbg = out_y0 || out_delay || out_drift || out_drift_switch;
  HIP_TRY(c->sim.drift_rows.reserve(R));
  HIP_TRY(c->sim.off.reserve(R + 1));
  HIP_TRY(c->sim.out.reserve(total));
  if (dbg) HIP_TRY(c->sim.u.reserve(4 * total));
  if (out_n_steps || out_wave_steps) HIP_TRY(c->sim.idx.reserve(total + waves));
  HIP_TRY(hipMemcpyAsync(c->sim.drift_rows.p, tab.data(), R * sizeof(wfpt::DriftRow),
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->sim.off.p, off.data(), (R + 1) * sizeof(int64_t),
                         hipMemcpyHostToDevice, c->stream));
  if (c->profile)
    for (int k = 0; k < 2; ++k)
      if (!c->sim.ev[k]) HIP_TRY(hipEventCreate(&c->sim.ev[k]));
  wfpt::DriftCall C;
  C.rows = c->sim.drift_rows.p;
  C.off = c->sim.off.p;
  C.R = R;
  C.row0 = row0;
  C.total = total;
  C.dt = dt;
  C.step = step;
  C.scale = scale;
  C.max_steps = (uint32_t)max_steps;
  C.wave_draws = (int32_t)wd;
  C.seed = seed;
  C.out = c->sim.out.p;
  C.y0 = out_y0 ? c->sim.u.p : nullptr;
  C.delay = out_delay ? c->sim.u.p + total : nullptr;
  C.drift = out_drift ? c->sim.u.p + 2 * total : nullptr;
  C.drift_switch = out_drift_switch ? c->sim.u.p + 3 * total : nullptr;
  C.n_steps = out_n_steps ? c->sim.idx.p : nullptr;
  C.wave_steps = out_wave_steps ? c->sim.idx.p + total : nullptr;
  if (c->profile) HIP_TRY(hipEventRecord(c->sim.ev[0], c->stream));
  wfpt::launch_sim_drift(C, c->stream);
  HIP_TRY(hipGetLastError());
  if (c->profile) {
    HIP_TRY(hipEventRecord(c->sim.ev[1], c->stream));
    HIP_TRY(hipEventSynchronize(c->sim.ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->sim.ev[0], c->sim.ev[1]));
    c->k_ms += ms;
    c->launches += 1;
  }
  if (out && total > 0)
    HIP_TRY(hipMemcpyAsync(out, c->sim.out.p, total * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
  const std::pair<double*, const double*> copies[] = {
      {out_y0, C.y0}, {out_delay, C.delay}, {out_drift, C.drift},
      {out_drift_switch, C.drift_switch}};
  for (const auto& cp : copies)
    if (cp.first)
      HIP_TRY(hipMemcpyAsync(cp.first, cp.second, total * sizeof(double), hipMemcpyDeviceToHost,
                             c->stream));
  if (out_n_steps)
    HIP_TRY(hipMemcpyAsync(out_n_steps, C.n_steps, total * sizeof(int64_t),
                           hipMemcpyDeviceToHost, c->stream));
  if (out_wave_steps)
    HIP_TRY(hipMemcpyAsync(out_wave_steps, C.wave_steps, waves * sizeof(int64_t),
                           hipMemcpyDeviceToHost, c->stream));
  if (sr) {
    if (int rc = stats_run(c, plan, c->sim.out.p, c->sim.off.p, off.data(), R, sr->out)) return rc;
  } else {
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  unsigned long long nan_dev = 0;
  if (!out && total > 0) {  // the draws stay on the device: their NaNs are counted there
    HIP_TRY(c->stats.count.reserve(1));
    HIP_TRY(hipMemsetAsync(c->stats.count.p, 0, sizeof(unsigned long long), c->stream));
    wfpt::launch_stats_count_nan(c->sim.out.p, total, c->stats.count.p, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&nan_dev, c->stats.count.p, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  int64_t nan = (int64_t)nan_dev;  // only a draw that ran out of steps is NaN
  if (out)
    for (int64_t i = 0; i < total; ++i) nan += std::isnan(out[i]) ? 1 : 0;
  *n_unfinished = nan;
  return WFPT_OK;
}

// ---------------------------------------------------------------------------
// Closed-loop RLDDM simulator (rl_sim_kernel; hddm/generate.py:430-516, 608-661)

struct RlSimDebug {
  double *feedback, *q_up, *q_low, *sim_drift, *drift, *y0, *delay;
  int64_t *n_steps, *wave_steps;
};
// The statistics rows of a fused call: groups of consecutive sequence rows.
struct RlSimGroups {
  const int64_t* off;
  int64_t n;
};

int gen_rlddm_rows_impl(wfpt_ctx* c, const wfpt_params* rows, const double* rl_rows, int64_t R,
                        const int64_t* counts, const wfpt_rl_source* src, double dt,
                        double intra_sv, int64_t max_steps, uint64_t seed, int64_t row0,
                        int32_t wave_rows, double* out, int64_t* n_unfinished,
                        const RlSimDebug& D, const RlSimGroups* G, const StatsReq* sr) {
  const std::string name = "gen_rlddm_rows";
  if (!rows || !rl_rows || !counts || !src || !n_unfinished)
    return fail(WFPT_ERR_ARG, "null pointer (rows / rl_rows / counts / source / n_unfinished)");
  if (R < 1) return fail(WFPT_ERR_ARG, name + ": R < 1");
  if (row0 < 0 || R > ((int64_t)1 << 31) || row0 > ((int64_t)1 << 31) - R)
    return fail(WFPT_ERR_ARG, name + ": row0 + R must lie in [1, 2^31]");
  if (!(dt > 0) || !std::isfinite(dt)) return fail(WFPT_ERR_ARG, name + ": dt <= 0");
  if (!(intra_sv > 0) || !std::isfinite(intra_sv))
    return fail(WFPT_ERR_ARG, name + ": intra_sv <= 0");
  if (max_steps < 1 || max_steps > (int64_t)1 << 31)
    return fail(WFPT_ERR_ARG, name + ": max_steps outside [1, 2^31]");
  if (wave_rows < 0 || wave_rows % 64 != 0)
    return fail(WFPT_ERR_ARG, name + ": wave_rows must be a multiple of 64 (0: default)");
  if (D.wave_steps && wave_rows == 0)
    return fail(WFPT_ERR_ARG, name + ": out_wave_steps needs an explicit wave_rows");
  const double root = std::sqrt(dt);
  const double step = root * intra_sv, scale = root / intra_sv;  // generate.py:258, 279
  if (!(step > 0) || !std::isfinite(step) || !std::isfinite(scale))
    return fail(WFPT_ERR_ARG, name + ": sqrt(dt) * intra_sv is not a usable step");
  std::vector<int64_t> off;
  if (int rc = counts_to_offsets(name.c_str(), counts, R, &off)) return rc;
  const int64_t total = off[R];
  if (!out && total > 0 && !sr) return fail(WFPT_ERR_ARG, "null pointer (out)");
  // the reward source
  const bool has_rew = src->rew_up || src->rew_low, has_obs = src->obs_response || src->obs_feedback;
  if ((src->p ? 1 : 0) + (has_rew ? 1 : 0) + (has_obs ? 1 : 0) != 1)
    return fail(WFPT_ERR_ARG, name + ": exactly one reward source (p, rew_up / rew_low or "
                                     "obs_response / obs_feedback) must be given");
  if ((has_rew && (!src->rew_up || !src->rew_low)) ||
      (has_obs && (!src->obs_response || !src->obs_feedback)))
    return fail(WFPT_ERR_ARG, name + ": null pointer (one array of the reward source's pair)");
  const int32_t source = src->p ? wfpt::kRlSimBernoulli
                                : has_rew ? wfpt::kRlSimSupplied : wfpt::kRlSimObserved;
  if (source != wfpt::kRlSimBernoulli) {
    if (src->n < 0) return fail(WFPT_ERR_ARG, name + ": negative length of the source arrays");
    for (int64_t r = 0; r < R; ++r) {
      const int64_t s0 = src->start ? src->start[r] : off[r];
      if (s0 < 0 || s0 > src->n || counts[r] > src->n - s0)
        return fail(WFPT_ERR_ARG, name + ": row " + std::to_string(r) + " reads [" +
                                      std::to_string(s0) + ", +" + std::to_string(counts[r]) +
                                      ") of source arrays of " + std::to_string(src->n));
    }
  }
  std::vector<wfpt::RlSimRow> tab((size_t)R);
  for (int64_t r = 0; r < R; ++r) {
    const wfpt_params& P = rows[r];
    const double q = rl_rows[3 * r], alpha = rl_rows[3 * r + 1], pos_alpha = rl_rows[3 * r + 2];
    wfpt::RlSimRow& Q = tab[r];
    Q = wfpt::RlSimRow{P.v, P.sv, P.a, P.z, P.sz, P.t, P.st, q, 0.0, 0.0, 0.0, 0.0, 0};
    Q.alfa = rl_rate(alpha);
    Q.pos_alfa = pos_alpha == 100.00 ? Q.alfa : rl_rate(pos_alpha);  // wfpt.pyx:105-108
    if (std::isnan(q) || std::isnan(Q.alfa) || std::isnan(Q.pos_alfa))
      return fail(WFPT_ERR_ARG, name + ": NaN in RL row " + std::to_string(r) +
                                    " (q, or a learning rate that is NaN)");
    if (source == wfpt::kRlSimBernoulli) {
      Q.p_up = src->p[2 * r];
      Q.p_low = src->p[2 * r + 1];
      if (!(Q.p_up >= 0 && Q.p_up <= 1) || !(Q.p_low >= 0 && Q.p_low <= 1))
        return fail(WFPT_ERR_ARG, name + ": reward probability outside [0, 1] in row " +
                                      std::to_string(r));
    } else {
      Q.src = src->start ? src->start[r] : off[r];
    }
  }
  StatsPlan plan;
  std::vector<int64_t> goff;  // the groups' offsets into the trials
  if (sr) {
    if (int rc = stats_check_q("gen_rlddm_rows_stats", sr->q, sr->nq, sr->out)) return rc;
    if (!G || !G->off) return fail(WFPT_ERR_ARG, "null pointer (group_off)");
    if (G->n < 1 || G->n >= (int64_t)1 << 31)
      return fail(WFPT_ERR_ARG, name + "_stats: n_groups outside [1, 2^31)");
    if (G->off[0] != 0 || G->off[G->n] != R)
      return fail(WFPT_ERR_ARG, name + "_stats: group_off must run from 0 to R");
    goff.resize((size_t)G->n + 1);
    for (int64_t g = 0; g <= G->n; ++g) {
      if (g > 0 && G->off[g] < G->off[g - 1])
        return fail(WFPT_ERR_ARG, name + "_stats: group_off falls at group " + std::to_string(g - 1));
      if (G->off[g] < 0 || G->off[g] > R)
        return fail(WFPT_ERR_ARG, name + "_stats: group_off outside [0, R]");
      goff[g] = off[G->off[g]];
    }
    if (int rc = stats_plan("gen_rlddm_rows_stats", goff.data(), G->n, sr->q, sr->nq, 0, &plan))
      return rc;
  }
  for (int64_t r = 0; r < R; ++r)
    if (!walk_row_ok(rows[r]))
      return fail(WFPT_ERR_UNSUPPORTED,
                  name + ": row " + std::to_string(r) +
                      " cannot be simulated (a non-finite parameter, a <= 0, or a start "
                      "point outside [0, 1]); no draws are returned");
  if (!c) return fail(WFPT_ERR_ARG, "null pointer (context)");
  // Rows per wave: one per lane until that gives every SIMD four waves, then
  // up to 16 per lane, taken in turn as rows end (gen_rts_drift_nodes' rule).
  const int64_t wd = wave_rows > 0 ? wave_rows
                                   : 64 * std::min<int64_t>(16, std::max<int64_t>(1, R / (64 * 4096)));
  const int64_t waves = (R + wd - 1) / wd;
  *n_unfinished = 0;
  if (total == 0 && !sr) return WFPT_OK;
  WFPT_RANGE("wfpt_gen_rlddm_rows");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const bool dbg = D.feedback || D.q_up || D.q_low || D.sim_drift || D.drift || D.y0 || D.delay;
  const int64_t n_in = source == wfpt::kRlSimBernoulli ? 0 : src->n;
  const int64_t n_obs = source == wfpt::kRlSimObserved ? n_in : 0;
  HIP_TRY(c->sim.rl_rows.reserve(R));
  HIP_TRY(c->sim.off.reserve(R + 1));
  HIP_TRY(c->sim.out.reserve(std::max<int64_t>(total, 1)));
  HIP_TRY(c->sim.rl_in.reserve(std::max<int64_t>(2 * n_in, 1)));
  HIP_TRY(c->sim.rl_idx.reserve(n_obs + (int64_t)goff.size() + 1));
  if (dbg) HIP_TRY(c->sim.u.reserve(std::max<int64_t>(7 * total, 1)));
  if (D.n_steps || D.wave_steps) HIP_TRY(c->sim.idx.reserve(total + waves));
  HIP_TRY(hipMemcpyAsync(c->sim.rl_rows.p, tab.data(), R * sizeof(wfpt::RlSimRow),
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->sim.off.p, off.data(), (R + 1) * sizeof(int64_t),
                         hipMemcpyHostToDevice, c->stream));
  if (n_in > 0) {
    const double* first = source == wfpt::kRlSimSupplied ? src->rew_up : src->obs_feedback;
    HIP_TRY(hipMemcpyAsync(c->sim.rl_in.p, first, n_in * sizeof(double), hipMemcpyHostToDevice,
                           c->stream));
    if (source == wfpt::kRlSimSupplied)
      HIP_TRY(hipMemcpyAsync(c->sim.rl_in.p + n_in, src->rew_low, n_in * sizeof(double),
                             hipMemcpyHostToDevice, c->stream));
    else
      HIP_TRY(hipMemcpyAsync(c->sim.rl_idx.p, src->obs_response, n_in * sizeof(int64_t),
                             hipMemcpyHostToDevice, c->stream));
  }
  int64_t* const d_goff = c->sim.rl_idx.p + n_obs;
  if (sr)
    HIP_TRY(hipMemcpyAsync(d_goff, goff.data(), goff.size() * sizeof(int64_t),
                           hipMemcpyHostToDevice, c->stream));
  if (c->profile)
    for (int k = 0; k < 2; ++k)
      if (!c->sim.ev[k]) HIP_TRY(hipEventCreate(&c->sim.ev[k]));
  wfpt::RlSimCall C;
  C.rows = c->sim.rl_rows.p;
  C.off = c->sim.off.p;
  C.R = R;
  C.row0 = row0;
  C.dt = dt;
  C.step = step;
  C.scale = scale;
  C.max_steps = (uint32_t)max_steps;
  C.wave_rows = (int32_t)wd;
  C.seed = seed;
  C.source = source;
  C.in_up = c->sim.rl_in.p;
  C.in_low = c->sim.rl_in.p + n_in;
  C.obs_resp = c->sim.rl_idx.p;
  C.out = c->sim.out.p;
  double* const host_dbg[7] = {D.feedback, D.q_up, D.q_low, D.sim_drift, D.drift, D.y0, D.delay};
  double** const dev_dbg[7] = {&C.feedback, &C.q_up, &C.q_low, &C.sim_drift,
                               &C.drift,    &C.y0,   &C.delay};
  for (int k = 0; k < 7; ++k) *dev_dbg[k] = host_dbg[k] ? c->sim.u.p + k * total : nullptr;
  C.n_steps = D.n_steps ? c->sim.idx.p : nullptr;
  C.wave_steps = D.wave_steps ? c->sim.idx.p + total : nullptr;
  if (c->profile) HIP_TRY(hipEventRecord(c->sim.ev[0], c->stream));
  wfpt::launch_rl_sim(C, c->stream);
  HIP_TRY(hipGetLastError());
  if (c->profile) {
    HIP_TRY(hipEventRecord(c->sim.ev[1], c->stream));
    HIP_TRY(hipEventSynchronize(c->sim.ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->sim.ev[0], c->sim.ev[1]));
    c->k_ms += ms;
    c->launches += 1;
  }
  if (out && total > 0)
    HIP_TRY(hipMemcpyAsync(out, c->sim.out.p, total * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
  for (int k = 0; k < 7; ++k)
    if (host_dbg[k] && total > 0)
      HIP_TRY(hipMemcpyAsync(host_dbg[k], *dev_dbg[k], total * sizeof(double),
                             hipMemcpyDeviceToHost, c->stream));
  if (D.n_steps && total > 0)
    HIP_TRY(hipMemcpyAsync(D.n_steps, C.n_steps, total * sizeof(int64_t), hipMemcpyDeviceToHost,
                           c->stream));
  if (D.wave_steps)
    HIP_TRY(hipMemcpyAsync(D.wave_steps, C.wave_steps, waves * sizeof(int64_t),
                           hipMemcpyDeviceToHost, c->stream));
  if (sr) {
    if (int rc = stats_run(c, plan, c->sim.out.p, d_goff, goff.data(), G->n, sr->out)) return rc;
  } else {
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  unsigned long long nan_dev = 0;
  if (!out && total > 0) {  // the draws stay on the device: their NaNs are counted there
    HIP_TRY(c->stats.count.reserve(1));
    HIP_TRY(hipMemsetAsync(c->stats.count.p, 0, sizeof(unsigned long long), c->stream));
    wfpt::launch_stats_count_nan(c->sim.out.p, total, c->stats.count.p, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&nan_dev, c->stats.count.p, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  int64_t nan = (int64_t)nan_dev;  // only a cut trial and the rest of its row are NaN
  if (out)
    for (int64_t i = 0; i < total; ++i) nan += std::isnan(out[i]) ? 1 : 0;
  *n_unfinished = nan;
  return WFPT_OK;
}

}  // namespace

int wfpt::capi::stats_device_rows(wfpt_ctx* c, const char* name, const double* d_rts,
                                  const int64_t* off, int64_t R, const double* q, int32_t nq,
                                  double* host_out) {
  StatsPlan plan;
  if (int rc = stats_plan(name, off, R, q, nq, 0, &plan)) return rc;
  HIP_TRY(c->sim.off.reserve(R + 1));
  HIP_TRY(hipMemcpyAsync(c->sim.off.p, off, (R + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                         c->stream));
  return stats_run(c, plan, d_rts, c->sim.off.p, off, R, host_out);
}

extern "C" {

int wfpt_gen_rts_nodes_ex(wfpt_ctx* c, const double* grid, int64_t G, const wfpt_params* rows,
                          int64_t R, const int64_t* counts, const double* u_choice,
                          const double* u_delay, uint64_t seed, int64_t workspace_bytes,
                          double* out, double* out_pdf, double* out_cdf, int64_t* out_idx,
                          double* out_u_choice, double* out_u_delay) {
  return gen_rts_nodes_impl(c, grid, G, rows, R, counts, u_choice, u_delay, seed, workspace_bytes,
                            out, out_pdf, out_cdf, out_idx, out_u_choice, out_u_delay, nullptr);
}

int wfpt_gen_rts_nodes(wfpt_ctx* c, const double* grid, int64_t G, const wfpt_params* rows,
                       int64_t R, const int64_t* counts, const double* u_choice,
                       const double* u_delay, uint64_t seed, int64_t workspace_bytes,
                       double* out) {
  return gen_rts_nodes_impl(c, grid, G, rows, R, counts, u_choice, u_delay, seed, workspace_bytes,
                            out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int wfpt_gen_rts_nodes_stats(wfpt_ctx* c, const double* grid, int64_t G, const wfpt_params* rows,
                             int64_t R, const int64_t* counts, const double* u_choice,
                             const double* u_delay, uint64_t seed, int64_t workspace_bytes,
                             double* out, const double* q, int32_t nq, double* stats_out) {
  const StatsReq sr{q, nq, stats_out};
  return gen_rts_nodes_impl(c, grid, G, rows, R, counts, u_choice, u_delay, seed, workspace_bytes,
                            out, nullptr, nullptr, nullptr, nullptr, nullptr, &sr);
}

int wfpt_gen_rts_drift_nodes_ex(wfpt_ctx* c, const wfpt_params* rows, int64_t R,
                                const double* sw, const int64_t* counts, double dt,
                                double intra_sv, int64_t max_steps, uint64_t seed, int64_t row0,
                                int32_t wave_draws, double* out, int64_t* n_unfinished,
                                double* out_y0, double* out_delay, double* out_drift,
                                double* out_drift_switch, int64_t* out_n_steps,
                                int64_t* out_wave_steps) {
  return gen_rts_drift_nodes_impl(c, rows, R, sw, counts, dt, intra_sv, max_steps, seed, row0,
                                  wave_draws, out, n_unfinished, out_y0, out_delay, out_drift,
                                  out_drift_switch, out_n_steps, out_wave_steps, nullptr);
}

int wfpt_gen_rts_drift_nodes_stats(wfpt_ctx* c, const wfpt_params* rows, int64_t R,
                                   const double* sw, const int64_t* counts, double dt,
                                   double intra_sv, int64_t max_steps, uint64_t seed, double* out,
                                   int64_t* n_unfinished, const double* q, int32_t nq,
                                   double* stats_out) {
  const StatsReq sr{q, nq, stats_out};
  return gen_rts_drift_nodes_impl(c, rows, R, sw, counts, dt, intra_sv, max_steps, seed, 0, 0,
                                  out, n_unfinished, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, &sr);
}

// ---------------------------------------------------------------------------
// Per-row RT statistics of host draws (stats_kernels.hip; hddm/utils.py:241-265)

int wfpt_rt_stats_rows_ex(wfpt_ctx* c, const double* rts, const int64_t* off, int64_t R,
                          const double* q, int32_t nq, int32_t tier, double* out) {
  if (!off) return fail(WFPT_ERR_ARG, "null pointer (off)");
  if (R < 1) return fail(WFPT_ERR_ARG, "rt_stats_rows: R < 1");
  if (R >= (int64_t)1 << 31) return fail(WFPT_ERR_ARG, "rt_stats_rows: R must be < 2^31");
  if (int rc = stats_check_q("rt_stats_rows", q, nq, out)) return rc;
  if (off[0] != 0) return fail(WFPT_ERR_ARG, "rt_stats_rows: off[0] != 0");
  for (int64_t r = 0; r < R; ++r)
    if (off[r + 1] < off[r])
      return fail(WFPT_ERR_ARG, "rt_stats_rows: off falls at row " + std::to_string(r));
  const int64_t total = off[R];
  if (!rts && total > 0) return fail(WFPT_ERR_ARG, "null pointer (rts)");
  StatsPlan plan;
  if (int rc = stats_plan("rt_stats_rows", off, R, q, nq, tier, &plan)) return rc;
  if (!c) return fail(WFPT_ERR_ARG, "null pointer (context)");
  WFPT_RANGE("wfpt_rt_stats_rows");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HIP_TRY(c->sim.off.reserve(R + 1));
  HIP_TRY(c->sim.out.reserve(std::max<int64_t>(total, 1)));
  HIP_TRY(hipMemcpyAsync(c->sim.off.p, off, (R + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                         c->stream));
  if (total > 0)
    HIP_TRY(hipMemcpyAsync(c->sim.out.p, rts, total * sizeof(double), hipMemcpyHostToDevice,
                           c->stream));
  return stats_run(c, plan, c->sim.out.p, c->sim.off.p, off, R, out);
}

int wfpt_rt_stats_rows(wfpt_ctx* c, const double* rts, const int64_t* off, int64_t R,
                       const double* q, int32_t nq, double* out) {
  return wfpt_rt_stats_rows_ex(c, rts, off, R, q, nq, 0, out);
}

int wfpt_gen_rts_drift_nodes(wfpt_ctx* c, const wfpt_params* rows, int64_t R, const double* sw,
                             const int64_t* counts, double dt, double intra_sv,
                             int64_t max_steps, uint64_t seed, double* out,
                             int64_t* n_unfinished) {
  return wfpt_gen_rts_drift_nodes_ex(c, rows, R, sw, counts, dt, intra_sv, max_steps, seed, 0, 0,
                                     out, n_unfinished, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr);
}

int wfpt_gen_rlddm_rows_ex(wfpt_ctx* c, const wfpt_params* rows, const double* rl_rows, int64_t R,
                           const int64_t* counts, const wfpt_rl_source* source, double dt,
                           double intra_sv, int64_t max_steps, uint64_t seed, int64_t row0,
                           int32_t wave_rows, double* out, int64_t* n_unfinished,
                           double* out_feedback, double* out_q_up, double* out_q_low,
                           double* out_sim_drift, double* out_drift, double* out_y0,
                           double* out_delay, int64_t* out_n_steps, int64_t* out_wave_steps) {
  const RlSimDebug D{out_feedback, out_q_up, out_q_low, out_sim_drift, out_drift,
                     out_y0,       out_delay, out_n_steps, out_wave_steps};
  return gen_rlddm_rows_impl(c, rows, rl_rows, R, counts, source, dt, intra_sv, max_steps, seed,
                             row0, wave_rows, out, n_unfinished, D, nullptr, nullptr);
}

int wfpt_gen_rlddm_rows(wfpt_ctx* c, const wfpt_params* rows, const double* rl_rows, int64_t R,
                        const int64_t* counts, const wfpt_rl_source* source, double dt,
                        double intra_sv, int64_t max_steps, uint64_t seed, double* out,
                        int64_t* n_unfinished) {
  return gen_rlddm_rows_impl(c, rows, rl_rows, R, counts, source, dt, intra_sv, max_steps, seed, 0,
                             0, out, n_unfinished, RlSimDebug{}, nullptr, nullptr);
}

int wfpt_gen_rlddm_rows_stats(wfpt_ctx* c, const wfpt_params* rows, const double* rl_rows,
                              int64_t R, const int64_t* counts, const wfpt_rl_source* source,
                              double dt, double intra_sv, int64_t max_steps, uint64_t seed,
                              double* out, int64_t* n_unfinished, const int64_t* group_off,
                              int64_t n_groups, const double* q, int32_t nq, double* stats_out) {
  const StatsReq sr{q, nq, stats_out};
  const RlSimGroups G{group_off, n_groups};
  return gen_rlddm_rows_impl(c, rows, rl_rows, R, counts, source, dt, intra_sv, max_steps, seed, 0,
                             0, out, n_unfinished, RlSimDebug{}, &G, &sr);
}

int wfpt_profile_stages(wfpt_ctx* c, double stage_ms[4], int reset) {
  if (!c || !stage_ms) return fail(WFPT_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(c->mu);
  for (int k = 0; k < 4; ++k) {
    stage_ms[k] = c->sim.ms[k];
    if (reset) c->sim.ms[k] = 0.0;
  }
  return WFPT_OK;
}

}  // extern "C"
