// sim_internal.h — launcher interface between the C ABI (capi_*.cpp) and the
// RT sampler kernels (sim_kernels.hip, rl_sim_kernels.hip). Not part of the
// public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wfpt {
struct Params;


// One tile of the batched inverse-CDF sampler (wfpt.pyx:323-354; DESIGN.md
// §15): rows [row0, row0 + nrows) of the call's parameter table over the
// shared grid x[0 .. G). The workspace W holds one row of m = G - 1 doubles per
// tile row, row-major: first the densities at x[1 .. G), then (in place) their
// running sums, then the normalised CDF.
struct SimTile {
  const double* grid;  // [G] rising RT grid
  int64_t m;           // G - 1 points per row
  const Params* rows;  // [R] the call's rows (t and st enter only the delays)
  int64_t row0;        // global index of the tile's first row
  int32_t nrows;       // rows of the tile
  double* W;           // [sim_ws_rows(nrows) * m]
  double* tot;         // [R] each row's unnormalised total (global row index)
};

// W[r][i] = full_pdf(x[i + 1], v, sv, a, z, sz, 0, 0, 1e-4) with full_pdf's
// defaults n_st = n_sz = 2, adaptive, simps_err = 1e-3 (wfpt.pyx:335): one grid
// point per lane, one row per block. Depth / budget flags are OR-ed into status.
void launch_sim_pdf(const SimTile& T, int* status, hipStream_t s);

// W[r][i] <- W[r][0] + ... + W[r][i], added in index order from 0.0 as the
// reference's loop does (wfpt.pyx:333-336), one lane per row; tot[row0 + r] =
// the row's last sum. The scan moves whole blocks of 64 rows: W must hold
// sim_ws_rows(nrows) rows (the rows past nrows are scratch).
inline int64_t sim_ws_rows(int64_t nrows) { return (nrows + 63) / 64 * 64; }
void launch_sim_scan(const SimTile& T, hipStream_t s);

// W[r][i] <- W[r][i] / tot[row0 + r] (wfpt.pyx:338).
void launch_sim_norm(const SimTile& T, hipStream_t s);

// The draws of the tile's rows: draw j of global row r is element off[r] + j
// of out / u_choice / u_delay / idx_out (off: [R + 1] prefix sums of the
// counts). u_choice == null: both uniforms are Philox4x32-10 draws keyed by
// seed at counter (j lo, j hi, r, stream) (stream 0 choice, 1 delay), so the
// tiling cannot change them. u_delay may be null when no row has st != 0.
// uc_out / ud_out / idx_out (nullable): the uniforms used and the grid index.
struct SimDraw {
  const int64_t* off;
  const double* u_choice;
  const double* u_delay;
  uint64_t seed;
  double* out;
  int64_t* idx_out;
  double* uc_out;
  double* ud_out;
};
void launch_sim_draw(const SimTile& T, const SimDraw& D, int64_t first,
                     int64_t ndraws, hipStream_t s);

// The diffusion-path simulator (hddm/generate.py:208-319): one
// row of the call's table. nn: the first step that uses the switched drift
// (round(t_switch / dt)), kDriftNoSwitch for a row without a switch.
constexpr uint32_t kDriftNoSwitch = 0xFFFFFFFFu;
struct DriftRow {
  double v, sv, a, z, sz, t, st;
  double v_switch, V_switch;
  uint32_t nn;
  uint32_t pad;
};

// Draw j of global row row0 + r is element off[r] + j of out and of the
// (nullable) per-draw arrays. step = sqrt(dt) * intra_sv and scale = sqrt(dt) /
// intra_sv are formed on the host as generate.py:258,279 forms them. Every
// random number is a Philox4x32-10 word keyed by seed at counter (j lo, j hi,
// row0 + r, stream), so neither the launch shape nor wave_draws (draws handed
// to one wave, a multiple of 64) can change a value. A draw that has not
// crossed after max_steps steps is NaN.
struct DriftCall {
  const DriftRow* rows;  // [R]
  const int64_t* off;    // [R + 1] prefix sums of the counts
  int64_t R;
  int64_t row0;
  int64_t total;
  double dt, step, scale;
  uint32_t max_steps;    // 1 .. 2^31
  int32_t wave_draws;
  uint64_t seed;
  double* out;
  double* y0;            // start point
  double* delay;         // non-decision time of the draw
  double* drift;         // drift rate
  double* drift_switch;  // drift rate from step nn on (0 for a row without a switch)
  int64_t* n_steps;      // steps taken: the crossing step's index + 1, or max_steps
  int64_t* wave_steps;   // [ceil(total / wave_draws)] steps each wave's loop ran
};
void launch_sim_drift(const DriftCall& C, hipStream_t s);

// The closed-loop RLDDM simulator (rl_sim_kernels.hip; hddm/generate.py:430-516,
// 608-661): one sequence row of the call's table. alfa / pos_alfa
// are the squashed learning rates (pos_alfa == alfa for "use alpha"), p_up /
// p_low the Bernoulli reward probabilities (kRlSimBernoulli only), src the
// row's first element in the call's supplied / observed arrays.
struct RlSimRow {
  double v, sv, a, z, sz, t, st;
  double q, alfa, pos_alfa;
  double p_up, p_low;
  int64_t src;
};

enum RlSimSource : int32_t {
  kRlSimBernoulli = 0,  // reward = u < p, u the option's own Philox stream
  kRlSimSupplied = 1,   // reward = in_up / in_low[src + k]
  kRlSimObserved = 2,   // Q moves by obs_resp / in_up (the observed feedback)[src + k]
};

// Trial k of global row row0 + r is element off[r] + k of out and of the
// (nullable) per-trial arrays. A lane owns one row and walks its trials in
// order; a wave owns rows [w * wave_rows, + wave_rows) and hands the next one
// to a lane whose row has ended. The walk is sim_drift_kernel's (DriftCall:
// step, scale, max_steps), its random words Philox4x32-10 at counter (k lo, k
// hi, row0 + r, stream): streams 1, 2, 3 and 16 + step / 4 as there, 5 / 6 the
// upper / lower option's reward uniform. A trial cut at max_steps is NaN and
// so is every later trial of its row.
constexpr uint32_t kRlSimStreamUp = 5, kRlSimStreamLow = 6;
struct RlSimCall {
  const RlSimRow* rows;  // [R]
  const int64_t* off;    // [R + 1] prefix sums of the trial counts
  int64_t R;
  int64_t row0;
  double dt, step, scale;
  uint32_t max_steps;  // 1 .. 2^31
  int32_t wave_rows;   // a multiple of 64
  uint64_t seed;
  int32_t source;          // RlSimSource
  const double* in_up;     // supplied: the upper option's rewards; observed: the feedback
  const double* in_low;    // supplied: the lower option's rewards
  const int64_t* obs_resp;  // observed: the responses (0 lower, else upper)
  double* out;
  double* feedback;   // the feedback that moved Q
  double* q_up;       // the Q values before the trial's update
  double* q_low;
  double* sim_drift;  // (q_up - q_low) * v
  double* drift;      // the walk's drift: sim_drift (+ sv * normal)
  double* y0;
  double* delay;
  int64_t* n_steps;     // steps taken; 0 for a trial after a cut one
  int64_t* wave_steps;  // [ceil(R / wave_rows)] steps each wave's loop ran
};
void launch_rl_sim(const RlSimCall& C, hipStream_t s);

}  // namespace wfpt
