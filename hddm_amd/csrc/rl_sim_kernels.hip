// rl_sim_kernels.hip — the closed-loop RLDDM simulator on gfx950
// (gen_rand_rlddm_data, hddm/generate.py:430-516, and its one-step-ahead form,
// generate.py:608-661).
//
//   rl_sim_kernel  one sequence per lane: simulate a trial as a diffusion path
//                  (sim_drift_kernel's walk), take the chosen option's reward,
//                  move its Q value (rl_scan_lane's update), form the next
//                  trial's drift, repeat
#include <hip/hip_runtime.h>

#include "rl_update.hpp"
#include "sim_internal.h"
#include "sim_philox.hpp"

#pragma clang fp contract(off)

namespace wfpt {
namespace {

constexpr int kRlSimBlock = 64;  // one wave per block, no LDS (sim_drift_kernel's shape)

// One wave owns rows [blockIdx.x * wave_rows, + wave_rows) of the call. A lane
// whose row has ended takes the next row of that range (the cursor is
// wave-uniform; the lane's row is the cursor plus its rank among the lanes
// that ask). Between two trials of a row the lane closes the loop: feedback, Q
// update, the next drift and its step threshold; the steady state is
// sim_drift_kernel's pass of four steps per Philox call. Nothing about a trial
// depends on the lane or the wave that ran it: its random words are functions
// of (seed, row, trial, stream), and its Q values of the row's earlier trials.
__global__ __launch_bounds__(kRlSimBlock) void rl_sim_kernel(RlSimCall C) {
  const int64_t lo = (int64_t)blockIdx.x * C.wave_rows;
  const int64_t hi = (C.R - lo < C.wave_rows) ? C.R : lo + C.wave_rows;
  const uint32_t key0 = (uint32_t)C.seed, key1 = (uint32_t)(C.seed >> 32);
  int64_t next = lo;
  uint32_t passes = 0;
  bool live = false;   // a walk is under way
  bool done = false;   // the wave's range has no row left for this lane
  int64_t r = 0;       // the lane's row in the call's table
  int64_t e0 = 0;      // element of its first trial
  int64_t n = 0, kt = 0;  // its trials, and the one under way
  uint32_t row = 0;    // global row index (the random streams')
  double q_up = 0.0, q_low = 0.0;
  uint32_t k = 0;
  uint64_t thr = 0;
  double y = 0.0, a = 0.0, delay = 0.0;
  for (;;) {
    if (__ballot(!live && !done) != 0) {
      const bool want = !live && !done && kt >= n;
      const uint64_t asks = __ballot(want);
      if (asks != 0) {
        if (want) {
          const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(asks >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)asks, 0u));
          r = next + rank;
          if (r < hi) {
            e0 = C.off[r];
            n = C.off[r + 1] - e0;
            kt = 0;
            row = (uint32_t)(C.row0 + r);
            q_up = q_low = C.rows[r].q;  // generate.py:478-479
          } else {
            done = true;
          }
        }
        next += __popcll(asks);
      }
      if (!live && !done && kt < n) {  // the next trial of the row
        const RlSimRow Q = C.rows[r];
        const uint64_t j = (uint64_t)kt;
        const int64_t e = e0 + kt;
        a = Q.a;
        const double sim_drift = (q_up - q_low) * Q.v;  // generate.py:487
        const double u_t = Q.st != 0 ? philox_uniform(C.seed, j, row, 1u) : 0.0;
        const double u_z = Q.sz != 0 ? philox_uniform(C.seed, j, row, 2u) : 0.0;
        delay = (Q.t + Q.st * u_t) - Q.st / 2.;    // generate.py:245-246
        y = ((Q.z + Q.sz * u_z) - Q.sz / 2.) * a;  // generate.py:252-253
        const double drift =
            Q.sv != 0 ? sim_drift + Q.sv * philox_normal(C.seed, j, row, 3u) : sim_drift;
        thr = drift_threshold(0.5 * (1 + C.scale * drift));  // generate.py:279
        k = 0;
        live = true;
        if (C.q_up) C.q_up[e] = q_up;
        if (C.q_low) C.q_low[e] = q_low;
        if (C.sim_drift) C.sim_drift[e] = sim_drift;
        if (C.drift) C.drift[e] = drift;
        if (C.y0) C.y0[e] = y;
        if (C.delay) C.delay[e] = delay;
      }
    }
    if (__ballot(live) == 0) {
      if (__ballot(!done) == 0) break;
      continue;  // rows without trials were handed out: the lanes ask again
    }
    ++passes;
    if (live) {
      // k is a multiple of 4 here: word k % 4 of stream 16 + k / 4 decides step k
      const Philox o = philox4x32_10((uint32_t)kt, (uint32_t)((uint64_t)kt >> 32), row,
                                     16u + (k >> 2), key0, key1);
      bool crossed = false, spent = false;
      double y2 = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // selects, no branches: a lane that has stopped keeps its state
        const double yn = y + ((uint64_t)o.w[i] < thr ? C.step : -C.step);  // generate.py:287-289
        const bool outside = yn < 0 || yn > a;                              // generate.py:291
        const bool cross = live && outside, move = live && !outside;
        y2 = cross ? yn : y2;
        crossed = crossed || cross;
        y = move ? yn : y;
        k += move ? 1u : 0u;
        const bool last = move && k == C.max_steps;
        spent = spent || last;
        live = move && !last;
      }
      const int64_t e = e0 + kt;
      if (crossed) {  // generate.py:301-313: y1 = y, the crossing step's index = k
        const double m = (y2 - y) / C.dt;
        const double b = y2 - (m * (double)k) * C.dt;
        const double rt = y2 < 0 ? (0 - b) / m : (a - b) / m;
        const double signed_rt = (rt + delay) * (y2 < 0 ? -1.0 : 1.0);
        C.out[e] = signed_rt;
        if (C.n_steps) C.n_steps[e] = (int64_t)k + 1;
        // generate.py:496-509: the response, the chosen option's reward, its Q value
        const RlSimRow* Q = C.rows + r;
        bool up = signed_rt > 0;
        double f;
        if (C.source == kRlSimObserved) {  // generate.py:640-655: Q follows the data
          up = C.obs_resp[Q->src + kt] != 0;
          f = C.in_up[Q->src + kt];
        } else if (C.source == kRlSimSupplied) {
          f = (up ? C.in_up : C.in_low)[Q->src + kt];
        } else {
          const double u = philox_uniform(C.seed, (uint64_t)kt, row,
                                          up ? kRlSimStreamUp : kRlSimStreamLow);
          f = u < (up ? Q->p_up : Q->p_low) ? 1.0 : 0.0;
        }
        const double qc = up ? q_up : q_low;
        const double qn = rl_q_update(qc, f > qc ? Q->pos_alfa : Q->alfa, f);
        q_up = up ? qn : q_up;
        q_low = up ? q_low : qn;
        if (C.feedback) C.feedback[e] = f;
        ++kt;
      } else if (spent) {  // the cut trial and the rest of its row are NaN
        const double nan = __builtin_nan("");
        if (C.n_steps) C.n_steps[e] = (int64_t)k;
        if (C.feedback) C.feedback[e] = nan;
        C.out[e] = nan;
        for (int64_t kk = kt + 1; kk < n; ++kk) {
          const int64_t t = e0 + kk;
          C.out[t] = nan;
          if (C.n_steps) C.n_steps[t] = 0;
          double* const dbg[] = {C.feedback, C.q_up, C.q_low, C.sim_drift, C.drift, C.y0, C.delay};
          for (double* d : dbg)
            if (d) d[t] = nan;
        }
        kt = n;
      }
    }
  }
  if (C.wave_steps && threadIdx.x == 0) C.wave_steps[blockIdx.x] = 4 * (int64_t)passes;
}

}  // namespace

// The caller checks that the wave count fits a grid's x dimension.
void launch_rl_sim(const RlSimCall& C, hipStream_t s) {
  if (C.R <= 0) return;
  const int64_t waves = (C.R + C.wave_rows - 1) / C.wave_rows;
  hipLaunchKernelGGL(rl_sim_kernel, dim3((unsigned)waves), dim3(kRlSimBlock), 0, s, C);
}

}  // namespace wfpt
