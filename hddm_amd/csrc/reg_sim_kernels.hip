// reg_sim_kernels.hip — the regressor's posterior predictive on gfx950
// (wfpt_reg_like's random(), hddm/models/hddm_regression.py:39-56: one
// simulated RT per trial at the trial's own regressed parameters, each by
// _gen_rts_from_simulated_drift, hddm/generate.py:208-319).
//
//   reg_sim_kernel   one walk per lane at a time over the (sweep, trial)
//                    elements of a tile of sweeps; a lane forms its trial's
//                    parameters (reg_predict) when it picks the element up
#include <hip/hip_runtime.h>

#include "reg_internal.h"
#include "reg_predict.hpp"
#include "sim_philox.hpp"
#include "wfpt_types.hpp"

#pragma clang fp contract(off)

namespace wfpt {
namespace {

constexpr int kRegSimBlock = 64;  // one wave per block, as sim_drift_kernel
constexpr int kRegSimRefill = 8;  // its kDriftRefill

// walk_row_ok's rule (capi_sim.cpp), which the host cannot apply to trial-wise
// parameters.
__device__ inline bool reg_sim_ok(double v, double sv, double a, double z, double sz, double t,
                                  double st) {
  const bool finite = isfinite(v) && isfinite(sv) && isfinite(a) && isfinite(z) && isfinite(sz) &&
                      isfinite(t) && isfinite(st);
  return finite && a > 0 && !(z - sz / 2. < 0) && !(z + sz / 2. > 1);
}

// The wave layout, the refill rule and the four-step pass are
// sim_drift_kernel's (sim_kernels.hip) without the in-trial switch. What
// differs is the refill: the element's row is not looked up in a table but
// formed from the design matrix, and a trial that cannot be walked never
// becomes live. Nothing about a draw depends on the lane or the wave that ran
// it: its random words are functions of (seed, sweep, caller trial, step).
__global__ __launch_bounds__(kRegSimBlock) void reg_sim_kernel(RegSimCall C) {
  const int64_t lo = (int64_t)blockIdx.x * C.wave_draws;
  const int64_t hi = (C.total - lo < C.wave_draws) ? C.total : lo + C.wave_draws;
  const uint32_t key0 = (uint32_t)C.seed, key1 = (uint32_t)(C.seed >> 32);
  int64_t next = lo;
  uint32_t passes = 0;
  uint32_t n_invalid = 0, n_cut = 0;  // wave-uniform
  bool live = false;
  int64_t e = 0;     // the lane's element of out
  uint64_t j = 0;    // its sweep: the draw index of the counter
  uint32_t row = 0;  // its trial's caller index: the row of the counter
  uint32_t k = 0;
  uint64_t thr = 0;
  double y = 0.0, a = 0.0, delay = 0.0;
  for (;;) {
    const uint64_t idle = __ballot(!live);
    const int n_idle = __popcll(idle);
    if (next < hi && (n_idle >= kRegSimRefill || n_idle == kRegSimBlock)) {
      bool bad = false;
      if (!live) {
        const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        e = next + rank;
        if (e < hi) {
          const int64_t sl = e / C.n, p = e - sl * C.n;
          const int64_t gr = sl * C.G + (C.group ? C.group[p] : 0);
          const double* b = C.coef + gr * C.C;
          const Params Q = C.P[gr];
          double f0 = Q.v, f1 = Q.sv, f2 = Q.a, f3 = Q.z, f4 = Q.sz, f5 = Q.t, f6 = Q.st;
#pragma unroll 1
          for (int t = 0; t < C.n_terms; ++t) {
            const double val = reg_predict(C.term[t], C.X + p, C.n, b);
            const int f = C.term[t].param;
            f0 = f == 0 ? val : f0;
            f1 = f == 1 ? val : f1;
            f2 = f == 2 ? val : f2;
            f3 = f == 3 ? val : f3;
            f4 = f == 4 ? val : f4;
            f5 = f == 5 ? val : f5;
            f6 = f == 6 ? val : f6;
          }
          if (C.par) {
            C.par[e] = f0;
            C.par[C.total + e] = f1;
            C.par[2 * C.total + e] = f2;
            C.par[3 * C.total + e] = f3;
            C.par[4 * C.total + e] = f4;
            C.par[5 * C.total + e] = f5;
            C.par[6 * C.total + e] = f6;
          }
          if (reg_sim_ok(f0, f1, f2, f3, f4, f5, f6)) {
            j = (uint64_t)(C.s0 + sl);
            row = (uint32_t)(C.caller ? C.caller[p] : p);
            a = f2;
            const double u_t = f6 != 0 ? philox_uniform(C.seed, j, row, 1u) : 0.0;
            const double u_z = f4 != 0 ? philox_uniform(C.seed, j, row, 2u) : 0.0;
            delay = (f5 + f6 * u_t) - f6 / 2.;  // generate.py:245-246
            y = ((f3 + f4 * u_z) - f4 / 2.) * a;  // generate.py:252-253
            const double drift = f1 != 0 ? f0 + f1 * philox_normal(C.seed, j, row, 3u) : f0;
            thr = drift_threshold(0.5 * (1 + C.scale * drift));  // generate.py:279
            k = 0;
            live = true;
            if (C.y0) C.y0[e] = y;
            if (C.delay) C.delay[e] = delay;
            if (C.drift) C.drift[e] = drift;
          } else {
            bad = true;
            const double nan = __builtin_nan("");
            C.out[e] = nan;
            if (C.y0) C.y0[e] = nan;
            if (C.delay) C.delay[e] = nan;
            if (C.drift) C.drift[e] = nan;
            if (C.n_steps) C.n_steps[e] = 0;
          }
        }
      }
      n_invalid += (uint32_t)__popcll(__ballot(bad));
      next += n_idle;
    }
    if (__ballot(live) == 0) {
      if (next < hi) continue;  // every element just handed out was invalid
      break;
    }
    ++passes;
    bool cut = false;
    if (live) {
      // k is a multiple of 4 here: word k % 4 of stream 16 + k / 4 decides step k
      const Philox o = philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), row, 16u + (k >> 2), key0,
                                     key1);
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
      if (crossed) {  // generate.py:301-313: y1 = y, the crossing step's index = k
        const double m = (y2 - y) / C.dt;
        const double b = y2 - (m * (double)k) * C.dt;
        const double rt = y2 < 0 ? (0 - b) / m : (a - b) / m;
        C.out[e] = (rt + delay) * (y2 < 0 ? -1.0 : 1.0);
        if (C.n_steps) C.n_steps[e] = (int64_t)k + 1;
      } else if (spent) {
        cut = true;
        C.out[e] = __builtin_nan("");
        if (C.n_steps) C.n_steps[e] = (int64_t)k;
      }
    }
    n_cut += (uint32_t)__popcll(__ballot(cut));
  }
  if (threadIdx.x == 0) {
    if (n_invalid) atomicAdd(C.counts, (unsigned long long)n_invalid);
    if (n_cut) atomicAdd(C.counts + 1, (unsigned long long)n_cut);
    if (C.wave_steps) C.wave_steps[blockIdx.x] = 4 * (int64_t)passes;
  }
}

}  // namespace

void launch_reg_sim(const RegSimCall& C, hipStream_t s) {
  if (C.total <= 0) return;
  const int64_t waves = (C.total + C.wave_draws - 1) / C.wave_draws;
  hipLaunchKernelGGL(reg_sim_kernel, dim3((unsigned)waves), dim3(kRegSimBlock), 0, s, C);
}

}  // namespace wfpt
