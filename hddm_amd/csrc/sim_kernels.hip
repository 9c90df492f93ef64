// sim_kernels.hip — the batched inverse-CDF RT sampler on gfx950
// (gen_rts_from_cdf, src/wfpt.pyx:323-354, for many parameter rows at once;
// DESIGN.md §15).
//
//   sim_pdf_kernel    the grid densities, one grid point per lane, one row
//                     per block
//   sim_scan_kernel   the reference's sequential running sum, one lane per row,
//                     tiles staged through LDS
//   sim_norm_kernel   division by the row's total
//   sim_draw_kernel   one draw per lane: uniforms (supplied or Philox),
//                     searchsorted(side='left') by bisection, the
//                     non-decision-time shift
// and the diffusion-path simulator (_gen_rts_from_simulated_drift,
// hddm/generate.py:208-319):
//   sim_drift_kernel  one walk per lane at a time, lanes refilled from their
//                     wave's range of draws, Philox step outcomes
#include <hip/hip_runtime.h>

#include "sim_internal.h"
#include "sim_philox.hpp"
#include "wfpt_quad.hpp"
#include "wfpt_types.hpp"

#pragma clang fp contract(off)

namespace wfpt {
namespace {

constexpr int kSimBlock = 256;   // grid points (pdf / norm) or draws per block
constexpr int kSimRows = 64;     // rows per scan block: one wave, one lane per row
constexpr int kSimCols = 32;     // grid points of a row staged per scan step
constexpr int kSimPitch = kSimCols + 1;  // LDS row pitch (doubles): the lanes' rows on distinct banks

// full_pdf's defaults, which wfpt.pyx:335 takes: n_st = n_sz = 2, adaptive,
// simps_err = 1e-3; err = 1e-4.
__device__ inline Knobs sim_knobs() {
  Knobs K;
  K.err = 1e-4;
  K.n_st = 2;
  K.n_sz = 2;
  K.use_adaptive = 1;
  K.simps_err = 1e-3;
  K.w_outlier = 0.0;
  return K;
}

// blockIdx.x = tile row * blocks per row + the block's position in the row:
// the row's parameters are uniform over the block.
__global__ __launch_bounds__(kSimBlock) void sim_pdf_kernel(SimTile T, int bpr, int* status) {
  const int64_t r = blockIdx.x / bpr;
  const int64_t i = (int64_t)(blockIdx.x % bpr) * kSimBlock + threadIdx.x;
  if (i >= T.m) return;
  Params Q = T.rows[T.row0 + r];
  Q.t = 0.0;  // wfpt.pyx:335: t = st = 0, the delays are added to the draws
  Q.st = 0.0;
  Q.p_outlier = 0.0;
  const Knobs K = sim_knobs();
  const double x = T.grid[i + 1];
  long long ne = 0;
  int flags = 0;
  double p = full_pdf<kRuntime, RegStack<2>>(x, Q, K, ne, flags);
  p = settle(p, x, Q, K, !trial_setup(x, Q).valid, ne, flags);
  if (flags & kFlagErrors) atomicOr(status, flags & kFlagErrors);
  T.W[r * T.m + i] = p;
}

// LDS hand-over inside the scan's one-wave block: orders the wave's LDS
// accesses without a barrier instruction. __syncthreads() would also wait for
// every outstanding global load and store, i.e. expose a memory round trip per
// piece.
__device__ inline void sim_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave per block, lane l owns tile row blockIdx.x * 64 + l. Per step the
// wave stages a 64 x 32 piece of the row-major workspace in LDS (each load
// instruction reads two rows' 256 consecutive bytes), every lane adds its own
// row's 32 values in index order, and the piece goes back the same way. Two
// LDS pieces alternate: the stores of the piece before and the loads of the
// piece after are both issued ahead of the adds, which depend on neither, so
// the wait at the top of the next step (the compiler waits for all of them)
// overlaps the adds instead of exposing a store round trip per step.
static_assert(kSimRows == 64, "sim_scan_kernel's block is one wave (sim_wave_sync)");
__global__ __launch_bounds__(kSimRows) void sim_scan_kernel(SimTile T) {
  __shared__ double tile[2][kSimRows * kSimPitch];
  const int l = threadIdx.x;
  const int half = l >> 5, col = l & (kSimCols - 1);
  const int64_t r0 = (int64_t)blockIdx.x * kSimRows;
  const int rows_here = (T.nrows - r0 < kSimRows) ? (int)(T.nrows - r0) : kSimRows;
  // lane (half, col) moves element col of rows half, half + 2, ... of a piece.
  // The workspace holds whole blocks of 64 rows (sim_ws_rows), so rows past
  // the tile's last are read and written like the others (their sums are
  // never used) and only a row's last, partial piece needs a bounds test:
  // the whole pieces' loads and stores carry no predicate and no branch.
  double* lane0 = T.W + (r0 + half) * T.m + col;
  const int64_t step = 2 * T.m;
  double nxt[kSimCols];
  auto fetch = [&](int64_t c0) {
    const double* p = lane0 + c0;
    if (c0 + kSimCols <= T.m) {
#pragma unroll
      for (int k = 0; k < kSimCols; ++k) nxt[k] = p[k * step];
    } else {
#pragma unroll
      for (int k = 0; k < kSimCols; ++k) nxt[k] = (c0 + col < T.m) ? p[k * step] : 0.0;
    }
  };
  auto put_back = [&](const double* t, int64_t c0) {
    double* p = lane0 + c0;
    if (c0 + kSimCols <= T.m) {
#pragma unroll
      for (int k = 0; k < kSimCols; ++k) p[k * step] = t[(2 * k + half) * kSimPitch + col];
    } else {
#pragma unroll
      for (int k = 0; k < kSimCols; ++k)
        if (c0 + col < T.m) p[k * step] = t[(2 * k + half) * kSimPitch + col];
    }
  };
  fetch(0);
  double acc = 0.0;  // l_cdf[0] = 0 (wfpt.pyx:332)
  int cur = 0;
  for (int64_t c0 = 0; c0 < T.m; c0 += kSimCols, cur ^= 1) {
    double* t = tile[cur];
#pragma unroll
    for (int k = 0; k < kSimCols; ++k) t[(2 * k + half) * kSimPitch + col] = nxt[k];
    sim_wave_sync();
    if (c0 > 0) put_back(tile[cur ^ 1], c0 - kSimCols);
    if (c0 + kSimCols < T.m) fetch(c0 + kSimCols);
    const int nc = (T.m - c0 < kSimCols) ? (int)(T.m - c0) : kSimCols;
#pragma unroll
    for (int k = 0; k < kSimCols; ++k) {
      if (k < nc) {
        acc = acc + t[l * kSimPitch + k];  // l_cdf[i] = l_cdf[i - 1] + pdf
        t[l * kSimPitch + k] = acc;
      }
    }
    sim_wave_sync();
  }
  put_back(tile[cur ^ 1], (T.m - 1) / kSimCols * kSimCols);
  if (l < rows_here) T.tot[T.row0 + r0 + l] = acc;
}

__global__ __launch_bounds__(kSimBlock) void sim_norm_kernel(SimTile T, int bpr) {
  const int64_t r = blockIdx.x / bpr;
  const int64_t i = (int64_t)(blockIdx.x % bpr) * kSimBlock + threadIdx.x;
  if (i >= T.m) return;
  const double tot = T.tot[T.row0 + r];
  T.W[r * T.m + i] = T.W[r * T.m + i] / tot;  // wfpt.pyx:338
}

// One draw per lane. The draw's row is found by bisection in the prefix sums
// (rows without draws are skipped by it); then np.searchsorted(l_cdf, f) of
// wfpt.pyx:347 over l_cdf = [0, W[r][0 .. m)]: the number of entries strictly
// below f, by NumPy's own bisection, clamped to the grid.
__global__ __launch_bounds__(kSimBlock) void sim_draw_kernel(SimTile T, SimDraw D, int64_t first,
                                                             int64_t ndraws) {
  const int64_t q = (int64_t)blockIdx.x * kSimBlock + threadIdx.x;
  if (q >= ndraws) return;
  const int64_t e = first + q;
  int64_t lo = T.row0, hi = T.row0 + T.nrows;  // the last row with off[row] <= e
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (D.off[mid] <= e) lo = mid;
    else hi = mid;
  }
  const int64_t r = lo, j = e - D.off[r];
  const Params Q = T.rows[r];
  double f, u = 0.0;
  if (D.u_choice) {
    f = D.u_choice[e];
    if (Q.st != 0 && D.u_delay) u = D.u_delay[e];
  } else {
    f = philox_uniform(D.seed, (uint64_t)j, (uint32_t)r, 0u);
    if (Q.st != 0) u = philox_uniform(D.seed, (uint64_t)j, (uint32_t)r, 1u);
  }
  const double* cdf = T.W + (r - T.row0) * T.m;
  int64_t a = 0, b = T.m + 1;
  while (a < b) {
    const int64_t mid = a + ((b - a) >> 1);
    const double cv = mid == 0 ? 0.0 : cdf[mid - 1];
    if (cv < f) a = mid + 1;
    else b = mid;
  }
  const int64_t idx = a < T.m ? a : T.m;
  const double rt = T.grid[idx];
  const double sgn = rt > 0 ? 1.0 : (rt < 0 ? -1.0 : 0.0);  // np.sign
  double res;
  if (Q.st == 0) {
    res = rt + sgn * Q.t;  // wfpt.pyx:350
  } else {
    const double delay = u * Q.st + (Q.t - Q.st / 2.);  // wfpt.pyx:345
    res = rt + sgn * delay;                             // wfpt.pyx:352
  }
  D.out[e] = res;
  if (D.idx_out) D.idx_out[e] = idx;
  if (D.uc_out) D.uc_out[e] = f;
  if (D.ud_out) D.ud_out[e] = u;
}

// ---------------------------------------------------------------------------
// The diffusion-path simulator (_gen_rts_from_simulated_drift,
// hddm/generate.py:208-319).

constexpr int kDriftBlock = 64;  // one wave per block: a wave's slot is free again when it ends
constexpr int kDriftRefill = 8;  // idle lanes that trigger a refill while others still walk

// One wave owns draws [blockIdx.x * wave_draws, + wave_draws) of the call.
// Its lanes take the next draw of that range when theirs has crossed (the
// range's cursor is wave-uniform; a finished lane's draw is the cursor plus
// its rank among the idle lanes), so a wave's time is about the mean of its
// trial lengths and not their maximum. Nothing about a draw depends on the
// lane or the wave that ran it: its random words are functions of (seed, row,
// draw index, step index). Each pass of the loop is four steps, one Philox
// call.
__global__ __launch_bounds__(kDriftBlock) void sim_drift_kernel(DriftCall C) {
  const int64_t lo = (int64_t)blockIdx.x * C.wave_draws;
  const int64_t hi = (C.total - lo < C.wave_draws) ? C.total : lo + C.wave_draws;
  const uint32_t key0 = (uint32_t)C.seed, key1 = (uint32_t)(C.seed >> 32);
  int64_t next = lo;
  uint32_t passes = 0;
  bool live = false;
  int64_t e = 0;         // the lane's draw: element of out
  uint64_t j = 0;        // its index inside the row
  uint32_t row = 0;      // global row index
  uint32_t k = 0, nn = kDriftNoSwitch;
  uint64_t thr = 0, thr_switch = 0;
  double y = 0.0, a = 0.0, delay = 0.0;
  for (;;) {
    const uint64_t idle = __ballot(!live);
    const int n_idle = __popcll(idle);
    if (next < hi && (n_idle >= kDriftRefill || n_idle == kDriftBlock)) {
      if (!live) {
        const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        e = next + rank;
        if (e < hi) {
          int64_t r0 = 0, r1 = C.R;  // the last row with off[row] <= e
          while (r1 - r0 > 1) {
            const int64_t mid = r0 + ((r1 - r0) >> 1);
            if (C.off[mid] <= e) r0 = mid;
            else r1 = mid;
          }
          const DriftRow Q = C.rows[r0];
          j = (uint64_t)(e - C.off[r0]);
          row = (uint32_t)(C.row0 + r0);
          a = Q.a;
          nn = Q.nn;
          const double u_t = Q.st != 0 ? philox_uniform(C.seed, j, row, 1u) : 0.0;
          const double u_z = Q.sz != 0 ? philox_uniform(C.seed, j, row, 2u) : 0.0;
          delay = (Q.t + Q.st * u_t) - Q.st / 2.;         // generate.py:245-246
          y = ((Q.z + Q.sz * u_z) - Q.sz / 2.) * a;       // generate.py:252-253
          const double drift = Q.sv != 0 ? Q.v + Q.sv * philox_normal(C.seed, j, row, 3u) : Q.v;
          thr = drift_threshold(0.5 * (1 + C.scale * drift));  // generate.py:279
          double drift_switch = 0.0;
          thr_switch = 0;
          if (nn != kDriftNoSwitch) {  // generate.py:272-277, 284-286
            drift_switch = Q.V_switch != 0
                               ? Q.v_switch + Q.V_switch * philox_normal(C.seed, j, row, 4u)
                               : Q.v_switch;
            thr_switch = drift_threshold(0.5 * (1 + C.scale * drift_switch));
          }
          k = 0;
          live = true;
          if (C.y0) C.y0[e] = y;
          if (C.delay) C.delay[e] = delay;
          if (C.drift) C.drift[e] = drift;
          if (C.drift_switch) C.drift_switch[e] = drift_switch;
        }
      }
      next += n_idle;
    }
    if (__ballot(live) == 0) break;
    ++passes;
    if (live) {
      // k is a multiple of 4 here: word k % 4 of stream 16 + k / 4 decides step k
      const Philox o = philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), row, 16u + (k >> 2), key0,
                                     key1);
      bool crossed = false, spent = false;
      double y2 = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // selects, no branches: a lane that has stopped keeps its state
        const uint64_t th = k >= nn ? thr_switch : thr;
        const double yn = y + ((uint64_t)o.w[i] < th ? C.step : -C.step);  // generate.py:287-289
        const bool outside = yn < 0 || yn > a;                             // generate.py:291
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
        C.out[e] = __builtin_nan("");
        if (C.n_steps) C.n_steps[e] = (int64_t)k;
      }
    }
  }
  if (C.wave_steps && threadIdx.x == 0) C.wave_steps[blockIdx.x] = 4 * (int64_t)passes;
}

int sim_blocks_per_row(int64_t m) { return (int)((m + kSimBlock - 1) / kSimBlock); }

}  // namespace

void launch_sim_pdf(const SimTile& T, int* status, hipStream_t s) {
  if (T.nrows <= 0 || T.m <= 0) return;
  const int bpr = sim_blocks_per_row(T.m);
  hipLaunchKernelGGL(sim_pdf_kernel, dim3((unsigned)((int64_t)bpr * T.nrows)), dim3(kSimBlock), 0,
                     s, T, bpr, status);
}

void launch_sim_scan(const SimTile& T, hipStream_t s) {
  if (T.nrows <= 0 || T.m <= 0) return;
  hipLaunchKernelGGL(sim_scan_kernel, dim3((T.nrows + kSimRows - 1) / kSimRows), dim3(kSimRows), 0,
                     s, T);
}

void launch_sim_norm(const SimTile& T, hipStream_t s) {
  if (T.nrows <= 0 || T.m <= 0) return;
  const int bpr = sim_blocks_per_row(T.m);
  hipLaunchKernelGGL(sim_norm_kernel, dim3((unsigned)((int64_t)bpr * T.nrows)), dim3(kSimBlock), 0,
                     s, T, bpr);
}

void launch_sim_draw(const SimTile& T, const SimDraw& D, int64_t first, int64_t ndraws,
                     hipStream_t s) {
  if (ndraws <= 0) return;
  hipLaunchKernelGGL(sim_draw_kernel, dim3((unsigned)((ndraws + kSimBlock - 1) / kSimBlock)),
                     dim3(kSimBlock), 0, s, T, D, first, ndraws);
}

// The caller checks that the wave count fits a grid's x dimension.
void launch_sim_drift(const DriftCall& C, hipStream_t s) {
  if (C.total <= 0) return;
  const int64_t waves = (C.total + C.wave_draws - 1) / C.wave_draws;
  hipLaunchKernelGGL(sim_drift_kernel, dim3((unsigned)waves), dim3(kDriftBlock), 0, s, C);
}

}  // namespace wfpt
