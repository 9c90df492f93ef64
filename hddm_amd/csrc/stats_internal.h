// stats_internal.h — launcher interface between the C ABI (capi_sim.cpp) and
// the per-row RT statistics kernels (stats_kernels.hip; gen_ppc_stats,
// hddm/utils.py:241-265). Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wfpt {

constexpr int kStatsMaxQ = 16;           // percentiles per call
constexpr int64_t kStatsWaveMax = 256;   // longest row of the wave tier
constexpr int64_t kStatsBlockMax = 4096; // longest row of the block tier

// The call's percentiles, by value in the kernel arguments.
struct StatsQ {
  double q[kStatsMaxQ];
  int32_t nq;
};
__host__ __device__ inline int stats_cols(int32_t nq) { return 8 + 2 * nq; }

// Row r's draws are rts[off[r] .. off[r + 1]); its K = 8 + 2 nq results go to
// out[r * K ..): n, n_ub, n_lb, accuracy, mean_ub, std_ub, q_ub[nq], mean_lb,
// std_lb, q_lb[nq]. A kernel scores the rows list[0 .. nlist) (list == null:
// rows 0 .. nlist).
struct StatsCall {
  const double* rts;
  const int64_t* off;
  double* out;
  StatsQ Q;
};

// Smallest power of two >= max(n, 2): the length a row is padded to for its
// bitonic sort.
__host__ __device__ inline int64_t stats_pow2(int64_t n) {
  int64_t P = 2;
  while (P < n) P <<= 1;
  return P;
}
// LDS doubles of a row padded to P: one spare double per 32 (stats_kernels.hip)
inline int64_t stats_lds_doubles(int64_t P) { return P + (P >> 5); }

// Wave tier: one wave per row (rows of at most kStatsWaveMax draws), four rows
// per block, each row sorted in its wave's own LDS piece.
void launch_stats_wave(const StatsCall& C, const int32_t* list, int64_t nlist, hipStream_t s);
// Block tier: one 256-thread block per row, sorted in P (+ padding) doubles of
// dynamic LDS; every listed row has stats_pow2(n) <= P <= kStatsBlockMax.
void launch_stats_block(const StatsCall& C, const int32_t* list, int64_t nlist, int64_t P,
                        hipStream_t s);
// Global tier, one row per call sequence: the keys of the row's n draws from
// rts[first] on, padded to P = stats_pow2(n) in ws[P], one launch per bitonic
// step, then the statistics.
void launch_stats_global(const StatsCall& C, int64_t row, int64_t first, int64_t n, double* ws,
                         hipStream_t s);
// *count += the NaNs of x[0 .. n) (the drift sampler's unfinished walks when
// its draws stay on the device); an integer atomic per wave.
void launch_stats_count_nan(const double* x, int64_t n, unsigned long long* count, hipStream_t s);

}  // namespace wfpt
