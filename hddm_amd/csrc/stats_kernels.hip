// stats_kernels.hip — per-row RT summary statistics on gfx950 (gen_ppc_stats,
// hddm/utils.py:241-265, for many rows of signed RTs at once).
//
// Every tier sorts the row's keys (x where x > 0 or x < 0, else 0.0: a zero or
// a NaN belongs to neither boundary) in rising order, padded with +inf to a
// power of two, by a bitonic network, and hands the sorted row to stats_finish,
// which one wave runs: the lower boundary's draws are the keys below 0, the
// upper boundary's the keys above it, both found by bisection; means and
// standard deviations are two-pass sums in one fixed order; the percentiles
// are scipy's scoreatpercentile read off the order statistics.
//
//   stats_wave_kernel    rows <= 256 draws: one wave per row, four rows per
//                        block, the row in the wave's own LDS piece
//   stats_block_kernel   rows <= 4096 draws: one block per row, the row in
//                        dynamic LDS
//   stats_fill / stats_step / stats_global_finish
//                        longer rows: the row in a device workspace, one
//                        launch per bitonic step
#include <hip/hip_runtime.h>

#include "stats_internal.h"

#pragma clang fp contract(off)

namespace wfpt {
namespace {

constexpr int kStatsWaveRows = 4;  // rows (waves) per block of the wave tier
constexpr int kStatsThreads = 256;

// LDS position of element i: one spare double after every 32, so the two
// stride-2 halves of a wave's first bitonic steps fall on different banks.
__device__ inline int stats_pad(int i) { return i + (i >> 5); }

__device__ inline double stats_key(double x) { return (x > 0 || x < 0) ? x : 0.0; }

// Orders one wave's LDS accesses without a barrier instruction (the waves of
// a wave-tier block run independently of each other).
__device__ inline void stats_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The sum of the 64 lanes' values by a fixed butterfly: every lane ends with
// the same bits (IEEE addition commutes).
__device__ inline double stats_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// Compare-exchange t of the bitonic step (kk, j): elements lo < hi = lo | j,
// rising where lo's bit kk is clear.
__device__ inline void stats_pair(int64_t t, int64_t kk, int64_t j, int64_t* lo, int64_t* hi,
                                  bool* up) {
  *lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
  *hi = *lo | j;
  *up = (*lo & kk) == 0;
}

// scipy.stats.scoreatpercentile (_compute_qth_percentile, 'fraction') on the
// m order statistics val(0) <= ... <= val(m - 1), operation for operation.
template <class Val>
__device__ inline double stats_percentile(Val val, int64_t m, double q) {
  if (m == 0) return __builtin_nan("");
  const double idx = q / 100. * (double)(m - 1);
  const int64_t i = (int64_t)idx;
  if ((double)i == idx) return val(i);
  const double w0 = (double)(i + 1) - idx, w1 = idx - (double)i;
  return (val(i) * w0 + val(i + 1) * w1) / (w0 + w1);
}

// Mean and population standard deviation of val(0 .. m): lane l adds elements
// l, l + 64, ... in that order, the 64 partial sums go through
// stats_wave_sum; the second pass sums the squared deviations from the rounded
// mean the same way. The order depends on the row alone. m == 0: NaN, NaN.
template <class Val>
__device__ inline void stats_moments(Val val, int64_t m, int lane, double* mean, double* sd) {
  double acc = 0.0;
  for (int64_t j = lane; j < m; j += 64) acc = acc + val(j);
  const double mu = stats_wave_sum(acc) / (double)m;
  double ss = 0.0;
  for (int64_t j = lane; j < m; j += 64) {
    const double d = val(j) - mu;
    ss = ss + d * d;
  }
  *mean = mu;
  *sd = sqrt(stats_wave_sum(ss) / (double)m);
}

// One whole wave: the statistics of the sorted keys s(0 .. n) into out[K].
template <class Get>
__device__ inline void stats_finish(Get s, int64_t n, const StatsQ& Q, double* out, int lane) {
  int64_t lo = 0, hi = n;  // keys below 0
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (s(mid) < 0.0) lo = mid + 1;
    else hi = mid;
  }
  const int64_t n_lb = lo;
  hi = n;                  // keys not above 0
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (s(mid) <= 0.0) lo = mid + 1;
    else hi = mid;
  }
  const int64_t ub0 = lo, n_ub = n - lo;
  auto ub = [&](int64_t j) { return s(ub0 + j); };              // rising
  auto lb = [&](int64_t j) { return s(n_lb - 1 - j); };         // signed, |x| rising
  auto lb_abs = [&](int64_t j) { return -s(n_lb - 1 - j); };    // np.abs(x[x < 0]), rising
  double mean_ub, sd_ub, mean_lb, sd_lb;
  stats_moments(ub, n_ub, lane, &mean_ub, &sd_ub);
  stats_moments(lb, n_lb, lane, &mean_lb, &sd_lb);
  const int nq = Q.nq;
  if (lane < nq) out[6 + lane] = stats_percentile(ub, n_ub, Q.q[lane]);
  if (lane >= 32 && lane - 32 < nq)
    out[8 + nq + (lane - 32)] = stats_percentile(lb_abs, n_lb, Q.q[lane - 32]);
  if (lane == 0) {
    out[0] = (double)n;
    out[1] = (double)n_ub;
    out[2] = (double)n_lb;
    out[3] = (double)n_ub / (double)n;  // np.mean(x > 0); 0 / 0 = NaN for an empty row
    out[4] = mean_ub;
    out[5] = sd_ub;
    out[6 + nq] = mean_lb;
    out[7 + nq] = sd_lb;
  }
}

static_assert(kStatsWaveMax + (kStatsWaveMax >> 5) == 264, "the wave tier's LDS piece");
__global__ __launch_bounds__(kStatsWaveRows * 64) void stats_wave_kernel(StatsCall C,
                                                                        const int32_t* list,
                                                                        int64_t nlist) {
  __shared__ double piece[kStatsWaveRows][264];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * kStatsWaveRows + wave;
  if (k >= nlist) return;  // wave-uniform; the block has no barrier
  const int64_t r = list ? list[k] : k;
  const int64_t b = C.off[r];
  const int n = (int)(C.off[r + 1] - b);
  const int P = (int)stats_pow2(n);
  double* s = piece[wave];
  for (int i = lane; i < P; i += 64)
    s[stats_pad(i)] = i < n ? stats_key(C.rts[b + i]) : __builtin_inf();
  stats_wave_sync();
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (P >> 1); t += 64) {
        int64_t lo, hi;
        bool up;
        stats_pair(t, kk, j, &lo, &hi, &up);
        const double x = s[stats_pad((int)lo)], y = s[stats_pad((int)hi)];
        if (up ? (x > y) : (x < y)) {
          s[stats_pad((int)lo)] = y;
          s[stats_pad((int)hi)] = x;
        }
      }
      stats_wave_sync();
    }
  }
  stats_finish([&](int64_t i) { return s[stats_pad((int)i)]; }, n, C.Q,
               C.out + r * stats_cols(C.Q.nq), lane);
}

__global__ __launch_bounds__(kStatsThreads) void stats_block_kernel(StatsCall C,
                                                                    const int32_t* list) {
  extern __shared__ double row[];
  const int64_t r = list ? list[blockIdx.x] : blockIdx.x;
  const int64_t b = C.off[r];
  const int n = (int)(C.off[r + 1] - b);
  const int P = (int)stats_pow2(n);  // <= the launch's P: fits the LDS
  for (int i = threadIdx.x; i < P; i += kStatsThreads)
    row[stats_pad(i)] = i < n ? stats_key(C.rts[b + i]) : __builtin_inf();
  __syncthreads();
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += kStatsThreads) {
        int64_t lo, hi;
        bool up;
        stats_pair(t, kk, j, &lo, &hi, &up);
        const double x = row[stats_pad((int)lo)], y = row[stats_pad((int)hi)];
        if (up ? (x > y) : (x < y)) {
          row[stats_pad((int)lo)] = y;
          row[stats_pad((int)hi)] = x;
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x < 64)
    stats_finish([&](int64_t i) { return row[stats_pad((int)i)]; }, n, C.Q,
                 C.out + r * stats_cols(C.Q.nq), (int)threadIdx.x);
}

__global__ __launch_bounds__(kStatsThreads) void stats_fill_kernel(const double* x, int64_t n,
                                                                   int64_t P, double* ws) {
  const int64_t i = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x;
  if (i < P) ws[i] = i < n ? stats_key(x[i]) : __builtin_inf();
}

__global__ __launch_bounds__(kStatsThreads) void stats_step_kernel(double* ws, int64_t P,
                                                                   int64_t kk, int64_t j) {
  const int64_t t = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x;
  if (t >= (P >> 1)) return;
  int64_t lo, hi;
  bool up;
  stats_pair(t, kk, j, &lo, &hi, &up);
  const double x = ws[lo], y = ws[hi];
  if (up ? (x > y) : (x < y)) {
    ws[lo] = y;
    ws[hi] = x;
  }
}

__global__ __launch_bounds__(64) void stats_global_finish_kernel(const double* ws, int64_t n,
                                                                 StatsQ Q, double* out) {
  stats_finish([&](int64_t i) { return ws[i]; }, n, Q, out, (int)threadIdx.x);
}

__global__ __launch_bounds__(kStatsThreads) void stats_count_nan_kernel(
    const double* x, int64_t n, unsigned long long* count) {
  const int64_t i = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x;
  const bool nan = i < n && x[i] != x[i];
  const uint64_t m = __ballot(nan);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (unsigned long long)__popcll(m));
}

}  // namespace

void launch_stats_wave(const StatsCall& C, const int32_t* list, int64_t nlist, hipStream_t s) {
  if (nlist <= 0) return;
  hipLaunchKernelGGL(stats_wave_kernel,
                     dim3((unsigned)((nlist + kStatsWaveRows - 1) / kStatsWaveRows)),
                     dim3(kStatsWaveRows * 64), 0, s, C, list, nlist);
}

void launch_stats_block(const StatsCall& C, const int32_t* list, int64_t nlist, int64_t P,
                        hipStream_t s) {
  if (nlist <= 0) return;
  hipLaunchKernelGGL(stats_block_kernel, dim3((unsigned)nlist), dim3(kStatsThreads),
                     (size_t)stats_lds_doubles(P) * sizeof(double), s, C, list);
}

void launch_stats_global(const StatsCall& C, int64_t row, int64_t first, int64_t n, double* ws,
                         hipStream_t s) {
  const int64_t P = stats_pow2(n);
  hipLaunchKernelGGL(stats_fill_kernel, dim3((unsigned)((P + kStatsThreads - 1) / kStatsThreads)),
                     dim3(kStatsThreads), 0, s, C.rts + first, n, P, ws);
  const unsigned blocks = (unsigned)(((P >> 1) + kStatsThreads - 1) / kStatsThreads);
  for (int64_t kk = 2; kk <= P; kk <<= 1)
    for (int64_t j = kk >> 1; j > 0; j >>= 1)
      hipLaunchKernelGGL(stats_step_kernel, dim3(blocks), dim3(kStatsThreads), 0, s, ws, P, kk, j);
  hipLaunchKernelGGL(stats_global_finish_kernel, dim3(1), dim3(64), 0, s, ws, n, C.Q,
                     C.out + row * stats_cols(C.Q.nq));
}

void launch_stats_count_nan(const double* x, int64_t n, unsigned long long* count,
                            hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(stats_count_nan_kernel,
                     dim3((unsigned)((n + kStatsThreads - 1) / kStatsThreads)),
                     dim3(kStatsThreads), 0, s, x, n, count);
}

}  // namespace wfpt
