// rl_kernels.hip — the reinforcement-learning likelihood family on gfx950
// (wiener_like_rlddm, wiener_like_rl, wiener_like_multi_rlddm; src/wfpt.pyx:79-241,
// 277-320).
//
//   rl_scan_kernel      the Q-value recurrence, one lane per segment -> each
//                       trial's drift (qs[1] - qs[0]) * v
//   rl_scan_multi_kernel, rl_fill_multi_kernel  the same over several row tables
//   rl_choice_kernel    wiener_like_rl's choice probability, one trial per lane
//   rl_fill_kernel      node parameter rows -> per-trial arrays (node batch)
//   rl_node_sum_kernel  per-node sums in the single-node call's order
//
// The densities of the DDM variants are not computed here: the drift buffer
// goes into the v slot of the per-trial-parameter pass (multi_fast_kernel /
// multi_kernel through launch_multi_fast / launch_multi).
#include <hip/hip_runtime.h>

#include "rl_internal.h"
#include "rl_update.hpp"
#include "wfpt_kernel_common.hpp"

#pragma clang fp contract(off)

namespace wfpt {
namespace {

constexpr int kRlScanBlock = 64; // one wave: few segments still spread over the CUs
constexpr int kRlSumBlock = 1024;  // finalize_kernel's block
constexpr int kRlAhead = 8;        // steps whose inputs the scan loads ahead

// The Q recurrence. Bit-exact with the reference's arithmetic: the drift is one
// subtraction and one multiplication, the update q + alfa * (f - q) three
// separately rounded operations (rl_q_update, shared with the closed-loop
// simulator), the learning-rate choice the strict feedback > q (wfpt.pyx:145).
// A one-ulp difference in q could flip that comparison and change every later
// trial.
__device__ __forceinline__ void rl_scan_lane(const RlLayout& L, int r, const RlRow& R,
                                             const double* vmul, const double* rate,
                                             double* drift_c, double* drift_in) {
  const int64_t start = L.lane_start[r], len = L.lane_len[r];
  const int64_t out0 = L.lane_out[r] - (L.score_first ? 0 : 1);
  double q0 = R.q, q1 = R.q;  // qs[0] lower, qs[1] upper boundary (wfpt.pyx:118-119)
  // The inputs of kRlAhead steps are loaded before the steps run: none of
  // them depends on q, and a step is otherwise one exposed memory round trip
  // (measured: 300 ns per step, 23 us for a 75-trial condition). Steps past
  // the segment's end load its last step again (a valid address) and are
  // skipped.
  for (int64_t k0 = 0; k0 < len; k0 += kRlAhead) {
    int resp[kRlAhead];
    double f[kRlAhead], vm[kRlAhead], al[kRlAhead];
#pragma unroll
    for (int u = 0; u < kRlAhead; ++u) {
      const int64_t k = k0 + u < len ? k0 + u : len - 1;
      const int64_t e = L.step_off[k] + r;  // consecutive lanes, consecutive addresses
      resp[u] = L.resp_t[e];
      f[u] = L.fb_t[e];
      vm[u] = vmul ? vmul[start + k] : R.v;
      al[u] = rate ? rate[start + k] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kRlAhead; ++u) {
      const int64_t k = k0 + u;
      if (k < len) {
        const int64_t j = start + k;
        const double drift = (q1 - q0) * vm[u];
        if (k > 0 || L.score_first) drift_c[out0 + k] = drift;
        if (drift_in) drift_in[L.caller ? L.caller[j] : j] = drift;
        const double qs = resp[u] ? q1 : q0;
        const double a = rate ? al[u] : (f[u] > qs ? R.pos_alfa : R.alfa);
        const double qn = rl_q_update(qs, a, f[u]);
        if (resp[u]) q1 = qn;
        else q0 = qn;
      }
    }
  }
}

__global__ __launch_bounds__(kRlScanBlock) void rl_scan_kernel(RlLayout L, RlRow one,
                                                               const RlRow* rows,
                                                               const double* vmul,
                                                               const double* rate, double* drift_c,
                                                               double* drift_in) {
  const int r = blockIdx.x * kRlScanBlock + threadIdx.x;
  if (r >= L.n_seg) return;
  const RlRow R = rows ? rows[L.lane_node ? L.lane_node[r] : 0] : one;
  rl_scan_lane(L, r, R, vmul, rate, drift_c, drift_in);
}

// The same recurrence over T.n_tables row tables: lane g scans segment g %
// n_seg with table g / n_seg's row of the segment's node, so the lanes of one
// table read the step-major addresses the one-table scan reads, and writes
// into that table's block of drift_c (m each) and drift_in (n each).
__global__ __launch_bounds__(kRlScanBlock) void rl_scan_multi_kernel(RlLayout L, RlTables T,
                                                                     const RlRow* rows,
                                                                     double* drift_c,
                                                                     double* drift_in) {
  const int g = blockIdx.x * kRlScanBlock + threadIdx.x;
  if (g >= T.n_tables * L.n_seg) return;
  const int t = g / L.n_seg, r = g - t * L.n_seg;
  const RlRow R = rows[(int64_t)t * T.n_nodes + L.lane_node[r]];
  rl_scan_lane(L, r, R, nullptr, nullptr, drift_c + (int64_t)t * T.m,
               drift_in ? drift_in + (int64_t)t * T.n : nullptr);
}

// wfpt.pyx:210-227: p = 0.5 at drift 0, else the ratio of the two
// 2.718281828459**(.) - 1 terms (the reference's truncated base, not exp) or
// one minus it by response; then the outlier mixture and the log. No a, no
// integration knobs: the reference ignores them here.
__global__ __launch_bounds__(kBlock) void rl_choice_kernel(const double* drift_c,
                                                             const unsigned char* resp_c,
                                                             int64_t m, double z, double p_outlier,
                                                             double wp_outlier, double* lp,
                                                             double* part, int* zeros) {
  __shared__ double ss[kBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double s = 0.0;
  if (i < m) {
    const double drift = drift_c[i];
    double p;
    if (drift == 0) {
      p = 0.5;
    } else {
      const double ratio = (pow(2.718281828459, -2 * z * drift) - 1) /
                           (pow(2.718281828459, -2 * drift) - 1);
      p = resp_c[i] == 1 ? ratio : 1 - ratio;
    }
    p = p * (1 - p_outlier) + wp_outlier;
    s = log_val(p);  // p == 0: -inf, the whole sum's value (wfpt.pyx:224-225)
    lp[i] = s;
  }
  // lp_sum_kernel's order (block_reduce)
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) ss[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x] = ((ss[0] + ss[1]) + (ss[2] + ss[3]));
    zeros[blockIdx.x] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void rl_fill_kernel(const int32_t* node_c, int64_t m,
                                                           const Params* P, int mask,
                                                           double* dst) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const double* row = reinterpret_cast<const double*>(P + node_c[i]);
  int slot = 0;
#pragma unroll
  for (int f = 1; f < 7; ++f) {
    if (mask & (1 << f)) {
      dst[(int64_t)slot * m + i] = row[f];
      ++slot;
    }
  }
}

// rl_fill_kernel over T.n_tables tables: trial i of the T.n_tables x T.m
// takes the row of its node in table i / m.
__global__ __launch_bounds__(kBlock) void rl_fill_multi_kernel(const int32_t* node_c, RlTables T,
                                                                 const Params* P, int mask,
                                                                 double* dst) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t total = (int64_t)T.n_tables * T.m;
  if (i >= total) return;
  const int64_t t = i / T.m;
  const double* row = reinterpret_cast<const double*>(P + t * T.n_nodes + node_c[i - t * T.m]);
  int slot = 0;
#pragma unroll
  for (int f = 1; f < 7; ++f) {
    if (mask & (1 << f)) {
      dst[(int64_t)slot * total + i] = row[f];
      ++slot;
    }
  }
}

// first partial of node j in the scratch array: the nodes' ranges
// ceil(m_j / 256) never overlap (floor(off[j + 1] / 256) - floor(off[j] / 256)
// + 1 >= ceil((off[j + 1] - off[j]) / 256))
__device__ inline int64_t rl_partial_base(int64_t off, int32_t j) { return off / kBlock + j; }

// One block per node. First the node's 256-trial block sums exactly as
// lp_sum_kernel forms them over the single-node call's compact array (block b
// = the node's trials [256 b, 256 b + 256), butterfly wave sums, then (w0 +
// w1) + (w2 + w3)); then finalize_kernel's one-block order over those
// partials: thread t adds partials t, t + 1024, ... onto 0.0, a butterfly per
// wave, and thread 0 adds the 16 wave sums in rising order onto 0.0.
__global__ __launch_bounds__(kRlSumBlock) void rl_node_sum_kernel(const double* lp,
                                                                  const int64_t* off,
                                                                  double* scratch, double* res) {
  __shared__ double sw[kRlSumBlock / 64];
  const int32_t j = blockIdx.x;
  const int64_t lo = off[j], hi = off[j + 1];
  const int64_t nb = (hi - lo + kBlock - 1) / kBlock;
  double* part = scratch + rl_partial_base(lo, j);
  const int t = threadIdx.x, w = t >> 6, g = t >> 8;  // g: the 256-lane group of the thread
  for (int64_t b0 = 0; b0 < nb; b0 += kRlSumBlock / kBlock) {
    const int64_t b = b0 + g;
    const int64_t i = lo + b * kBlock + (t & (kBlock - 1));
    double v = (b < nb && i < hi) ? lp[i] : 0.0;
    v = wave_sum(v);
    if ((t & 63) == 0) sw[w] = v;
    __syncthreads();
    if ((t & (kBlock - 1)) == 0 && b < nb)
      part[b] = ((sw[4 * g] + sw[4 * g + 1]) + (sw[4 * g + 2] + sw[4 * g + 3]));
    __syncthreads();
  }
  double s = 0.0;
  for (int64_t b = t; b < nb; b += kRlSumBlock) s += part[b];
  s = wave_sum(s);
  if ((t & 63) == 0) sw[w] = s;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
    for (int k = 0; k < kRlSumBlock / 64; ++k) tot += sw[k];
    res[j] = tot;
  }
}

}  // namespace

void launch_rl_scan(const RlLayout& L, const RlRow& one, const RlRow* rows, const double* vmul,
                    const double* rate, double* drift_c, double* drift_in, hipStream_t s) {
  if (L.n_seg <= 0) return;
  const int nb = (L.n_seg + kRlScanBlock - 1) / kRlScanBlock;
  hipLaunchKernelGGL(rl_scan_kernel, dim3(nb), dim3(kRlScanBlock), 0, s, L, one, rows, vmul, rate,
                     drift_c, drift_in);
}

void launch_rl_scan_multi(const RlLayout& L, const RlTables& T, const RlRow* rows, double* drift_c,
                          double* drift_in, hipStream_t s) {
  const int64_t lanes = (int64_t)T.n_tables * L.n_seg;
  if (lanes <= 0) return;
  const int nb = (int)((lanes + kRlScanBlock - 1) / kRlScanBlock);
  hipLaunchKernelGGL(rl_scan_multi_kernel, dim3(nb), dim3(kRlScanBlock), 0, s, L, T, rows, drift_c,
                     drift_in);
}

void launch_rl_choice(const double* drift_c, const unsigned char* resp_c, int64_t m, double z,
                      double p_outlier, double wp_outlier, double* lp, double* part, int* zeros,
                      hipStream_t s) {
  const int64_t nb = (m + kBlock - 1) / kBlock;
  if (nb == 0) return;
  hipLaunchKernelGGL(rl_choice_kernel, dim3(nb), dim3(kBlock), 0, s, drift_c, resp_c, m, z,
                     p_outlier, wp_outlier, lp, part, zeros);
}

void launch_rl_fill(const int32_t* node_c, int64_t m, const Params* P, int mask, double* dst,
                    hipStream_t s) {
  const int64_t nb = (m + kBlock - 1) / kBlock;
  if (nb == 0 || (mask & 0x7e) == 0) return;
  hipLaunchKernelGGL(rl_fill_kernel, dim3(nb), dim3(kBlock), 0, s, node_c, m, P, mask, dst);
}

void launch_rl_fill_multi(const int32_t* node_c, const RlTables& T, const Params* P, int mask,
                          double* dst, hipStream_t s) {
  const int64_t nb = ((int64_t)T.n_tables * T.m + kBlock - 1) / kBlock;
  if (nb == 0 || (mask & 0x7e) == 0) return;
  hipLaunchKernelGGL(rl_fill_multi_kernel, dim3(nb), dim3(kBlock), 0, s, node_c, T, P, mask, dst);
}

static_assert(kBlock == 256, "rl_node_partials (rl_internal.h) counts 256-trial blocks");

void launch_rl_node_sum(const double* lp, const int64_t* off, int32_t n_nodes, double* scratch,
                        double* res, hipStream_t s) {
  if (n_nodes <= 0) return;
  hipLaunchKernelGGL(rl_node_sum_kernel, dim3(n_nodes), dim3(kRlSumBlock), 0, s, lp, off, scratch,
                     res);
}

}  // namespace wfpt
