// pointwise_kernels.hip — the model-comparison pass on gfx950:
// the reduction over sweeps, per trial, of the log terms every node call leaves
// in device memory.
//
//   pointwise_accumulate_kernel  one trial per lane: the lane reads its state,
//                                walks the tile's T sweeps in rising order and
//                                writes the state back
//   pointwise_finish_kernel      one trial per lane: lppd, p_waic, mean, n_inf
//
// No LDS, no atomics, no cross-lane traffic: a trial's sweeps are visited in
// order by one lane, so the result cannot depend on how the sweeps were tiled.
// A sweep's terms are contiguous over trials: a wave reads 512 consecutive
// bytes per sweep. The update rule is pointwise_update.hpp's.
#include <hip/hip_runtime.h>

#include "pointwise_internal.h"
#include "pointwise_update.hpp"

#pragma clang fp contract(off)

namespace wfpt {
namespace {

constexpr int kPwBlock = 256;

__global__ __launch_bounds__(kPwBlock) void pointwise_accumulate_kernel(
    const double* __restrict__ lp, int64_t T, int64_t len, PointwiseState st) {
  const int64_t i = (int64_t)blockIdx.x * kPwBlock + threadIdx.x;
  if (i >= len) return;
  wfpt_pw::State s{st.m[i], st.r[i], st.mean[i], st.M2[i], st.k[i], st.n_inf[i]};
  const double* p = lp + i;
#pragma unroll 1
  for (int64_t t = 0; t < T; ++t, p += len) wfpt_pw::update(s, *p);
  st.m[i] = s.m;
  st.r[i] = s.r;
  st.mean[i] = s.mean;
  st.M2[i] = s.M2;
  st.k[i] = s.k;
  st.n_inf[i] = s.n_inf;
}

__global__ __launch_bounds__(kPwBlock) void pointwise_finish_kernel(PointwiseState st, int64_t len,
                                                                    int64_t S,
                                                                    double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kPwBlock + threadIdx.x;
  if (i >= len) return;
  const wfpt_pw::State s{st.m[i], st.r[i], st.mean[i], st.M2[i], st.k[i], st.n_inf[i]};
  const wfpt_pw::Result R = wfpt_pw::finish(s, S);
  out[i] = R.lppd;
  out[len + i] = R.p_waic;
  out[2 * len + i] = R.mean;
  out[3 * len + i] = (double)s.n_inf;
}

}  // namespace

void launch_pointwise_accumulate(const double* lp, int64_t T, int64_t len, const PointwiseState& st,
                                 hipStream_t s) {
  const int64_t nb = (len + kPwBlock - 1) / kPwBlock;
  if (nb == 0 || T <= 0) return;
  hipLaunchKernelGGL(pointwise_accumulate_kernel, dim3(nb), dim3(kPwBlock), 0, s, lp, T, len, st);
}

void launch_pointwise_finish(const PointwiseState& st, int64_t len, int64_t S, double* out,
                             hipStream_t s) {
  const int64_t nb = (len + kPwBlock - 1) / kPwBlock;
  if (nb == 0) return;
  hipLaunchKernelGGL(pointwise_finish_kernel, dim3(nb), dim3(kPwBlock), 0, s, st, len, S, out);
}

}  // namespace wfpt
