// wfpt_fold.hip — fold_kernel<MODE>: one wave per chunk, its deferred trials
// (exact path, trees deeper than kTreeDepth) settled in lane order on the
// per-lane walk and added to the chunk's partial.
#include "wfpt_kernel_common.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// Blocks of the deferred-trial kernel (fold).
constexpr int kFoldGrid = 16384;

// Folds every chunk's deferred trials into it, one wave per chunk: slot k of
// chunk c (its k-th deferred lane) on lane k, settled on the exact path
// (near-ties, ambiguous series decisions, subnormal densities) or the per-lane
// walk (trees deeper than kTreeDepth); the mixture and log (emit), and the
// wave sum added to the chunk's partial (a fixed order).
template <int MODE, bool COUNT, int OUT>
__global__ __launch_bounds__(256, WFPT_SLOW_WAVES) void fold_kernel(TrialArgs A, Work W, int64_t nw) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  long long ne = 0;
  int errf = 0;
  for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < nw; c += nwaves) {
    const int ntot = W.wl_n[c];
    if (ntot == 0) continue;  // wave-uniform
    double lp = 0.0;
    int zero = 0;
    if (lane < ntot) {
      const int64_t slot = c * 64 + lane;
      const int64_t i = c * 64 + W.wl[slot];
      const int fl = W.rflag[slot];
      long long n1 = 0;
      const double p = (fl & kFlagExact) ? exact_pdf(A.x[i], A.P, A.K, &n1, &errf)
                                         : fallback_pdf<MODE>(A.x[i], A.P, A.K, &n1, &errf);
      ne += n1;
      if (COUNT) atomicAdd(&W.prof[(fl & kFlagExact) ? 5 : 6], 1);
      emit<OUT>(A, i, p, lp, zero);
    }
    if (sum_out(OUT)) {
      lp = wave_sum(lp);
      const int zs = __popcll(__ballot(zero != 0));
      if (lane == 0) {
        A.out[c] = A.out[c] + lp;
        A.zeros[c] = A.zeros[c] + zs;
      }
    }
  }
  if (errf & kFlagErrors) atomicOr(A.status, errf & kFlagErrors);
  if (COUNT) {
    ne = wave_sum_ll(ne);
    if (lane == 0) atomicAdd(A.evals, (unsigned long long)ne);
  }
}

// ---------------------------------------------------------------------------
// launchers

// One wave per chunk, up to kFoldGrid blocks of 4.
void launch_fold(int mode, bool count, int out, const TrialArgs& A, const Work& W, hipStream_t s) {
  const int64_t nw = (A.n + 63) / 64;
  const int64_t gf = std::min<int64_t>(kFoldGrid, (nw + 3) / 4);
  with_mode(mode, [&](auto m) {
    with_build<true>(count, out, [&](auto c, auto o) {
      hipLaunchKernelGGL((fold_kernel<decltype(m)::value, decltype(c)::value, decltype(o)::value>),
                         dim3(gf), dim3(256), 0, s, A, W, nw);
    });
  });
}

}  // namespace wfpt
