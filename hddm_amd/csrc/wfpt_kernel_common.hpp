// wfpt_kernel_common.hpp — what the likelihood kernel units share: block
// sizes, the output kinds, the wave / block reductions, a trial's output
// (emit, chunk_out), the deferred slots, the result slot (fin_write), the
// host dispatch from runtime (mode, count, out) to template arguments, and
// the launchers the units export to each other. Included by .hip units only.
//
// The units (one family each; none includes another's .hip):
//   wfpt_level0.hip  direct_kernel, lean_kernel
//   wfpt_engine.hip  engine_kernel (wfpt_engine.hpp: the refinement rounds) and the
//                    uniform-family per-trial-parameter path (multi_fast_kernel,
//                    multi_records_kernel, multi_direct_records_kernel, lp_sum_kernel)
//   wfpt_fold.hip    fold_kernel (the deferred trials)
//   wfpt_sum.hip     launch_trials, finalize_kernel, small_kernel, small_split_kernel,
//                    trial_kernel (fixed Simpson), multi_kernel (mixed families),
//                    publish_kernel, poison_kernel
//   wfpt_node.hip    per-node parameters (wfpt_wiener_like_nodes)
//
// Adaptive / direct integration families (the HDDM case), one resident call:
//   lean_kernel<MODE>     level 0 of every trial, one 64-trial chunk per wave,
//                         boundary-uniform root grids in scalar registers (4
//                         waves/SIMD; the 2-D family's waves whose lanes agree on
//                         every t node's series decision keep those in scalar
//                         registers too: lean_uniform_level0, wfpt_lean.hpp):
//                         a chunk none of whose trials refines
//                         ends here (mixture, log, chunk partial); a chunk that
//                         refines is flagged for the engine's redo pass
//   engine_kernel<MODE>   level 0 + in-wave refinement rounds (z walks, t-node
//                         tasks, tree17) of a chunk per wave; heavy chunks
//                         recorded by the previous call run as 8 split units
//   small_kernel<MODE>    <= 256 trials (one HDDM node): level 0 and the
//                         finalize in one launch
//   direct_kernel         the simple DDM (one pdf_sv per trial)
//   fold_kernel<MODE>     one wave per chunk: its deferred trials (exact path,
//                         trees deeper than kTreeDepth) settled in lane
//                         order and added to the chunk's partial
//   finalize_kernel       fixed-order sum of the chunk partials -> mapped slot
// The per-chunk partial of a chunk is the same value whichever sequence ran
// it (lean, lean + redo, engine, split), so a likelihood is bitwise
// reproducible across call histories. No float atomics on any likelihood
// value. OUT_BOTH builds of the same kernels also write each trial's term
// (wfpt_wiener_like_trials: the per-trial check of the summing path).
#pragma once
#include <cstdio>
#include <cstdlib>

#include "wfpt_grid.hpp"
#include "wfpt_internal.h"
#include "wfpt_lean_tables.hpp"
#include "wfpt_level0.hpp"
#include "wfpt_math.hpp"
#include "wfpt_quad.hpp"
#include "wfpt_series.hpp"
#include "wfpt_types.hpp"
#include "wfpt_zgrid.hpp"

#pragma clang fp contract(off)

namespace wfpt {

constexpr int kBlock = 256;
// Threads per block of the level-0 fast kernel (barrier-free, one chunk of 64
// trials per wave): the block is only the hardware's dispatch unit.
constexpr int kFastBlock = 256;
static inline int64_t fast_blocks(int64_t n) { return (n + kFastBlock - 1) / kFastBlock; }

// Minimum waves per SIMD requested for the level-0 fast kernels (0 = let the
// compiler choose): WFPT_FAST_WAVES for the 1-D / direct modes,
// WFPT_FAST_WAVES_TZ for the 2-D mode. Chosen by tools/ab_variants.py.
#ifndef WFPT_FAST_WAVES
#define WFPT_FAST_WAVES 3
#endif
#ifndef WFPT_FAST_WAVES_TZ
#define WFPT_FAST_WAVES_TZ 3
#endif
template <int MODE>
struct FastWaves {
  static constexpr int value = MODE == kAdaptTZ ? WFPT_FAST_WAVES_TZ : WFPT_FAST_WAVES;
};
// Minimum waves per SIMD of the general (per-lane walk) kernels.
#ifndef WFPT_SLOW_WAVES
#define WFPT_SLOW_WAVES 2
#endif

// OUT_BOTH (the per-trial check of the summing kernels, wfpt_wiener_like_trials):
// exactly OUT_SUM's chunk partials and zero words, plus each trial's log term
// (-inf for a zero density) in A.trial[i]: the same template with one more store.
enum Out : int { OUT_SUM = 0, OUT_ARRAY = 1, OUT_BOTH = 3 };
constexpr bool sum_out(int out) { return out == OUT_SUM || out == OUT_BOTH; }
// OUT_SUM per-chunk zero-count word: zero-density trials | kZeroDefer if the
// chunk's level-0 pass deferred trials (or left the chunk to the redo pass)
constexpr int kZeroDefer = 1 << 16;

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline unsigned long long lanemask_lt(int lane) { return (1ull << lane) - 1ull; }

// Block (256 lanes = 4 waves) reduction of (sum, zeros, evals); lane 0 returns.
template <bool COUNT>
__device__ inline void block_reduce(double& s, int& zeros, long long& ne) {
  __shared__ double ss[kBlock / 64];
  __shared__ int sz[kBlock / 64];
  __shared__ long long sn[kBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  s = wave_sum(s);
  const unsigned long long zb = __ballot(zeros != 0);
  if (COUNT) ne = wave_sum_ll(ne);
  if (lane == 0) {
    ss[w] = s;
    sz[w] = __popcll(zb);
    if (COUNT) sn[w] = ne;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = ((ss[0] + ss[1]) + (ss[2] + ss[3]));
    zeros = sz[0] + sz[1] + sz[2] + sz[3];
    if (COUNT) ne = sn[0] + sn[1] + sn[2] + sn[3];
  }
}

struct TrialArgs {
  const double* x;
  int64_t n;
  Params P;
  Knobs K;
  double wp_outlier;      // w_outlier * p_outlier
  double* out;            // OUT_SUM/BOTH: chunk / block partial sums; OUT_ARRAY: per trial
  int* zeros;             // OUT_SUM/BOTH: chunk / block zero counts
  double* trial;          // OUT_BOTH: per-trial log terms
  unsigned long long* evals;
  int* status;            // error flags (kFlagDepth | kFlagBudget)
  int logp;               // OUT_ARRAY: return log density
};

// Trial output of a settled density p (wfpt.pyx:44 / :70).
template <int OUT>
__device__ inline void emit(const TrialArgs& A, int64_t i, double p, double& lp, int& zero) {
  if (OUT == OUT_ARRAY) {
    p = p * (1 - A.P.p_outlier) + (A.K.w_outlier * A.P.p_outlier);  // wfpt.pyx:44
    A.out[i] = A.logp ? log_val(p) : p;
  } else {
    p = p * (1 - A.P.p_outlier) + A.wp_outlier;  // wfpt.pyx:70
    if (p == 0) zero = 1;
    else lp = log_val(p);
    if (OUT == OUT_BOTH) A.trial[i] = zero ? -INFINITY : lp;
  }
}

// ---------------------------------------------------------------------------
// Deferred trials. A trial the level-0 kernels cannot settle (kFlagExact: its
// value hinges on last-bit rounding; kFlagFallback: its tree is deeper than
// kTreeDepth) takes slot c * 64 + k of its chunk c (k = its rank among the
// chunk's deferred trials): no atomic, and fold_kernel finds a chunk's
// deferred trials on its first lanes.
// Returns whether the chunk deferred any trial (its zero-count word then
// carries kZeroDefer, which finalize reports).
__device__ inline bool defer_slots(const Work& W, int64_t c, int lane, bool defer, int rflag) {
  const unsigned long long b = __ballot(defer);
  const int64_t slot = c * 64 + __popcll(b & lanemask_lt(lane));
  if (defer) {
    W.wl[slot] = (unsigned char)lane;
    W.rflag[slot] = rflag;
  }
  if (lane == 0) W.wl_n[c] = __popcll(b);
  return b != 0ull;
}

// Chunk outputs of the owner lanes (one wave): per-trial emit, deferred
// slots, the chunk partial and the evaluation count.
template <bool COUNT, int OUT>
__device__ inline void chunk_out(const TrialArgs& A, const Work& W, int64_t c, int lane, double p,
                                 bool defer, int rf, long long ne) {
  const int64_t i = c * 64 + lane;
  double lp = 0.0;
  int zero = 0;
  if (i < A.n && !defer) emit<OUT>(A, i, p, lp, zero);  // invalid parameters: p = 0
  const bool anyd = defer_slots(W, c, lane, defer, rf);
  if (sum_out(OUT)) {
    lp = wave_sum(lp);
    const int zs = __popcll(__ballot(zero != 0));
    if (lane == 0) {
      A.out[c] = lp;
      A.zeros[c] = zs | (anyd ? kZeroDefer : 0);
    }
  }
  if (COUNT) {
    const long long nf = wave_sum_ll((i < A.n && !defer) ? ne : 0ll);
    if (lane == 0) atomicAdd(A.evals, (unsigned long long)nf);
  }
}

// Root z grid of boundary b (0: lower, 1: upper) with b wave-uniform: the
// grid is read through a reference into the kernel argument block (scalar
// loads at a uniform offset, on demand) instead of select-copied into
// registers, so it stays in scalar registers. The large-time sines come from
// the call's table (R.S) instead of the per-lane recurrence (same values).
__device__ inline const ZGrid& zgrid_uniform(const RootGrids& R, int b) { return R.G[b]; }

// eng_level0_t's tail (KEEP_F) for one trial, from its five t-node values.
template <int MODE>
__device__ inline int l0_finish(const Trial& tr, const Params& P, const Knobs& K, int flags,
                                unsigned pend, const double (&f)[5], double& p) {
  p = 0.0;
  if (!tr.valid) return kFinal;
  if (flags & kFlagExact) return kExact;
  if (pend) return kTree;
  double lb, ub;
  tree_root<MODE>(tr, P, lb, ub);
  const bool structural = tr.x - lb <= 0;
  const Simp s = simp5(ub - lb, f[0], f[1], f[2], f[3], f[4]);
  int fl = 0;
  const bool refine = simpson_refine(s.S, s.S2, K.simps_err, K.n_st, fl);
  if (fl & kFlagExact) return kExact;
  if (refine) return kTree;
  p = s.S2 + (s.S2 - s.S) / 15;
  if (p > kExactBelow || structural) return kFinal;
  if (!tiny_absorbed(p, P.p_outlier, K.w_outlier)) return kExact;
  p = 0.0;
  return kFinal;
}

// The completion word of a result slot in mapped host memory: a system-scope
// release store, after every result store the call's publication ordered
// before it; the host reads it with an acquire load (wait_word).
__device__ __forceinline__ void publish_word(unsigned long long* w, unsigned long long seq) {
  __hip_atomic_store(w, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The result slot of a call (finalize's last step, one thread): {sum, zero
// count, encoded errors, flags, -, heavy chunks, #tree} and then the
// completion word; resets the device status word.
__device__ inline void fin_write(double t, long long zz, int dd, int* status, double* out,
                                 unsigned long long seq, const int* split_rd, int* split_rs,
                                 int* tree_any, double* mirror) {
  const int st = *status;
  *status = 0;
  out[0] = t;
  out[1] = (double)zz;
  out[2] = (double)(st & kFlagDepth) + ((st & kFlagBudget) ? kBudgetUnit : 0.0);
  int res3 = dd ? kResDeferred : 0;
  double ntree = 0.0;
  if (tree_any) {
    if (*tree_any) res3 |= kResTree;
    ntree = (double)*tree_any;
    *tree_any = 0;
  }
  out[6] = ntree;
  out[3] = (double)res3;
  // heavy chunks recorded for the next call (Split)
  out[5] = split_rd ? (double)split_rd[0] : 0.0;  // class 1 (Split)
  out[7] = split_rd ? (double)split_rd[2] : 0.0;  // class 2
  if (split_rs) {
    split_rs[0] = 0;
    split_rs[2] = 0;
  }
  if (mirror) {  // device copy of the result (the RCCL exchange reads it)
    mirror[0] = out[0];
    mirror[1] = out[1];
    mirror[2] = out[2];
    mirror[3] = out[3];
    mirror[5] = out[5];
    mirror[6] = out[6];
    mirror[7] = out[7];
  }
  // completion word, a system-scope release store after the results (one
  // thread wrote them all): the host may poll it (acquire) instead of waiting
  // on the stream
  publish_word(reinterpret_cast<unsigned long long*>(out) + 4, seq);
}

// The per-lane walk's stack by stack_kind (node_kernel, multi_kernel).
template <int STK>
struct StackOf {
  using type = typename std::conditional<
      STK == 0, RegStack<2>,
      typename std::conditional<STK == 1, RegStack<4>, MemStack<WFPT_MAX_DEPTH>>::type>::type;
};

// ---------------------------------------------------------------------------
// Host side.

inline TrialArgs trial_args(const double* x, int64_t n, const Params& P, const Knobs& K,
                            double* out, int* zeros, unsigned long long* evals, int* status,
                            int logp, double* trial = nullptr) {
  TrialArgs A;
  A.x = x;
  A.n = n;
  A.P = P;
  A.K = K;
  A.wp_outlier = K.w_outlier * P.p_outlier;
  A.out = out;
  A.zeros = zeros;
  A.evals = evals;
  A.status = status;
  A.logp = logp;
  A.trial = trial;
  return A;
}

// Runtime value -> template argument, over a closed set: an unknown value is
// a bug in the caller, never another family's kernel.
[[noreturn]] inline void bad_dispatch(const char* what, int v) {
  fprintf(stderr, "wfpt: no kernel for %s = %d\n", what, v);
  abort();
}
// f(std::integral_constant<int, V>{}) for v == V in [LO, HI] (an integration
// family, or stack_kind's 0..2).
template <int LO, int HI, class F>
inline void with_value(int v, F&& f) {
  if constexpr (LO > HI) bad_dispatch("mode / stack kind", v);
  else if (v == LO) f(std::integral_constant<int, LO>{});
  else with_value<LO + 1, HI>(v, f);
}
template <class F>
inline void with_mode(int mode, F&& f) {  // the direct and adaptive families
  with_value<kDirect, kAdaptTZ>(mode, f);
}
template <class F>
inline void with_flag(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
// f(COUNT, OUT) for the builds a caller of launch_trials / launch_small can
// reach, which are the only ones instantiated:
//   (false | true, OUT_SUM)  the summing call; evals selects the counting build
//   (false, OUT_BOTH)        the per-trial check (wfpt_wiener_like_trials, launch_small)
//   (false, OUT_ARRAY)       wfpt_pdf_array (kPassAll: never the lean pass, so
//                            lean_kernel and the small kernels take ARRAY = false)
template <bool ARRAY, class F>
inline void with_build(bool count, int out, F&& f) {
  if (out == OUT_SUM) {
    with_flag(count, [&](auto c) { f(c, std::integral_constant<int, OUT_SUM>{}); });
    return;
  }
  if (count) bad_dispatch("a counting build of out kind", out);
  if (out == OUT_BOTH) {
    f(std::false_type{}, std::integral_constant<int, OUT_BOTH>{});
    return;
  }
  if constexpr (ARRAY) {
    if (out == OUT_ARRAY) {
      f(std::false_type{}, std::integral_constant<int, OUT_ARRAY>{});
      return;
    }
  }
  bad_dispatch("out kind", out);
}

// What the units export to launch_trials (wfpt_sum.hip). Each does its own
// (mode, count, out) dispatch.
// wfpt_level0.hip: the level-0 pass of the direct family / the lean pass.
void launch_direct(bool count, int out, const TrialArgs& A, const Work& W, hipStream_t s);
// dt: the call's decision table (decision_tab of its err; null: one that never answers)
// first: the chunks dispatched first (the 2-D family; null: stored order)
void launch_lean(int mode, bool count, int out, const TrialArgs& A, const Work& W, hipStream_t s,
                 const DecisionTab* dt, const LeanFirst* first = nullptr);
// wfpt_engine.hip: S's split units, then one wave per chunk (Split{}: the
// redo pass over the chunks W.redo flags).
void launch_engine(int mode, bool count, int out, const TrialArgs& A, const Work& W,
                   const EngTables& T, const Split& S, hipStream_t s);
// wfpt_fold.hip: the fold of the deferred trials.
void launch_fold(int mode, bool count, int out, const TrialArgs& A, const Work& W, hipStream_t s);

}  // namespace wfpt
