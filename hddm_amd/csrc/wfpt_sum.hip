// wfpt_sum.hip — a resident call's launch sequence and its result slot:
//   launch_trials      the level-0 pass, the redo pass and the fold of one
//                      call (or the fixed Simpson kernel), by family
//   finalize_kernel    fixed-order sum of the chunk partials -> mapped slot
//   small_kernel<MODE>, small_split_kernel
//                      <= 256 trials (one HDDM node): level 0 and the
//                      finalize in one launch (launch_small)
//   trial_kernel<MODE> fixed composite Simpson (use_adaptive = 0)
//   multi_kernel       wiener_like_multi with mixed families (launch_multi)
//   publish_kernel, poison_kernel   the all-reduced (or a failed rank's) result
#include "wfpt_kernel_common.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// out[0] = sum of nb partials, out[1] = number of zero trials, out[2] = error
// flags encoded as counts that survive a sum over ranks (depth + 2^20 budget),
// out[3] = kResDeferred if some chunk's word carries kZeroDefer (defer_bits:
// per-chunk partials of the adaptive / direct families) | kResTree, then the
// 64-bit completion word out[4] once they are visible. `out` may be mapped
// pinned host memory. Resets the device status word. Fixed summation order
// for a given nb: thread k owns partials k + 1024 j, loaded kFinLoads at a
// time (all in flight together) and summed in j order; then a fixed tree.
// Large nb (C2's 10M trials: 156k partials): one block is bound by a single
// CU's load bandwidth (29 us), so gridDim.x = G > 1 blocks each reduce a
// contiguous range the same way into fin[g] (sum), fin[kFinMaxBlocks + g]
// (zero count), fin[2 kFinMaxBlocks + g] (defer bits), and the last block to
// finish (agent-scope ticket) adds the G block results in g order. Fixed
// order for a given (nb, G); G = 1 is the single-block order.
constexpr int kFinLoads = 16;
constexpr int kFinMaxBlocks = 64;
constexpr int64_t kFinPerBlock = 8192;  // partials per block when split
__global__ __launch_bounds__(1024) void finalize_kernel(const double* part, const int* zeros,
                                                        int64_t nb, int defer_bits,
                                                        int* status, double* out,
                                                        unsigned long long seq,
                                                        const int* split_rd, int* split_rs,
                                                        int* tree_any, double* mirror,
                                                        double* fin, int* ticket) {
  __shared__ double ss[16];
  __shared__ long long sz[16];
  __shared__ int sd[16];
  __shared__ int last;
  const int G = gridDim.x;
  int64_t lo = 0, hi = nb;
  if (G > 1) {
    const int64_t L = (nb + G - 1) / G;
    lo = (int64_t)blockIdx.x * L;
    hi = lo + L < nb ? lo + L : nb;
  }
  double s = 0.0;
  long long z = 0;
  int def = 0;
  for (int64_t b0 = lo + threadIdx.x; b0 < hi; b0 += kFinLoads * 1024) {
    double v[kFinLoads];
    int w[kFinLoads];
#pragma unroll
    for (int j = 0; j < kFinLoads; ++j) {
      const int64_t b = b0 + (int64_t)j * 1024;
      v[j] = b < hi ? part[b] : 0.0;
      w[j] = b < hi ? zeros[b] : 0;
    }
#pragma unroll
    for (int j = 0; j < kFinLoads; ++j) {
      s += v[j];
      z += w[j] & (kZeroDefer - 1);
      def |= w[j];
    }
  }
  def = defer_bits ? (def & kZeroDefer) : 0;
  s = wave_sum(s);
  z = wave_sum_ll(z);
  const bool anyd = __ballot(def != 0) != 0ull;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    ss[w] = s;
    sz[w] = z;
    sd[w] = anyd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    long long zz = 0;
    int dd = 0;
    for (int k = 0; k < 16; ++k) {
      t += ss[k];
      zz += sz[k];
      dd |= sd[k];
    }
    if (G > 1) {
      fin[blockIdx.x] = t;
      fin[kFinMaxBlocks + blockIdx.x] = (double)zz;
      fin[2 * kFinMaxBlocks + blockIdx.x] = (double)dd;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      const int prev =
          __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = prev == G - 1;
    } else {
      last = 1;
    }
    if (G > 1 && last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      t = 0.0;
      zz = 0;
      dd = 0;
      for (int g = 0; g < G; ++g) {
        t += __hip_atomic_load(&fin[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        zz += (long long)__hip_atomic_load(&fin[kFinMaxBlocks + g], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
        dd |= (int)__hip_atomic_load(&fin[2 * kFinMaxBlocks + g], __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
      }
      *ticket = 0;  // ready for the next call (stream order)
    }
    if (!last) return;
    fin_write(t, zz, dd, status, out, seq, split_rd, split_rs, tree_any, mirror);
  }
}

// One-block calls (n <= kFastBlock trials: an HDDM node's 250, the drop-in's
// per-node call): the level-0 pass of the direct family (fast_level0's
// operations) or of the adaptive families (lean_kernel's), then the finalize
// of the block's <= 4 chunk partials in the same launch, with finalize_kernel's
// exact operations on them (thread k holds partial k, one wave sum, then the
// 16 wave sums added in order, the 15 empty ones as +0.0), so the result and
// the completion word are bit for bit those of the two-launch sequence. The
// chunk partials and zero words are written as usual (a deferred pass after a
// misprediction reads them).
struct FinArgs {
  int* status;
  double* out;
  unsigned long long seq;
  int* tree_any;
  int defer_bits;
};

template <int MODE, int OUT>
__global__ __launch_bounds__(kFastBlock) void small_kernel(TrialArgs A, Work W, RootGrids R,
                                                           FinArgs F) {
  __shared__ double fp[kFastBlock / 64];
  __shared__ int fz[kFastBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = threadIdx.x, c = wv;
  const bool has = c * 64 < A.n;  // wave-uniform
  const bool own = i < A.n;
  double part = 0.0;
  int zw = 0;
  bool tree = false;  // lean: the chunk is left to the redo pass (no partial)
  if (has) {
    double p = 0.0, f0[5];
    long long ne0 = 0;
    unsigned pend0 = 0u;
    int oc = kFinal;
    if constexpr (MODE == kDirect) {
      int flags = 0;
      if (own) oc = fast_level0<MODE>(A.x[i], A.P, A.K, p, f0, ne0, flags, pend0);
      double lp = 0.0;
      int zero = 0;
      if (own && oc == kFinal) emit<OUT>(A, i, p, lp, zero);
      const bool anyd = defer_slots(W, c, lane, oc != kFinal, kFlagExact);
      part = wave_sum(lp);
      zw = __popcll(__ballot(zero != 0)) | (anyd ? kZeroDefer : 0);
    } else {
      const double x0 = own ? A.x[i] : 0.0;
      const bool pos = x0 > 0;
      const unsigned long long bo = __ballot(own), bp = __ballot(own && pos);
      const int b = (bp == bo) ? 1 : 0;
      if (own && pos == (b != 0))
        oc = eng_level0_t<MODE, false, true>(
            trial_setup_b(x0, A.P, b != 0), A.P, A.K, zgrid_uniform(R, b), p, f0, ne0, pend0,
            &R.S[b][0][0]);
      if (bp != 0ull && bp != bo) {
        if (own && pos)
          oc = eng_level0_t<MODE, false, true>(
              trial_setup_b(x0, A.P, true), A.P, A.K, R.G[1], p, f0, ne0, pend0,
              &R.S[1][0][0]);
      }
      if (__ballot(oc == kTree) != 0ull) {
        if (lane == 0) W.redo[c] = 1;  // the host runs the redo pass (lean_kernel)
        part = 0.0;                    // (discarded: the call is reported deferred)
        zw = kZeroDefer;
        tree = true;
      } else {
        double lp = 0.0;
        int zero = 0;
        const bool defer = oc == kExact;
        if (own && !defer) emit<OUT>(A, i, p, lp, zero);
        const bool anyd = defer_slots(W, c, lane, defer, kFlagExact);
        part = wave_sum(lp);
        zw = __popcll(__ballot(zero != 0)) | (anyd ? kZeroDefer : 0);
      }
    }
    if (lane == 0) {
      if (!tree) A.out[c] = part;
      A.zeros[c] = zw;
      fp[wv] = part;
      fz[wv] = zw;
    }
  }
  __syncthreads();
  if (wv != 0) return;
  const int nb = (int)((A.n + 63) / 64);
  double s = 0.0;
  long long z = 0;
  int def = 0;
  if (lane < nb) {
    s += fp[lane];
    z += fz[lane] & (kZeroDefer - 1);
    def |= fz[lane];
  }
  def = F.defer_bits ? (def & kZeroDefer) : 0;
  s = wave_sum(s);
  z = wave_sum_ll(z);
  const bool anyd = __ballot(def != 0) != 0ull;
  if (lane == 0) {
    double t = 0.0;
    long long zz = 0;
    int dd = 0;
    const double ss[2] = {s, 0.0};
    for (int k = 0; k < 16; ++k) {
      t += ss[k == 0 ? 0 : 1];
      zz += k == 0 ? z : 0ll;
      dd |= k == 0 ? (int)anyd : 0;
    }
    fin_write(t, zz, dd, F.status, F.out, F.seq, nullptr, nullptr, F.tree_any, nullptr);
  }
}

// One-block calls of the full DDM (kAdaptTZ: 25 pdf_sv evaluations per
// trial, the per-node drop-in call of HDDM with sv, sz, st) are one wave's
// latency in small_kernel: 64 trials per wave, each lane its trial's 5 t
// nodes in sequence. Here three lanes share a trial (768 threads: 3 waves per
// SIMD, so the generic t-node code fits its registers): lane s of trial k
// evaluates t nodes s and s + 3 (l0_node, the function the split units'
// level-0 tasks use, bit-identical to the per-lane loop) into LDS; then waves
// 0-3 take one trial per lane again (chunk c on wave c), run the root stop
// test and the value from the five values as eng_level0_t does, and continue
// exactly as small_kernel (chunk partials, zero words, deferred slots, the
// finalize), so every output is small_kernel's, bit for bit.
constexpr int kSplitLanes = 3;
constexpr int kSplitBlock = kSplitLanes * kFastBlock;

template <int MODE, int OUT>
__global__ __launch_bounds__(kSplitBlock) void small_split_kernel(TrialArgs A, Work W,
                                                                 RootGrids R, FinArgs F) {
  static_assert(MODE == kAdaptTZ, "t-node split of the full DDM");
  __shared__ double sf[5][kFastBlock];  // t-node values, node-major
  __shared__ int sfl[kSplitLanes][kFastBlock];
  __shared__ unsigned spd[kSplitLanes][kFastBlock];
  __shared__ double fp[kFastBlock / 64];
  __shared__ int fz[kFastBlock / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int k = t / kSplitLanes, sub = t - k * kSplitLanes;  // this lane's trial and share
  const bool own = k < A.n;
  const double x0 = own ? A.x[k] : 0.0;
  const bool pos = x0 > 0;
  const unsigned long long bo = __ballot(own), bp = __ballot(own && pos);
  const int b = (bp == bo) ? 1 : 0;
  int flags = 0;
  unsigned pend = 0u;
  long long ne = 0;
  // pass 1: the lanes of boundary b (a single-boundary wave: all); pass 2: the
  // upper-boundary lanes of a mixed wave (wave-uniform grids, as small_kernel)
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const bool mine = pass == 0 ? (own && pos == (b != 0)) : (bp != 0ull && bp != bo && own && pos);
    if (!mine) continue;
    const int bb = pass == 0 ? b : 1;
    const Trial tr = trial_setup_b(x0, A.P, bb != 0);
    if (!tr.valid) continue;
    double lb, ub;
    tree_root<MODE>(tr, A.P, lb, ub);
    const L0Hints H = l0_hints(tr.x, lb, ub, A.P.a, A.K.err);
#pragma unroll 1
    for (int j = sub; j < 5; j += kSplitLanes) {
      bool pj = false;
      sf[j][k] = l0_node<MODE>(tr, A.P, A.K, lb, ub, H, j, zgrid_uniform(R, bb), flags, pj, ne,
                               &R.S[bb][0][0]);
      if (pj) pend |= 1u << (j * (kTreeW / 4));
    }
  }
  if (own) {
    sfl[sub][k] = flags;
    spd[sub][k] = pend;
  }
  __syncthreads();
  // one trial per lane again: chunk c on wave c (small_kernel's operations)
  if (wv < kFastBlock / 64) {
    const int i = t, c = wv;
    if (c * 64 < A.n) {  // wave-uniform
      const bool own1 = i < A.n;
      int oc = kFinal;
      double p = 0.0;
      if (own1) {
        const double xi = A.x[i];
        int fl = 0;
        unsigned pd = 0u;
#pragma unroll
        for (int q = 0; q < kSplitLanes; ++q) {
          fl |= sfl[q][i];
          pd |= spd[q][i];
        }
        const double f[5] = {sf[0][i], sf[1][i], sf[2][i], sf[3][i], sf[4][i]};
        oc = l0_finish<MODE>(trial_setup_b(xi, A.P, xi > 0), A.P, A.K, fl, pd, f, p);
      }
      double part = 0.0;
      int zw = 0;
      bool tree = false;
      if (__ballot(oc == kTree) != 0ull) {
        if (lane == 0) W.redo[c] = 1;  // the host runs the redo pass (lean_kernel)
        zw = kZeroDefer;
        tree = true;
      } else {
        double lp = 0.0;
        int zero = 0;
        const bool defer = oc == kExact;
        if (own1 && !defer) emit<OUT>(A, i, p, lp, zero);
        const bool anyd = defer_slots(W, c, lane, defer, kFlagExact);
        part = wave_sum(lp);
        zw = __popcll(__ballot(zero != 0)) | (anyd ? kZeroDefer : 0);
      }
      if (lane == 0) {
        if (!tree) A.out[c] = part;
        A.zeros[c] = zw;
        fp[wv] = part;
        fz[wv] = zw;
      }
    }
  }
  __syncthreads();
  if (wv != 0) return;
  const int nb = (int)((A.n + 63) / 64);
  double s = 0.0;
  long long z = 0;
  int def = 0;
  if (lane < nb) {
    s += fp[lane];
    z += fz[lane] & (kZeroDefer - 1);
    def |= fz[lane];
  }
  def = F.defer_bits ? (def & kZeroDefer) : 0;
  s = wave_sum(s);
  z = wave_sum_ll(z);
  const bool anyd = __ballot(def != 0) != 0ull;
  if (lane == 0) {
    double tt = 0.0;
    long long zz = 0;
    int dd = 0;
    const double ss[2] = {s, 0.0};
    for (int q = 0; q < 16; ++q) {
      tt += ss[q == 0 ? 0 : 1];
      zz += q == 0 ? z : 0ll;
      dd |= q == 0 ? (int)anyd : 0;
    }
    fin_write(tt, zz, dd, F.status, F.out, F.seq, nullptr, nullptr, F.tree_any, nullptr);
  }
}

// ---------------------------------------------------------------------------
// Fixed composite Simpson (use_adaptive = 0): one trial per lane, full_pdf +
// settle, per-block {sum, zeros} (OUT_SUM) or per-trial outputs.
template <int MODE, bool COUNT, int OUT>
__global__ __launch_bounds__(kBlock, WFPT_SLOW_WAVES) void trial_kernel(TrialArgs A) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  long long ne = 0;
  double lp = 0.0;
  int zero = 0, flags = 0;
  if (i < A.n) {
    const double x = A.x[i];
    double p = full_pdf<MODE, RegStack<2>>(x, A.P, A.K, ne, flags);
    p = settle(p, x, A.P, A.K, !trial_setup(x, A.P).valid, ne, flags);
    if (flags & kFlagErrors) atomicOr(A.status, flags & kFlagErrors);
    emit<OUT>(A, i, p, lp, zero);
  }
  if (sum_out(OUT) || COUNT) {
    block_reduce<COUNT>(lp, zero, ne);
    if (threadIdx.x == 0) {
      if (sum_out(OUT)) {
        A.out[blockIdx.x] = lp;
        A.zeros[blockIdx.x] = zero;
      }
      if (COUNT) atomicAdd(A.evals, (unsigned long long)ne);
    }
  }
}

// wiener_like_multi (wfpt.pyx:244-274): per-trial parameters, ±999 = missing.
template <int STK>
__global__ __launch_bounds__(kBlock, WFPT_SLOW_WAVES) void multi_kernel(
    const double* x, int64_t n, const double* const* arr, const double* scal, Knobs K,
    double p_outlier, double* out, int* zeros, int* status, double* lpo) {
  using Stack = typename StackOf<STK>::type;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double lp = 0.0;
  int zero = 0, flags = 0;
  long long ne = 0;
  if (i < n) {
    double q[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = arr[j] ? arr[j][i] : scal[j];
    Params Q;
    Q.v = q[0];
    Q.sv = q[1];
    Q.a = q[2];
    Q.z = q[3];
    Q.sz = q[4];
    Q.t = q[5];
    Q.st = q[6];
    Q.p_outlier = p_outlier;
    const double xi = x[i];
    double p;
    if (fabs(xi) != 999.) {
      // out of line, as node_kernel's three callers of the same walk keep it
      // (this unit's only caller would inline 45k instructions and 1.6 KB more scratch)
      [[clang::noinline]] p = full_pdf<kRuntime, Stack>(xi, Q, K, ne, flags);
      p = settle(p, xi, Q, K, !trial_setup(xi, Q).valid, ne, flags);
      if (flags & kFlagErrors) atomicOr(status, flags & kFlagErrors);
      p = p * (1 - p_outlier) + (K.w_outlier * p_outlier);
    } else if (xi == 999.) {
      p = prob_ub(Q.v, Q.a, Q.z);
    } else {
      p = 1 - prob_ub(Q.v, Q.a, Q.z);
    }
    // the reference has no early exit here: log(0) = -inf enters the sum
    lp = log_val(p);
    if (lpo) lpo[i] = lp;
  }
  block_reduce<false>(lp, zero, ne);
  if (threadIdx.x == 0) {
    out[blockIdx.x] = lp;
    zeros[blockIdx.x] = 0;
  }
}

// Copies a device result {sum, zeros, errors} (after the RCCL all-reduce) to
// the mapped host slot, then writes the completion word.
__global__ __launch_bounds__(64) void publish_kernel(const double* res, double* out,
                                                     unsigned long long seq) {
  if (threadIdx.x == 0) {
    out[0] = res[0];
    out[1] = res[1];
    out[2] = res[2];
    out[3] = res[3];
    out[5] = res[5];
    out[6] = res[6];
    publish_word(reinterpret_cast<unsigned long long*>(out) + 4, seq);
  }
}

void launch_publish(const double* res, double* out, unsigned long long seq, hipStream_t s) {
  hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, s, res, out, seq);
}

__global__ __launch_bounds__(64) void poison_kernel(double* res) {
  if (threadIdx.x < 8) res[threadIdx.x] = threadIdx.x == 2 ? kPeerFailUnit : 0.0;
}

void launch_poison(double* res, hipStream_t s) {
  hipLaunchKernelGGL(poison_kernel, dim3(1), dim3(64), 0, s, res);
}

// ---------------------------------------------------------------------------
// launchers

int stack_kind(const Knobs& K) {
  const int d = (K.n_st > K.n_sz) ? K.n_st : K.n_sz;
  return d <= 2 ? 0 : (d <= 4 ? 1 : 2);
}

int64_t blocks_for(int64_t n) { return (n + kBlock - 1) / kBlock; }

bool has_deferred_pass(const Params& P, const Knobs& K) {
  return select_mode(P.sz, P.st, K.use_adaptive) <= kAdaptTZ;
}

int64_t partials_for(int64_t n, const Params& P, const Knobs& K) {
  return has_deferred_pass(P, K) ? (n + 63) / 64 : blocks_for(n);
}

static void launch_fixed(int mode, bool count, int out, const TrialArgs& A, hipStream_t s) {
  with_value<kFixedT, kFixedTZ>(mode, [&](auto m) {
    with_build<true>(count, out, [&](auto c, auto o) {
      hipLaunchKernelGGL((trial_kernel<decltype(m)::value, decltype(c)::value, decltype(o)::value>),
                         dim3(blocks_for(A.n)), dim3(kBlock), 0, s, A);
    });
  });
}

// evals selects a counting build for OUT_SUM only: OUT_ARRAY and OUT_BOTH are
// non-counting (with_build lists the builds that exist).
void launch_trials(int out_kind, int part, const double* x, int64_t n, const Params& P,
                   const Knobs& K, double* out, int* zeros, unsigned long long* evals, int* status,
                   int logp, const Work& W, hipStream_t s, hipEvent_t fast_done,
                   const Split* split, double* trial, const DecisionTab* dtab,
                   const LeanFirst* first) {
  if (n <= 0) return;
  Split S{};
  if (split) S = *split;
  const TrialArgs A = trial_args(x, n, P, K, out, zeros, evals, status, logp, trial);
  const int mode = select_mode(P.sz, P.st, K.use_adaptive);
  const bool count = evals && out_kind == OUT_SUM;
  if (mode > kAdaptTZ) {
    launch_fixed(mode, count, out_kind, A, s);
    if (fast_done) (void)hipEventRecord(fast_done, s);
    return;
  }
  // the engine's tables (the lean pass alone needs only its root grids)
  EngTables T;
  const bool engine = ((part & kPassFast) && !(part & kPassLean)) || (part & kPassRedo);
  if (mode != kDirect && engine) eng_tables(A.P, T);
  // W.redo is live only in the lean and redo passes (a full engine
  // launch processes every chunk); the host never combines kPassRedo with a
  // full engine level-0 pass
  Work F = W;
  F.redo = (part & (kPassLean | kPassRedo)) ? W.redo : nullptr;
  if (part & kPassFast) {
    if (mode == kDirect) launch_direct(count, out_kind, A, F, s);
    else if (part & kPassLean) launch_lean(mode, count, out_kind, A, F, s, dtab, first);
    else launch_engine(mode, count, out_kind, A, F, T, S, s);
    if (fast_done) (void)hipEventRecord(fast_done, s);
  }
  if (part & kPassDeferred) {
    // the engine over the chunks the lean pass flagged (one wave each)
    if (mode != kDirect && (part & kPassRedo)) launch_engine(mode, count, out_kind, A, F, T, Split{}, s);
    launch_fold(mode, count, out_kind, A, F, s);
  }
}

int launch_small(const double* x, int64_t n, const Params& P, const Knobs& K, double* part,
                 int* zeros, int* status, const Work& W, double* out, unsigned long long seq,
                 int* tree_any, hipStream_t s, double* trial) {
  if (n <= 0 || n > kFastBlock) return kSmallNone;
  const int mode = select_mode(P.sz, P.st, K.use_adaptive);
  if (mode > kAdaptTZ) return kSmallNone;
  const TrialArgs A = trial_args(x, n, P, K, part, zeros, nullptr, status, 0, trial);
  Work F = W;
  F.redo = mode == kDirect ? nullptr : W.redo;
  RootGrids R{};
  if (mode != kDirect) root_grids(P, R);
  const FinArgs Fa{status, out, seq, tree_any, 1};
  with_build<false>(false, trial ? OUT_BOTH : OUT_SUM, [&](auto, auto o) {
    constexpr int O = decltype(o)::value;
    if (mode == kAdaptTZ)
      hipLaunchKernelGGL((small_split_kernel<kAdaptTZ, O>), dim3(1), dim3(kSplitBlock), 0, s, A, F,
                         R, Fa);
    else
      with_value<kDirect, kAdaptZ>(mode, [&](auto m) {
        hipLaunchKernelGGL((small_kernel<decltype(m)::value, O>), dim3(1), dim3(kFastBlock), 0, s,
                           A, F, R, Fa);
      });
  });
  return mode == kAdaptTZ ? kSmallSplit : kSmallOne;
}

void launch_multi(const double* x, int64_t n, const double* const* arr, const double* scal,
                  const Knobs& K, double p_outlier, double* part, int* zeros, int* status,
                  hipStream_t s, double* lp) {
  const int64_t nb = blocks_for(n);
  if (nb == 0) return;
  with_value<0, 2>(stack_kind(K), [&](auto stk) {
    hipLaunchKernelGGL((multi_kernel<decltype(stk)::value>), dim3(nb), dim3(kBlock), 0, s, x, n,
                       arr, scal, K, p_outlier, part, zeros, status, lp);
  });
}

void launch_finalize(const double* part, const int* zeros, int64_t nb, int defer_bits,
                     int* status, double* out, unsigned long long seq, hipStream_t s,
                     const int* split_rd, int* split_rs, int* tree_any, double* mirror,
                     double* fin, int* ticket) {
  int64_t g = 1;
  if (fin && ticket && nb > 2 * kFinPerBlock)
    g = std::min<int64_t>(kFinMaxBlocks, (nb + kFinPerBlock - 1) / kFinPerBlock);
  hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)g), dim3(1024), 0, s, part, zeros, nb,
                     defer_bits, status, out, seq, split_rd, split_rs, tree_any, mirror, fin,
                     ticket);
}

}  // namespace wfpt
