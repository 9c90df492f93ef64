// wfpt_engine.hip — the kernels built on the in-wave refinement engine
// (wfpt_engine.hpp) on gfx950, and the per-trial-parameter path they serve:
//   engine_kernel<MODE>   level 0 + in-wave refinement rounds (z walks, t-node
//                         tasks, tree17) of a chunk per wave; heavy chunks
//                         recorded by the previous call run as 8 split units
//   wiener_like_multi with a uniform family (launch_multi_fast):
//   multi_fast_kernel<MODE> (level 0 per lane) + multi_records_kernel<MODE>
//   (one wave per deferred record; the direct family's rare exact-path
//   records: multi_direct_records_kernel) + lp_sum_kernel.
// The two share a unit because engine_kernel<kAdaptT> compiles to the code it
// always had only next to the per-trial path's kAdaptT instantiations.
#include "wfpt_engine.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// ---------------------------------------------------------------------------
// The engine of the adaptive families (kAdaptT, kAdaptZ, kAdaptTZ;
// integrate.pxi:72-206 driven by pdf.pxi:132-146). One wave owns a chunk of 64
// consecutive trials and completes their quadrature trees, up to kTreeDepth
// refinement levels per axis (HDDM's n_st = n_sz = 2):
//   * level 0 runs in registers, each lane its own trial (fast_level0: its
//     root interval's 5 t nodes with shared series decisions and the q
//     recurrence, or its root z grid); a chunk none of whose trials refines
//     ends there;
//   * refinement runs in rounds (refine_rounds). A task is one evaluation of a
//     trial's integrand at one t node: a 5-wide z grid (kAdaptZ, kAdaptTZ:
//     tnode_pdf_sv_grid5) or one pdf_sv (kAdaptT). The stop tests of level L
//     (each lane its own tree: tree17, the reference's recursion in
//     straight-line form over the values in registers) queue level L + 1's
//     tasks in LDS, and each round gives every lane of the team one task;
//   * kAdaptTZ: a t node whose z integral asks for refinement queues a z walk:
//     4 lanes evaluate its 4 z grids (the root again, L1, L2L, L2R: every z
//     node a depth-2 walk can reach), then one lane runs tree17 over the z
//     tree's 17 values;
//   * every evaluation of the rounds goes through one code site.
// Heavy chunks: a chunk whose level 0 leaves more than kHeavyZ z walks (the
// shortest RTs, where every t node's z integral refines) would serialise
// tens of rounds in one wave and set the launch's length. On a resident
// dataset the engine records such chunks (Split, next_*); the following call
// runs each of them as kSplit units of kSplitTrials trials, one wave each,
// dispatched first: the unit's level 0 runs as tasks (l0_node, bit-identical
// to the per-lane loop) and its refinement spreads over the whole wave. The
// last unit of a chunk to finish folds the chunk's per-trial terms in the
// same order wave_sum uses, so a chunk's partial does not depend on whether
// it was split (likelihoods stay bitwise reproducible across call histories).
// Trials whose value hinges on last-bit rounding (kFlagExact) or whose tree is
// deeper (kFlagFallback) become deferred slots for fold_kernel.

// Waves per SIMD the engine kernel is built for (its LDS, 4 x 13.4 KB per
// block, allows 3; its registers fit 2 without spilling)
#ifndef WFPT_ENG_WAVES
#define WFPT_ENG_WAVES 2
#endif
// Heavy chunks: more than kHeavyZ z walks after level 0 (class 1). A chunk
// with more than kHeavyZ z walks over all its levels (not after level 0
// alone) is heavy too: class 2, split while the dataset has few heavy
// chunks (Split::n2)
constexpr int kHeavyZ = 96;

__device__ inline void tally_out(const Work& W, const Tally& ty) {
  atomicAdd(&W.prof[1], ty.t1);
  atomicAdd(&W.prof[2], ty.t2);
  atomicAdd(&W.prof[4], ty.rec);
  atomicAdd(&W.prof[7], ty.z[0] + ty.z[1] + ty.z[2]);
  atomicAdd(&W.prof[8], ty.z[0]);
  atomicAdd(&W.prof[9], ty.z[1]);
  atomicAdd(&W.prof[10], ty.z[2]);
}

// Records chunk c for the next call's split (lane 0 of its last wave).
__device__ inline void record_heavy(const Split& S, int64_t c, int cls) {
  if (!S.next_pred) return;
  unsigned char flag = 0;
  if (cls) {
    const int half = S.cap / 2;
    const int slot = atomicAdd(S.next_n + (cls == 2 ? 2 : 0), 1);
    if (slot < half) {
      S.next_list[(cls == 2 ? half : 0) + slot] = (int)c;
      flag = (unsigned char)cls;
    }
  }
  S.next_pred[c] = flag;
}
// Heavy class of a chunk from its z walks after level 0 (z0) and over all
// levels (zt): 1, 2 or 0.
__device__ inline int heavy_class(int z0, int zt) {
  return z0 > kHeavyZ ? 1 : (zt > kHeavyZ ? 2 : 0);
}

// Chunk outputs of a split unit's trials: per-trial outputs now, the chunk
// partial's terms to S.lp / S.meta; the chunk's last unit (agent-scope
// release / acquire hand-off) folds them in wave_sum's order and writes the
// chunk's deferred slots in lane order, exactly as an unsplit chunk's wave.
template <int MODE, bool COUNT, int OUT>
__device__ inline void split_out(const TrialArgs& A, const Work& W, const Split& S,
                                 const ChunkLds<1>& cl, int slot, int sub, int lane, double x0,
                                 int nz0, int nzt) {
  const int64_t c = S.list[slot < S.n ? slot : S.cap / 2 + (slot - S.n)];
  const int64_t i = c * 64 + sub * kSplitTrials + lane;
  const bool own = lane < kSplitTrials && i < A.n;
  double p = 0.0, lp = 0.0;
  bool defer = false;
  int rf = kFlagExact, zero = 0;
  if (own && !(cl.fl[lane] & kFlagIdle)) tree_density<MODE, 1>(A, cl, lane, x0, p, defer, rf);
  if (own && !defer) emit<OUT>(A, i, p, lp, zero);  // invalid parameters: p = 0
  if (lane < kSplitTrials) {
    const int k = slot * 64 + sub * kSplitTrials + lane;
    S.lp[k] = lp;
    S.meta[k] = zero | ((int)defer << 1) | (rf << 2);
  }
  if (COUNT) {
    const long long nf = wave_sum_ll((own && !defer) ? (long long)cl.cnt[lane] : 0ll);
    if (lane == 0) atomicAdd(A.evals, (unsigned long long)nf);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int prev = 0;
  if (lane == 0) {
    atomicAdd(&S.zn[slot], nz0 + (nzt << 16));
    prev = __hip_atomic_fetch_add(&S.done[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  prev = __shfl(prev, 0, 64);
  if (prev != kSplit - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const double lpc = S.lp[slot * 64 + lane];
  const int m = S.meta[slot * 64 + lane];
  const bool anyd = defer_slots(W, c, lane, (m >> 1) & 1, m >> 2);
  if (sum_out(OUT)) {
    const double sum = wave_sum(lpc);
    const int zs = __popcll(__ballot((m & 1) != 0));
    if (lane == 0) {
      A.out[c] = sum;
      A.zeros[c] = zs | (anyd ? kZeroDefer : 0);
    }
  }
  if (lane == 0) {
    const int znc = __hip_atomic_load(&S.zn[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    record_heavy(S, c, heavy_class(znc & 0xffff, znc >> 16));
    S.done[slot] = 0;
    S.zn[slot] = 0;
  }
}

template <int MODE, bool COUNT, int OUT>
__global__ __launch_bounds__(kEngBlock, WFPT_ENG_WAVES) void engine_kernel(TrialArgs A, Work W, EngTables tab,
                                                              Split S) {
  __shared__ ChunkLds<1> lds[kEngWaves];
  const int lane = threadIdx.x & 63;
  ChunkLds<1>& cl = lds[threadIdx.x >> 6];
  PhaseClock pc;
  pc.start();
#ifdef WFPT_PHASE_TIMING
  const long long rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  // work units: the split chunks' units first (dispatched first), then one
  // wave per chunk
  const int64_t u = (int64_t)blockIdx.x * kEngWaves + (threadIdx.x >> 6);
  const int ns = S.n + S.n2;  // split chunks: class 1's units, then class 2's
  const bool split = u < (int64_t)ns * kSplit;
  const int slot = split ? (int)(u / kSplit) : 0, sub = split ? (int)(u % kSplit) : 0;
  const int64_t c = split ? (int64_t)S.list[slot < S.n ? slot : S.cap / 2 + (slot - S.n)]
                          : u - (int64_t)ns * kSplit;
  // past the end / split in this call (class 2 only while n2 > 0)
  if (!split && (c * 64 >= A.n ||
                 (ns > 0 && (S.pred[c] == 1 || (S.pred[c] == 2 && S.n2 > 0)))))
    return;
  if (W.redo && !W.redo[c]) return;  // redo pass: only the chunks the lean pass flagged
  load_tables(cl, tab, lane);
  const int64_t i = split ? c * 64 + sub * kSplitTrials + lane : c * 64 + lane;
  const bool own = (split ? lane < kSplitTrials : true) && i < A.n;
  const double x0 = own ? A.x[i] : 0.0;
  wave_sync();
  double p = 0.0;
  long long ne0 = 0;
  int oc = kFinal, stage = 1;
  bool rounds;
  if (!split) {
    // ---- level 0, each lane its own trial, in registers ----
    double f0[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    unsigned pend0 = 0u;
    if (own) {
      const ZGrid G = cl.tab.G[x0 > 0][kGridRoot];
      oc = eng_level0<MODE>(x0, A.P, A.K, G, p, f0, ne0, pend0);
    }
    pc.mark(0);
    rounds = __ballot(oc == kTree) != 0ull;
    if (rounds) {
      cl.X[lane] = x0;
      cl.fl[lane] = oc == kTree ? 0 : (oc == kExact ? (int)kFlagExact : (int)kFlagIdle);
      if (COUNT) cl.cnt[lane] = (int)ne0;
      if (oc == kTree) {
#pragma unroll
        for (int j = 0; j < 5; ++j) cl.F[j * (kTreeW / 4) * 64 + lane] = f0[j];
      }
      if (lane == 0) {
        cl.qn[0] = 0;
        cl.qn[1] = 0;
      }
      wave_sync();
      // the pending z integrals of the refining trials (kAdaptTZ)
      if (MODE == kAdaptTZ) {
#pragma unroll
        for (int j = 0; j < 5; ++j)
          team_push(oc == kTree && ((pend0 >> (j * (kTreeW / 4))) & 1u),
                    lane | ((j * (kTreeW / 4)) << 6), cl.ZQ, &cl.qn[1]);
      }
    }
  } else {
    // ---- a split unit: its kSplitTrials trials' level 0 as tasks (t node j
    // of owner o, or owner o's root z grid) ----
    cl.X[lane] = x0;
    cl.fl[lane] = (own && trial_setup(x0, A.P).valid) ? 0 : kFlagIdle;
    if (COUNT) cl.cnt[lane] = 0;
    if (lane == 0) {
      cl.qn[0] = 0;
      cl.qn[1] = 0;
    }
    wave_sync();
    constexpr int n0 = (MODE == kAdaptZ) ? 1 : 5;
    const int o = lane % kSplitTrials, j = lane / kSplitTrials;
    team_push(j < n0 && !(cl.fl[o] & kFlagStop), o | ((j * (kTreeW / 4)) << 6), cl.Q, &cl.qn[0]);
    stage = 0;
    rounds = true;
  }
  Tally ty;
  int nz0 = 0, nzt = 0;
  if (rounds) {
    // chunks that refined in-wave (a split chunk once: its unit 0); finalize
    // reports the count, which picks the next call's level-0 pass
    if (lane == 0 && (!split || sub == 0)) atomicAdd(W.tree_any, 1);
    wave_sync();
    nz0 = cl.qn[1];
    pc.mark(1);
    refine_rounds<MODE, COUNT, 1>(A, cl, lane, stage, ty, pc);
    if (split) nz0 = ty.z[0];
    nzt = ty.z[0] + ty.z[1] + ty.z[2];  // the z walks of every level
  }
  if (split) {
    split_out<MODE, COUNT, OUT>(A, W, S, cl, slot, sub, lane, x0, nz0, nzt);
    if (COUNT && lane == 0) tally_out(W, ty);
#ifdef WFPT_PHASE_TIMING
    // split units in the upper half of the records (unit u at kPhaseWaves / 2 + u)
    if (lane == 0 && u < kPhaseWaves / 2) {
      unsigned long long* rec = W.phase + (kPhaseWaves / 2 + u) * 8;
      rec[0] = rt0;
      rec[1] = __builtin_amdgcn_s_memrealtime();
      for (int k = 0; k < 5; ++k) rec[2 + k] = pc.ph[k];
      rec[7] = (unsigned long long)pc.nz | ((unsigned long long)pc.nt << 32);
    }
#endif
    return;
  }
  if (lane == 0) {
    record_heavy(S, c, heavy_class(nz0, nzt));
    if (W.redo) W.redo[c] = 0;
  }
  bool defer = oc == kExact;
  int rf = kFlagExact;
  if (oc == kTree) tree_density<MODE, 1>(A, cl, lane, x0, p, defer, rf);
  chunk_out<COUNT, OUT>(A, W, c, lane, p, defer, rf, oc == kTree ? (long long)cl.cnt[lane] : ne0);
  pc.mark(4);
#ifdef WFPT_PHASE_TIMING
  if (lane == 0 && c < kPhaseWaves / 2) {
    unsigned long long* rec = W.phase + c * 8;
    rec[0] = rt0;
    rec[1] = __builtin_amdgcn_s_memrealtime();
    for (int k = 0; k < 5; ++k) rec[2 + k] = pc.ph[k];
    rec[7] = (unsigned long long)pc.nz | ((unsigned long long)pc.nt << 32);
  }
#endif
  if (COUNT && lane == 0) tally_out(W, ty);
}

// The deferred records of multi_fast_kernel, adaptive families: one wave per
// record (node_records with wiener_like_multi's term).
template <int MODE, bool COUNT>
__global__ __launch_bounds__(kEngBlock, 2) void multi_records_kernel(
    const double* x, Knobs K, double* lp, const int64_t* d_idx, const Params* d_par,
    const int* n_defer, unsigned long long* evals, int* status) {
  __shared__ ChunkLds<1> lds[kEngWaves];
  const int lane = threadIdx.x & 63;
  node_records<MODE, COUNT, true>(
      lds[threadIdx.x >> 6], lane,
      __builtin_amdgcn_readfirstlane((int)blockIdx.x * kEngWaves + (int)(threadIdx.x >> 6)),
      (int)gridDim.x * kEngWaves, x, K, lp, d_idx, d_par, *n_defer, evals, status);
}

// S's split units first, then one wave per chunk.
void launch_engine(int mode, bool count, int out, const TrialArgs& A, const Work& W,
                   const EngTables& T, const Split& S, hipStream_t s) {
  const int64_t units = (int64_t)(S.n + S.n2) * kSplit + (A.n + 63) / 64;
  with_value<kAdaptT, kAdaptTZ>(mode, [&](auto m) {
    with_build<true>(count, out, [&](auto c, auto o) {
      hipLaunchKernelGGL(
          (engine_kernel<decltype(m)::value, decltype(c)::value, decltype(o)::value>),
          dim3((units + kEngWaves - 1) / kEngWaves), dim3(kEngBlock), 0, s, A, W, T, S);
    });
  });
}

// multi_fast_kernel's deferred records of the adaptive families, one wave
// each. (Instantiated here, next to engine_kernel: where the compiler meets
// these instantiations decides whether engine_kernel<kAdaptT> and
// multi_records_kernel<kAdaptT> come out as they always have.)
static void launch_multi_records(int mode, bool count, const double* x, int64_t n, const Knobs& K,
                                 double* lp, const int64_t* d_idx, const Params* d_par,
                                 const int* n_defer, unsigned long long* evals, int* status,
                                 hipStream_t s) {
  const int64_t nb = std::min<int64_t>(std::max<int64_t>((n + kEngBlock - 1) / kEngBlock, 1), 256);
  with_value<kAdaptT, kAdaptTZ>(mode, [&](auto m) {
    with_flag(count, [&](auto c) {
      hipLaunchKernelGGL((multi_records_kernel<decltype(m)::value, decltype(c)::value>), dim3(nb),
                         dim3(kEngBlock), 0, s, x, K, lp, d_idx, d_par, n_defer, evals, status);
    });
  });
}

// ---------------------------------------------------------------------------
// Per-trial parameters (wiener_like_multi), uniform family.

// The deferred records of multi_fast_kernel, direct family (the rare
// exact-path trials), one lane each: wiener_like_multi's trial term
// (wfpt.pyx:266-272: the mixture with the call's p_outlier and a plain log,
// no range check).
template <bool COUNT>
__global__ __launch_bounds__(64, WFPT_SLOW_WAVES) void multi_direct_records_kernel(
    const double* x, Knobs K, double* lp, const int64_t* d_idx, const Params* d_par,
    const int* n_defer, unsigned long long* evals, int* status) {
  const int nd = *n_defer;
  long long ne = 0;
  int flags = 0;
  for (int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x; k < nd; k += (int64_t)gridDim.x * 64) {
    const int64_t i = d_idx[k];
    const Params Q = d_par[k];
    long long n1 = 0;
    int f1 = 0;
    double p = full_pdf<kDirect, RegStack<2>>(x[i], Q, K, n1, f1);
    if (f1 & kFlagExact) p = __builtin_nan("");  // near-tie: settled exactly below
    flags |= f1 & kFlagErrors;
    p = settle(p, x[i], Q, K, false, n1, flags);
    ne += n1;
    lp[i] = log_val(p * (1 - Q.p_outlier) + (K.w_outlier * Q.p_outlier));
  }
  if (flags & kFlagErrors) atomicOr(status, flags & kFlagErrors);
  if (COUNT) {
    ne = wave_sum_ll(ne);
    if (threadIdx.x == 0) atomicAdd(evals, (unsigned long long)ne);
  }
}

// wiener_like_multi's level-0 pass when the integration family is uniform
// (sz and st are scalars, adaptive): one trial per lane with its own
// parameters (per-trial arrays, or the scalars), the same fast_level0 as the
// per-node path; trials whose root test refines (or hinge on rounding) go to
// the records kernels above as (index, parameter row) records. |x| = 999
// trials are scored by prob_ub (wfpt.pyx:267-271). lp[i] = the trial's term.
template <int MODE, bool COUNT>
__global__ __launch_bounds__(kBlock, FastWaves<MODE>::value > 0 ? FastWaves<MODE>::value : 1)
void multi_fast_kernel(const double* x, int64_t n, const double* const* arr, const double* scal,
                       Knobs K, double p_outlier, double* lp, int64_t* d_idx, Params* d_par,
                       int* n_defer, unsigned long long* evals) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  long long ne = 0;
  bool defer = false;
  Params Q;
  if (i < n) {
    double q[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = arr[j] ? arr[j][i] : scal[j];
    Q.v = q[0];
    Q.sv = q[1];
    Q.a = q[2];
    Q.z = q[3];
    Q.sz = q[4];
    Q.t = q[5];
    Q.st = q[6];
    Q.p_outlier = p_outlier;
    const double xi = x[i];
    if (fabs(xi) != 999.) {
      double p, f[5];
      int flags = 0;
      unsigned pend;
      const int oc = fast_level0<MODE>(xi, Q, K, p, f, ne, flags, pend);
      if (oc == kFinal) lp[i] = log_val(p * (1 - p_outlier) + (K.w_outlier * p_outlier));
      else defer = true;
    } else {
      const double pu = prob_ub(Q.v, Q.a, Q.z);
      lp[i] = log_val(xi == 999. ? pu : 1 - pu);
    }
  }
  const unsigned long long b = __ballot(defer);
  if (b) {
    int base = 0;
    if (lane == 0) base = atomicAdd(n_defer, __popcll(b));
    base = __shfl(base, 0, 64);
    if (defer) {
      const int k = base + __popcll(b & lanemask_lt(lane));
      d_idx[k] = i;
      d_par[k] = Q;
    }
  }
  if (COUNT) {
    ne = wave_sum_ll(defer ? 0 : ne);
    if (lane == 0) atomicAdd(evals, (unsigned long long)ne);
  }
}

// Fixed-order per-block sums of per-trial terms (finalize adds the blocks).
__global__ __launch_bounds__(kBlock) void lp_sum_kernel(const double* lp, int64_t n, double* part,
                                                        int* zeros) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double s = i < n ? lp[i] : 0.0;
  int zero = 0;
  long long ne = 0;
  block_reduce<false>(s, zero, ne);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s;
    zeros[blockIdx.x] = 0;
  }
}

template <int MODE, bool COUNT>
static void launch_multi_two_pass(const double* x, int64_t n, const double* const* arr,
                                  const double* scal, const Knobs& K, double p_outlier, double* lp,
                                  int64_t* d_idx, Params* d_par, int* n_defer,
                                  unsigned long long* evals, int* status, hipStream_t s) {
  hipLaunchKernelGGL((multi_fast_kernel<MODE, COUNT>), dim3(blocks_for(n)), dim3(kBlock), 0, s, x,
                     n, arr, scal, K, p_outlier, lp, d_idx, d_par, n_defer, evals);
  if constexpr (MODE != kDirect) {
    // adaptive families: one wave per deferred record
    launch_multi_records(MODE, COUNT, x, n, K, lp, d_idx, d_par, n_defer, evals, status, s);
  } else {
    // direct family: only exact-path records, one lane each
    const int64_t nl = (n + 63) / 64;
    const int64_t g = nl < 64 ? nl : 64;  // rare exact-path records; kilobytes of scratch per lane
    hipLaunchKernelGGL((multi_direct_records_kernel<COUNT>), dim3(g), dim3(64), 0, s, x, K, lp,
                       d_idx, d_par, n_defer, evals, status);
  }
}

void launch_multi_fast(int mode, const double* x, int64_t n, const double* const* arr,
                       const double* scal, const Knobs& K, double p_outlier, double* lp,
                       int64_t* d_idx, Params* d_par, int* n_defer, double* part, int* zeros,
                       unsigned long long* evals, int* status, hipStream_t s) {
  with_mode(mode, [&](auto m) {
    with_flag(evals != nullptr, [&](auto c) {
      launch_multi_two_pass<decltype(m)::value, decltype(c)::value>(
          x, n, arr, scal, K, p_outlier, lp, d_idx, d_par, n_defer, evals, status, s);
    });
  });
  hipLaunchKernelGGL(lp_sum_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, lp, n, part, zeros);
}

}  // namespace wfpt
