// wfpt_level0.hip — the level-0 passes of a resident call on gfx950:
//   direct_kernel        the simple DDM (one pdf_sv per trial)
//   lean_kernel<MODE>    level 0 of every trial of the adaptive families, one
//                        64-trial chunk per wave; a chunk that refines is
//                        flagged for the engine's redo pass (wfpt_engine.hip).
//                        The 2-D family has two sites: waves whose lanes agree
//                        on every t node's series decision (lean_uniform_level0,
//                        wfpt_lean.hpp) and the per-lane one (eng_level0_t).
//                        A wave learns that its lanes agree from the decision's
//                        breakpoint table (table_decisions: its two extreme
//                        |rt| looked up) or, where the table has no answer,
//                        from every lane's own fp32 estimate and a vote
//                        (l0_decisions). Static counts from the assembly with
//                        line tables (hipcc -S -gline-tables-only): the table
//                        stage issues ~62 VALU per lane (35 in
//                        table_decisions, 27 in the kernel's lines around it,
//                        the 1 / a^2 division among them), the per-lane
//                        pre-pass 170 to 410
// (One-block calls run level 0 and the finalize in one launch: wfpt_sum.hip.)
#include "wfpt_kernel_common.hpp"
#include "wfpt_lean.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// Direct family (sz = st = 0): one pdf_sv per trial, one chunk of 64 trials
// per wave. The level-0 pass takes the call's per-boundary constants
// (DirectArgs: v, w, sin / 2cos(pi w), (-v) a w, 1 / a^2 computed once on the
// host) instead of per-lane flips, sincospi and a division: the same outputs
// as fast_level0<kDirect> bit for bit (direct_level0). As in the lean pass, a
// wave's trials are taken by boundary (datasets are ordered by boundary, then
// |rt|), so the constants are wave-uniform; only the wave at the boundary
// switch takes the second call site.
template <bool COUNT, int OUT>
__global__ __launch_bounds__(kFastBlock, FastWaves<kDirect>::value > 0 ? FastWaves<kDirect>::value : 1)
void direct_kernel(TrialArgs A, Work W, DirectArgs D) {
  const int64_t i = (int64_t)blockIdx.x * kFastBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t c = i >> 6;
  if (c * 64 >= A.n) return;  // a wave past the last chunk (wave-uniform)
  const bool own = i < A.n;
  const double x0 = own ? A.x[i] : 0.0;
  double p = 0.0;
  long long ne = 0;
  int flags = 0, oc = kFinal;
  const bool pos = x0 > 0;
  const unsigned long long bo = __ballot(own), bp = __ballot(own && pos);
  const int b = (bp == bo) ? 1 : 0;  // every trial upper: 1; otherwise lower first
  if (own && pos == (b != 0)) oc = direct_level0(x0, A.P, A.K, D, b, p, ne, flags);
  if (bp != 0ull && bp != bo) {  // mixed wave: its upper-boundary lanes
    if (own && pos) oc = direct_level0(x0, A.P, A.K, D, 1, p, ne, flags);
  }
  double lp = 0.0;
  int zero = 0;
  if (own && oc == kFinal) emit<OUT>(A, i, p, lp, zero);
  const bool anyd = defer_slots(W, c, lane, oc != kFinal, kFlagExact);
  if (sum_out(OUT)) {
    lp = wave_sum(lp);
    const int zs = __popcll(__ballot(zero != 0));
    if (lane == 0) {
      A.out[c] = lp;
      A.zeros[c] = zs | (anyd ? kZeroDefer : 0);
    }
  }
  if (COUNT) {
    const long long nf = wave_sum_ll(oc == kFinal ? ne : 0);
    if (lane == 0) atomicAdd(A.evals, (unsigned long long)nf);
  }
}

// The engine's level 0 alone (kPassLean), for resident datasets whose last
// call refined no chunk in-wave (the usual MCMC case at HDDM's knobs): no LDS,
// no refinement code, so the register allocation and occupancy are those of
// level 0 (FastWaves) instead of the engine's. Each lane runs eng_level0 on
// the table's root z grid, i.e. the same operations on the same inputs as the
// engine's level 0, and a chunk without refining trials leaves the bits the
// engine would (chunk_out). A chunk with a refining trial writes nothing but
// its redo flag and a nonzero deferred count; the engine's redo pass
// (kPassRedo) then processes it from scratch, as a full engine call would.
// Block size of the lean pass (WFPT_LEAN_BLOCK; its waves are independent:
// one chunk each, no block-level exchange). The launch bound's second
// argument is waves per SIMD (amdgpu_waves_per_eu), independent of the block
// size, so the register budget is the same for every block size.
#ifndef WFPT_LEAN_BLOCK
#define WFPT_LEAN_BLOCK 256
#endif
constexpr int kLeanBlock = WFPT_LEAN_BLOCK;
static_assert(kLeanBlock % 64 == 0 && kLeanBlock <= kFastBlock, "kLeanBlock");
static_assert(sizeof(TrialArgs) + sizeof(Work) + sizeof(RootGrids) + sizeof(UniformTabs) +
                      sizeof(DecisionTab) + sizeof(LeanFirst) <= 4096,
              "lean_kernel's arguments exceed the 4 KB kernel argument segment");
// FIRST: the build that reads the list F (launched only with F.n > 0). The
// list's prologue keeps values live that move the kernel's scalar register
// allocation (sgpr_spill_count 62 -> 82), so a launch without a list runs
// the build without it, whose stream is the one before the list existed.
template <int MODE, bool COUNT, int OUT, bool FIRST>
__global__ __launch_bounds__(kLeanBlock, FastWaves<MODE>::value > 0 ? FastWaves<MODE>::value : 1)
void lean_kernel(TrialArgs A, Work W, RootGrids R, UniformTabs T, DecisionTab D, LeanFirst F) {
#ifdef WFPT_PHASE_TIMING
  const long long rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int lane = threadIdx.x & 63;
  // Wave w of the grid takes chunk w, unless the host listed chunks to
  // dispatch first (F.n > 0, the grid is F.n waves longer): then the first
  // F.n waves take the listed chunks and wave w >= F.n takes chunk w - F.n,
  // or nothing if that chunk is listed. Each chunk still has exactly one wave.
  int64_t i = (int64_t)blockIdx.x * kLeanBlock + threadIdx.x;
  if constexpr (FIRST) {
    const int w = (int)(i >> 6);
    if (w < F.n) {
      i = (int64_t)F.c[w] * 64 + lane;
    } else {
      const int listed = F.c[lane];
      if (__ballot(lane < F.n && listed == w - F.n) != 0ull) return;
      i -= (int64_t)F.n * 64;
    }
  }
  const int64_t c = i >> 6;
  if (c * 64 >= A.n) return;  // a wave past the last chunk (wave-uniform)
#ifdef WFPT_PHASE_TIMING
  // the wave of the grid that takes the chunk, where that is not the chunk's
  // own number (stored here: nothing kept live)
  if (FIRST && lane == 0 && c < kPhaseWaves)
    W.phase[c * 8 + 5] = ((unsigned long long)blockIdx.x * kLeanBlock + threadIdx.x) >> 6;
#endif
  const bool own = i < A.n;
  const double x0 = own ? A.x[i] : 0.0;
  double p = 0.0, f0[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  long long ne0 = 0;
  unsigned pend0 = 0u;
  int oc = kFinal;
  // The wave's trials by boundary. Inside one boundary the root z grid and
  // the flipped v, z (pdf.pxi:116-118) are wave-uniform: they stay in scalar
  // registers (zgrid_uniform) instead of per-lane selects and copies.
  // Datasets are ordered by boundary, then |rt| (wfpt_dataset_create), so
  // only the wave at the boundary switch is mixed: its upper-boundary lanes
  // take the second call site.
  const bool pos = x0 > 0;
  const unsigned long long bo = __ballot(own), bp = __ballot(own && pos);
  const int b = (bp == bo) ? 1 : 0;  // every trial upper: 1; otherwise lower first
  // kAdaptTZ: a wave of one boundary whose own lanes all reach the same
  // (small, K) at each of the five t nodes, by the table or each by its own
  // decision, and all pass the per-trial range test keeps the decisions in
  // scalar registers (lean_uniform_level0). Every other wave, and a uniform
  // wave one of whose lanes met a value the fix-up code handles, runs the
  // generic site below.
  bool done = false;
#ifdef WFPT_PHASE_TIMING
  int site = 2;  // 0: uniform by the table, 1: uniform by the vote, 2: generic
#endif
  if constexpr (MODE == kAdaptTZ) {
    if (bp == bo || bp == 0ull) {
      const Trial tr = trial_setup_b(x0, A.P, b != 0);
      double lb, ub;
      tree_root<MODE>(tr, A.P, lb, ub);
      L0Hints H;
      unsigned kp0, sm0;
      // The table stage (table_decisions): the wave's two extreme |rt| looked
      // up among the decision's breakpoints settle all five nodes for every
      // lane. What l0_decisions asks besides the decisions is tested per lane
      // here: valid parameters, x - ub > 0, and the recurrence's q0 / R where
      // a large-time node reads them (only there are they computed).
      H.q0 = -1.0;
      H.R = 0.0;
      H.ia2 = 1.0 / (A.P.a * A.P.a);
      H.D0 = H.D4 = Decision{0, 0, 0};
      H.ok0 = H.ok4 = H.shared = false;
      const bool pre = __ballot(own && tr.valid && tr.x - ub > 0) == bo;
      bool tab = pre && table_decisions(D, tr.x, lb, ub, H.ia2, bo, lane, kp0, sm0);
      if (tab && sm0 != 31u) {
        const double q0 = exp_node((-kPi2 * ((tr.x - lb) * H.ia2)) * 0.5);
        const double Rr = exp_node((kPi2 * (ub - lb)) * (0.125 * H.ia2));
        H.q0 = q0;
        H.R = Rr;
        tab = __ballot(own && q0 > 1e-280 && Rr < 1e10) == bo;
      }
      bool uni = tab;
      // the per-lane pre-pass and vote, unless the table proves the wave split
      // between two pieces (table_split: the vote cannot pass)
      if (!tab && !(pre && table_split(D, tr.x, lb, ub, H.ia2, bo, lane))) {
        unsigned kp, sm;
        const bool okd = own && l0_decisions(tr, A.P, A.K, H, kp, sm);
        kp0 = __builtin_amdgcn_readfirstlane(kp);
        sm0 = __builtin_amdgcn_readfirstlane(sm);
        uni = __ballot(okd && kp == kp0 && sm == sm0) == bo;
      }
      if (uni) {
        int kmax = 0;  // the largest K among the small-time nodes
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          const int kj = (int)((kp0 >> (4 * j)) & 15u);
          if (((sm0 >> j) & 1u) != 0u && kj > kmax) kmax = kj;
        }
        const UniformTab& U = T.U[b];
        const bool safe = uniform_guard((tr.x - ub) * H.ia2, (tr.v * tr.v) * (tr.x - lb), A.P.sv,
                                        U.k[kmax].bound, U.amax);
        if (__ballot(own && safe) == bo) {
          bool bail = false;
          if (own)
            oc = lean_uniform_level0(tr, A.P, A.K, zgrid_uniform(R, b), U, &R.S[b][0][0], H, kp0,
                                     sm0, p, ne0, pend0, bail);
          done = __ballot(own && bail) == 0ull;
#ifdef WFPT_PHASE_TIMING
          if (done) site = tab ? 0 : 1;
#endif
          // counting build: the waves the table settled
          if (COUNT && done && tab && lane == 0) atomicAdd(&W.prof[0], 1);
        }
      }
    }
  }
  if (!done) {
    p = 0.0;
    ne0 = 0;
    pend0 = 0u;
    oc = kFinal;
    if (own && pos == (b != 0))
      oc = eng_level0_t<MODE, false, true>(trial_setup_b(x0, A.P, b != 0), A.P, A.K,
                                           zgrid_uniform(R, b), p, f0, ne0, pend0, &R.S[b][0][0]);
    if (bp != 0ull && bp != bo) {  // mixed wave: its upper-boundary lanes
      if (own && pos)
        oc = eng_level0_t<MODE, false, true>(trial_setup_b(x0, A.P, true), A.P, A.K, R.G[1], p, f0,
                                             ne0, pend0, &R.S[1][0][0]);
    }
    // counting build: the lean waves that took the generic site (prof[0]: the
    // ones the table settled, above)
    if (COUNT && MODE == kAdaptTZ && lane == 0) atomicAdd(&W.prof[3], 1);
  }
  if (__ballot(oc == kTree) != 0ull) {
    if (lane == 0) {
      W.redo[c] = 1;
      // finalize reports the call as deferred: the host runs the redo pass
      if (sum_out(OUT)) A.zeros[c] = kZeroDefer;
    }
    return;
  }
  chunk_out<COUNT, OUT>(A, W, c, lane, p, oc == kExact, kFlagExact, ne0);
#ifdef WFPT_PHASE_TIMING
  // per-wave start / end (the lean pass has no split units: every record)
  if (lane == 0 && c < kPhaseWaves) {
    unsigned long long* rec = W.phase + c * 8;
    rec[0] = rt0;
    rec[1] = __builtin_amdgcn_s_memrealtime();
    unsigned hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    rec[2] = hw;
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    rec[3] = xcc;
    rec[4] = (unsigned long long)site;  // the site the wave took
  }
#endif
}

// ---------------------------------------------------------------------------
// launchers

void launch_direct(bool count, int out, const TrialArgs& A, const Work& W, hipStream_t s) {
  DirectArgs D;
  direct_args(A.P, D);
  with_build<true>(count, out, [&](auto c, auto o) {
    hipLaunchKernelGGL((direct_kernel<decltype(c)::value, decltype(o)::value>),
                       dim3(fast_blocks(A.n)), dim3(kFastBlock), 0, s, A, W, D);
  });
}

void launch_lean(int mode, bool count, int out, const TrialArgs& A, const Work& W, hipStream_t s,
                 const DecisionTab* dt, const LeanFirst* first) {
  DecisionTab D;  // by value, as the other tables: each lane reads its own edge
  if (dt) D = *dt;
  else decision_tab_clear(D);
  RootGrids R;
  root_grids(A.P, R);
  UniformTabs T;  // read by the 2-D family's uniform waves only
  uniform_tabs(R, T);
  // the chunks dispatched first: distinct chunks of this call, or none
  LeanFirst F;
  F.n = 0;
  for (int k = 0; k < kLeanFirstMax; ++k) F.c[k] = 0;
  const int64_t nw = (A.n + 63) / 64;
  if (first && mode == kAdaptTZ && first->n > 0 && first->n <= kLeanFirstMax) {
    bool ok = true;
    for (int k = 0; k < first->n; ++k)  // ascending: in range and without duplicates
      ok = ok && first->c[k] >= 0 && first->c[k] < nw && (k == 0 || first->c[k] > first->c[k - 1]);
    if (ok) F = *first;
  }
  const int64_t waves = nw + F.n, per = kLeanBlock / 64;
  const dim3 grid((waves + per - 1) / per);
  with_value<kAdaptT, kAdaptTZ>(mode, [&](auto m) {
    with_build<false>(count, out, [&](auto c, auto o) {
      if (F.n > 0)  // (the 2-D family only)
        hipLaunchKernelGGL((lean_kernel<kAdaptTZ, decltype(c)::value, decltype(o)::value, true>),
                           grid, dim3(kLeanBlock), 0, s, A, W, R, T, D, F);
      else
        hipLaunchKernelGGL(
            (lean_kernel<decltype(m)::value, decltype(c)::value, decltype(o)::value, false>), grid,
            dim3(kLeanBlock), 0, s, A, W, R, T, D, F);
    });
  });
}

// Resident waves of the 2-D family's lean kernel on the current device, from
// the runtime's occupancy of the built kernel (0: unknown).
int64_t lean_wave_slots() {
  int dev = 0, cus = 0, blocks = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &blocks, lean_kernel<kAdaptTZ, false, OUT_SUM, true>, kLeanBlock, 0) != hipSuccess)
    return 0;
  return (int64_t)cus * blocks * (kLeanBlock / 64);
}

}  // namespace wfpt
