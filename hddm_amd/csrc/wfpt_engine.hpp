// wfpt_engine.hpp — the in-wave refinement engine (device only): a chunk's
// LDS, the breadth-first refinement rounds, a refined tree's density, and the
// one-wave-per-record form of the same rounds. Shared by engine_kernel
// and multi_records_kernel (wfpt_engine.hip) and node_chunk_kernel
// (wfpt_node.hip).
#pragma once
#include "wfpt_kernel_common.hpp"

#pragma clang fp contract(off)

namespace wfpt {

constexpr int kEngBlock = 256;
constexpr int kEngWaves = kEngBlock / 64;
constexpr int kQCap = 2 * (1 << kTreeDepth) * 64;  // tasks (or z walks) of one level
constexpr int kFlagIdle = 16;                       // lane without a trial to integrate
constexpr int kFlagStop = kFlagExact | kFlagFallback | kFlagIdle;

// LDS of one chunk under refinement by a team of TW waves. A z walk's 17
// values are not staged here: the lane that runs its tree17 gathers them by
// wave shuffles (no LDS, no barrier; 3-4% faster on the stress sets in the r04
// interleaved A/B than staging them, despite 28 B of engine scratch).
template <int TW>
struct ChunkLds {
  double F[kTreePoints * 64];              // tree values: point * 64 + owner lane
  double X[64];                            // the owners' x
  EngTables tab;                           // the call's tables
  int fl[64];                              // the owners' flags
  int cnt[64];                             // the owners' pdf_sv evaluations (COUNT)
  int qn[2];                               // lengths of Q and ZQ
  uint16_t Q[kQCap];                       // tasks of the level: owner | point << 6 | grid << 11
  uint16_t ZQ[kQCap];                      // z walks of the level: owner | point << 6
};

__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int TW>
__device__ inline void team_sync() {
  if (TW == 1) wave_sync();
  else __syncthreads();
}

// Appends `code` of every flagged lane of this wave to q at the LDS length
// counter *n (one LDS atomic per wave). Read *n after the next team_sync.
__device__ inline void team_push(bool flag, int code, uint16_t* q, int* n) {
  const int lane = threadIdx.x & 63;
  const unsigned long long b = __ballot(flag);
  if (!b) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(n, __popcll(b));
  base = __shfl(base, 0, 64);
  if (flag) q[base + __popcll(b & lanemask_lt(lane))] = (uint16_t)code;
}

// Point of value y[j] of a grid (GridSel) and whether this grid supplies it.
__device__ inline int grid_point(int gs, int j) {
  const int k0 = gs == kGridRoot ? 0 : gs == kGridL1 ? 2 : gs == kGridL2L ? 1 : 7;
  return k0 + j * (gs <= kGridL1 ? 4 : 2);
}
__device__ inline bool grid_owns(int gs, int j) {
  return gs == kGridRoot ? true : gs == kGridL2R ? j > 0 : j < 4;
}

template <int TW>
__device__ inline void load_tables(ChunkLds<TW>& cl, const EngTables& tab, int tid) {
  const double* src = reinterpret_cast<const double*>(&tab);
  double* dst = reinterpret_cast<double*>(&cl.tab);
  for (int k = tid; k < (int)(sizeof(EngTables) / sizeof(double)); k += 64 * TW) dst[k] = src[k];
}

// Own tree of owner lane `o` in registers.
template <int TW>
__device__ inline void load_tree(const ChunkLds<TW>& cl, int o, double (&f)[kTreePoints]) {
#pragma unroll
  for (int k = 0; k < kTreePoints; ++k) f[k] = cl.F[k * 64 + o];
}

// Work tallies of one chunk (COUNT builds; wfpt_profile_lists).
struct Tally {
  int t1 = 0, t2 = 0, rec = 0, z[3] = {0, 0, 0};
};

// WFPT_PHASE_TIMING (diagnostic builds): shader-clock time per engine phase,
// per wave in W.phase (level 0, tables, z rounds, t rounds, tests + epilogue;
// wfpt_profile_lists reports the sums in kilo-cycles, wfpt_debug_waves the
// per-wave records).
#ifdef WFPT_PHASE_TIMING
struct PhaseClock {
  long long ph[5] = {0, 0, 0, 0, 0};
  long long t = 0;
  int nz = 0, nt = 0;
  __device__ void start() { t = __builtin_amdgcn_s_memtime(); }
  __device__ void mark(int k) {
    const long long now = __builtin_amdgcn_s_memtime();
    ph[k] += now - t;
    t = now;
  }
};
#else
struct PhaseClock {
  int nz = 0, nt = 0;
  __device__ void start() {}
  __device__ void mark(int) {}
};
#endif

// Refinement rounds of one chunk by a team of TW waves (tid = 0..64 TW - 1;
// the chunk's owner lanes are tid < 64). Entry: stage 1 after level 0 with
// its values in F and its z walks queued (engine_kernel), or stage 0 with
// level 0's t nodes (root z grids) queued as tasks (split_unit: they take the
// level-0 hints, l0_hints, so their bits equal fast per-lane level 0's). All
// control is team-uniform.
template <int MODE, bool COUNT, int TW>
__device__ inline void refine_rounds(const TrialArgs& A, ChunkLds<TW>& cl, int tid, int stage,
                                     Tally& ty, PhaseClock& pc) {
  constexpr int NT = 64 * TW;
  const double v = A.P.v, sv = A.P.sv, a = A.P.a, z = A.P.z, t = A.P.t;
  const double err = A.K.err, se = A.K.simps_err;
  const int nsz = A.K.n_sz;
  const int depth = (MODE == kAdaptZ) ? A.K.n_sz : A.K.n_st;
  const double iwt = 1.0 / (cl.tab.tP[kTreeW] - cl.tab.tP[0]);
  const double ia2 = 1.0 / (a * a);  // as l0_hints: the same tt for the same t node
  int L = 0, r = 0;
#pragma unroll 1
  for (;;) {
    const int nq = cl.qn[0], nz = cl.qn[1];
    if (stage == 0 && r * NT >= nq) {
      stage = 1;
      r = 0;
    }
    if (stage == 1 && (MODE != kAdaptTZ || r * 16 * TW >= nz)) stage = 2;
    if (stage == 2) {
      pc.mark(2);
      // constant indices: a runtime index would put the tally in scratch
      if (L == 0) ty.z[0] = nz;
      else if (L == 1) ty.z[1] = nz;
      else if (L == 2) ty.z[2] = nz;
      // stop tests of level L, each owner lane its own tree
      unsigned need = 0u;
      if (tid < 64 && !(cl.fl[tid] & kFlagStop)) {
        double f[kTreePoints];
        load_tree(cl, tid, f);
        const double(&P)[kTreePoints] =
            (MODE == kAdaptZ) ? cl.tab.zP[cl.X[tid] > 0] : cl.tab.tP;
        int fl = 0, nref = 0;
        (void)tree17(f, P, se, depth, L, fl, need, nref);
        if (L == kTreeDepth && need) fl |= kFlagFallback;  // deeper than the in-wave levels
        if (fl & (kFlagExact | kFlagFallback)) {
          atomicOr(&cl.fl[tid], fl & (kFlagExact | kFlagFallback));
          need = 0u;
        }
      }
      if (COUNT && L == 0 && tid < 64) ty.rec = __popcll(__ballot(need != 0u));
      if (L == kTreeDepth) break;
      if (tid == 0) {
        cl.qn[0] = 0;
        cl.qn[1] = 0;
      }
      team_sync<TW>();
      // level L + 1's tasks: for each refining interval m of level L, the aux
      // nodes d, e of both its halves (kAdaptZ: one grid per interval)
      if (tid < 64) {
        if (MODE == kAdaptZ) {
          for (int m = 0; m < (1 << L); ++m)
            team_push((need >> m) & 1u, tid | ((L == 0 ? kGridL1 : kGridL2L + m) << 11), cl.Q,
                      &cl.qn[0]);
        } else {
          const int wm = kTreeW >> L;  // width of a level-L interval
          for (int m = 0; m < (1 << L); ++m)
            for (int q = 1; q < 8; q += 2)
              team_push((need >> m) & 1u, tid | ((m * wm + q * (wm / 8)) << 6), cl.Q, &cl.qn[0]);
        }
      }
      team_sync<TW>();
      pc.mark(4);
      if (COUNT) {
        if (L == 0) ty.t1 = cl.qn[0];
        else ty.t2 = cl.qn[0];
      }
      if (cl.qn[0] == 0) break;
      ++L;
      stage = 0;
      r = 0;
      continue;
    }
    // ---- one round: at most one evaluation per lane ----
    int owner = tid & 63, pos = 0, gs = kGridRoot, zslot = 0;
    bool on;
    if (stage == 0) {
      const int e = r * NT + tid;
      on = e < nq;
      if (on) {
        const int code = cl.Q[e];
        owner = code & 63;
        pos = (code >> 6) & 31;
        gs = code >> 11;
      }
    } else {
      zslot = tid >> 2;
      const int e = r * 16 * TW + zslot;
      on = e < nz;
      gs = tid & 3;
      if (on) {
        const int code = cl.ZQ[e];
        owner = code & 63;
        pos = (code >> 6) & 31;
      }
    }
    on = on && !(cl.fl[owner] & kFlagStop);
    double y[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int flip = 0;
    bool ovf = false;  // a drift factor overflowed (tnode_pdf_sv_grid5)
    if (on) {
      const double xo = cl.X[owner];
      flip = xo > 0;
      const double vo = flip ? -v : v;
      const double xa = fabs(xo);
      const double xx = (MODE == kAdaptZ) ? xa - t : xa - cl.tab.tP[pos];
      // level-0 t nodes (split units): the per-lane loop's hints (l0_hints)
      double qh = -1.0;
      bool known = false;
      Decision kd{0, 0, 0};
      if (MODE != kAdaptZ && L == 0 && stage == 0) {
        const L0Hints H = l0_hints(xa, cl.tab.tP[0], cl.tab.tP[kTreeW], a, err);
        const int j = pos / (kTreeW / 4);
        qh = H.qh(j);
        known = j == 0 ? H.ok0 : (j == 4 ? H.ok4 : H.shared);
        kd = j == 4 ? H.D4 : H.D0;
      }
      const TNode T = tnode_setup_r(xx, vo, sv, a, ia2, err, qh, known, kd);
      if (T.amb) atomicOr(&cl.fl[owner], (int)kFlagExact);
      if (MODE == kAdaptT) y[0] = tnode_pdf_sv(T, flip ? 1. - z : z, vo, sv, a);
      else
        ovf = !tnode_pdf_sv_grid5(T, cl.tab.G[flip][gs], vo, sv, a, y);  // literal values
    }
    if (stage == 0) {
      bool pend = false;
      if (on) {
        if (MODE == kAdaptT) {
          cl.F[pos * 64 + owner] = y[0] * iwt;
          if (COUNT) atomicAdd(&cl.cnt[owner], 1);
        } else if (MODE == kAdaptZ) {
          const double izf = cl.tab.iz[flip];
#pragma unroll
          for (int j = 0; j < 5; ++j)
            if (grid_owns(gs, j)) cl.F[grid_point(gs, j) * 64 + owner] = y[j] * izf;
          if (COUNT) atomicAdd(&cl.cnt[owner], gs == kGridRoot ? 5 : 4);
        } else {
          // kAdaptTZ: the z integral's prologue + root test (integrate.pxi:
          // 114-141); a refinement queues the z walk
          // (inner_root's operations: the root grid's weights, simp_value)
          const double izf = cl.tab.iz[flip];
          const ZGrid& gr = cl.tab.G[flip][kGridRoot];
          const Simp s = simp5p(gr.h6, gr.h12, y[0] * izf, y[1] * izf, y[2] * izf, y[3] * izf,
                                y[4] * izf);
          int f = 0;
          // an overflowed root grid: the z walk (inner_root's rule)
          pend = simpson_refine(s.S, s.S2, se, nsz, f) || ovf;
          if (ovf) f = 0;
          if (f) atomicOr(&cl.fl[owner], f);
          else if (!pend) cl.F[pos * 64 + owner] = simp_value(s) * iwt;
          if (COUNT) atomicAdd(&cl.cnt[owner], 5);
        }
      }
      if (MODE == kAdaptTZ) {
        team_push(pend && on, owner | (pos << 6), cl.ZQ, &cl.qn[1]);
      }
      ++pc.nt;
    } else if (MODE == kAdaptTZ) {
      double zv[kTreePoints];
      static_assert(TW == 1, "z walks gather their values by wave shuffles");
      // lane t < 16 runs walk t: its 17 values come from lanes 4t .. 4t + 3
      // (grid gs = source lane & 3; grid_point / grid_owns), by shuffles
      const double izf = on ? cl.tab.iz[flip] : 0.0;
      double yz[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) yz[j] = y[j] * izf;
      const int b4 = (tid & 15) * 4;
#pragma unroll
      for (int j = 0; j < 5; ++j) zv[4 * j] = __shfl(yz[j], b4 + kGridRoot, 64);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        zv[2 + 4 * j] = __shfl(yz[j], b4 + kGridL1, 64);
        zv[1 + 2 * j] = __shfl(yz[j], b4 + kGridL2L, 64);
        zv[9 + 2 * j] = __shfl(yz[j + 1], b4 + kGridL2R, 64);
      }
      const int e = r * 16 * TW + tid;
      if (tid < 16 * TW && e < nz) {
        const int code = cl.ZQ[e];
        const int ow = code & 63, ps = (code >> 6) & 31;
        if (!(cl.fl[ow] & kFlagStop)) {
          int f = 0, nref = 0;
          unsigned need = 0u;
          const double zi = tree17(zv, cl.tab.zP[cl.X[ow] > 0], se, nsz, kTreeDepth, f, need, nref);
          if (need) f |= kFlagFallback;  // z tree deeper than the walk's levels
          if (f & (kFlagExact | kFlagFallback)) atomicOr(&cl.fl[ow], f & (kFlagExact | kFlagFallback));
          else cl.F[ps * 64 + ow] = zi * iwt;
          if (COUNT) atomicAdd(&cl.cnt[ow], 4 * nref);
        }
      }
      ++pc.nz;
    }
    ++r;
    team_sync<TW>();
    if (stage == 0) pc.mark(3);
  }
}

// Final density of owner lane o (a refined tree: tree17 over its stored
// values; the level tests already flagged ties and deeper trees).
template <int MODE, int TW>
__device__ inline void tree_density(const TrialArgs& A, const ChunkLds<TW>& cl, int o, double x,
                                    double& p, bool& defer, int& rf) {
  const int ff = cl.fl[o];
  if (ff & (kFlagExact | kFlagFallback)) {
    defer = true;
    rf = (ff & kFlagExact) ? kFlagExact : kFlagFallback;
    return;
  }
  double f[kTreePoints];
  load_tree(cl, o, f);
  const Trial tr = trial_setup(x, A.P);
  const double(&P)[kTreePoints] = (MODE == kAdaptZ) ? cl.tab.zP[x > 0] : cl.tab.tP;
  const int depth = (MODE == kAdaptZ) ? A.K.n_sz : A.K.n_st;
  int fl = 0, nref = 0;
  unsigned need = 0u;
  p = tree17(f, P, A.K.simps_err, depth, kTreeDepth, fl, need, nref);
  // structural zero: no evaluation point with x - t_node > 0
  const bool structural = (MODE == kAdaptZ) ? tr.x - A.P.t <= 0 : tr.x - P[0] <= 0;
  defer = (fl & kFlagExact) || need || !(p > kExactBelow || structural);
  if (defer && !(fl & kFlagExact) && !need && tiny_absorbed(p, A.P.p_outlier, A.K.w_outlier)) {
    defer = false;  // the mixture absorbs it (tiny_absorbed)
    p = 0.0;
  }
  rf = kFlagExact;
}

// A node's trial term: mixture with the node's p_outlier, -inf for a zero
// density or a p_outlier outside [0, 1] (wfpt.pyx:63-72 per node).
__device__ inline double node_logp(double p, const Params& Q, const Knobs& K) {
  const bool ok = (Q.p_outlier >= 0) & (Q.p_outlier <= 1);  // wfpt.pyx:63-64 per node
  p = p * (1 - Q.p_outlier) + K.w_outlier * Q.p_outlier;
  return (!ok || p == 0) ? -INFINITY : log_val(p);
}

// The per-call tables (EngTables) of one trial's parameters, built by the lanes
// of a wave in parallel: lanes 0-7 the 8 z grids, then the dyadic points of the
// t tree and of both z trees, then 1 / (ub_z - lb_z). The same functions as
// the host's eng_tables.
__device__ inline void eng_tables_wave(const Params& P, EngTables& T, int lane) {
  constexpr int kP = kTreePoints;
  if (lane < 8) {
    const int flip = lane >> 2, sel = lane & 3;
    const double zf = flip ? 1. - P.z : P.z, vf = flip ? -P.v : P.v;
    T.G[flip][sel] = zgrid_of(zf - P.sz / 2., zf + P.sz / 2., sel, vf, P.sv, P.a);
  } else if (lane < 8 + kP) {
    T.tP[lane - 8] = dyadic_point(P.t - P.st / 2., P.t + P.st / 2., lane - 8);
  } else if (lane < 8 + 3 * kP) {
    const int idx = lane - 8 - kP, flip = idx / kP, k = idx % kP;
    const double zf = flip ? 1. - P.z : P.z;
    T.zP[flip][k] = dyadic_point(zf - P.sz / 2., zf + P.sz / 2., k);
  } else if (lane < 8 + 3 * kP + 2) {
    const int flip = lane - (8 + 3 * kP);
    const double zf = flip ? 1. - P.z : P.z;
    T.iz[flip] = 1.0 / ((zf + P.sz / 2.) - (zf - P.sz / 2.));
  }
  wave_sync();
}

// Deferred trials of the per-node and per-trial-parameter paths (records of
// index + parameter row; adaptive families). The per-lane recursion would
// leave one lane walking a trial's whole tree serially (~40 dependent
// evaluations at one-wave latency set the call's length); instead one wave
// takes one record and runs the engine's breadth-first rounds on the trial's
// own tables: its level-0 t nodes (or root z grid) as tasks, then refinement
// levels and z walks across the lanes, exactly as a split unit of the dataset
// engine. Trees deeper than kTreeDepth and rounding-critical values are left
// to the caller's rare list, or (MULTI: wiener_like_multi's term) take the
// per-lane fallback / exact path on lane 0.
// One wave per record, wave ids w0, w0 + nwaves, ...: the record's tables in
// the wave's LDS, its level-0 t nodes as tasks, the refinement rounds, and on
// lane 0 its density (tree17, the exact path or the per-lane walk) and term.
// A record's index is virtual (t n_tab + i: trial i of parameter table t, the
// multi-table node call); its RT is x[i], its term lp[t n_tab + i].
__device__ inline int64_t tab_trial(int64_t v, int64_t n_tab) { return v < n_tab ? v : v % n_tab; }
// (the node path's rare list: see node_sum)
constexpr int kRareShift = 56;
constexpr int64_t kRareMask = (1LL << kRareShift) - 1;
constexpr int kRareExact = 1, kRareWalk = 2;
struct NodeRare {
  int64_t* v;
  int32_t* j;
  int* n;
};
__device__ inline void rare_push(const NodeRare& R, int64_t v, int32_t vj, int kind, double* lp) {
  const int k = atomicAdd(R.n, 1);
  R.v[k] = v | ((int64_t)kind << kRareShift);
  R.j[k] = vj;
  lp[v] = 0.0;  // a neutral addend until the summing kernel settles the trial
}

template <int MODE, bool COUNT, bool MULTI>
__device__ inline void node_records(ChunkLds<1>& cl, int lane, int w0, int nwaves,
                                    const double* x, const Knobs& K, double* lp,
                                    const int64_t* d_idx, const Params* d_par, int nd,
                                    unsigned long long* evals, int* status,
                                    int64_t n_tab = INT64_MAX, const NodeRare* R = nullptr,
                                    const int32_t* node = nullptr, int32_t n_nodes = 0) {
  long long ne = 0;
  int errf = 0;
  for (int k = w0; k < nd; k += nwaves) {
    const int64_t i = d_idx[k];
    const Params Q = d_par[k];
    TrialArgs A{};
    A.x = x;
    A.P = Q;
    A.K = K;
    A.wp_outlier = K.w_outlier * Q.p_outlier;
    const double x0 = x[tab_trial(i, n_tab)];
    eng_tables_wave(Q, cl.tab, lane);
    cl.X[lane] = lane == 0 ? x0 : 0.0;
    cl.fl[lane] = (lane == 0 && trial_setup(x0, Q).valid) ? 0 : (int)kFlagIdle;
    if (COUNT) cl.cnt[lane] = 0;
    if (lane == 0) {
      cl.qn[0] = 0;
      cl.qn[1] = 0;
    }
    wave_sync();
    constexpr int n0 = (MODE == kAdaptZ) ? 1 : 5;
    team_push(lane < n0 && !(cl.fl[0] & kFlagStop), (lane * (kTreeW / 4)) << 6, cl.Q, &cl.qn[0]);
    wave_sync();
    Tally ty;
    PhaseClock pc;
    refine_rounds<MODE, COUNT, 1>(A, cl, lane, 0, ty, pc);
    if (lane == 0) {
      double p = 0.0;
      bool defer = false;
      int rf = kFlagExact;
      long long n1 = 0;
      if (!(cl.fl[0] & kFlagIdle)) {
        tree_density<MODE, 1>(A, cl, 0, x0, p, defer, rf);
        if (COUNT) n1 = cl.cnt[0];
      }
      if constexpr (MULTI) {
        if (defer) {
          n1 = 0;
          p = (rf & kFlagExact) ? exact_pdf(x0, Q, K, &n1, &errf)
                                : fallback_pdf<MODE>(x0, Q, K, &n1, &errf);
        }
        ne += n1;
        lp[i] = log_val(p * (1 - Q.p_outlier) + (K.w_outlier * Q.p_outlier));
      } else {
        if (defer) {  // the node path's rare list (node_sum settles it)
          const int64_t t = i / n_tab;
          rare_push(*R, i, (int32_t)(t * n_nodes + node[i - t * n_tab]),
                    (rf & kFlagExact) ? kRareExact : kRareWalk, lp);
        } else {
          ne += n1;
          lp[i] = node_logp(p, Q, K);
        }
      }
    }
    wave_sync();  // the next record reuses this wave's LDS
  }
  if (errf & kFlagErrors) atomicOr(status, errf & kFlagErrors);
  if (COUNT) {
    ne = wave_sum_ll(ne);
    if (lane == 0) atomicAdd(evals, (unsigned long long)ne);
  }
}

}  // namespace wfpt
