// wfpt_zgrid.hpp — the z grids the host builds per call with the device's own
// operations (bit-identical): a grid's per-trial constants (ZGrid), the dyadic
// points of a root interval, the engine's four grid selections, the large-time
// sine tables and the lean pass's root grids. Host + device; the device-only
// evaluation on a grid is wfpt_grid.hpp.
// Compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "wfpt_math.hpp"
#include "wfpt_types.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// ---------------------------------------------------------------------------
// Per-trial part of the root-level z grid. The 5 z nodes (lb, d, c, e, ub of
// integrate.pxi:114-141 / 143-178) are the same for every t node of a trial,
// so everything that depends on z alone is computed once per trial:
//   * sin/cos(pi g_0), sin/cos(pi g_4) and sin/cos(pi (g_4 - g_0) / 4), from
//     which each large-time t node rotates to g_1..g_3 (angle addition); g_4 is
//     evaluated directly so the w = 1 edge keeps the reference's sin(pi);
//   * the z-only part A_j of the drift-factor exponent (pdf.pxi:96-101):
//     c_j = (A_j - v^2 x) / (2 sv^2 x + 2)   (sv > 0),  c_j = A_j - v^2 x / 2  (sv = 0).
// g[] holds the reference's own node coordinates (every polynomial in w uses
// them); only transcendental factors use the rotations / recurrences.
struct ZGrid {
  double g[5];
  double s0, c0, s4, c4, sd, cd;
  double A[5];
  double h6, h12;  // (g4 - g0) / 6 and / 12: the Simpson weights of this grid's interval
};

// Large-time sines of a grid (pdf.pxi:61-62: sin(k pi w) at the grid's 5
// nodes), k = 1..kSinK, exactly as tnode_pdf_sv_grid5's recurrence produces
// them: sin / cos of nodes 1..3 rotated from node 0 (node 4 direct), then
// s_k = 2 cos(pi w) s_{k-1} - s_{k-2} in the same fused operations. Built on
// the host per call (RootGrids) so the lean pass reads them instead of
// recomputing them per lane; bit-identical to the per-lane recurrence.
constexpr int kSinK = 8;
__host__ __device__ inline void sin_rot(const ZGrid& G, double (&sj)[5], double (&cj)[5]) {
  sj[0] = G.s0;
  cj[0] = G.c0;
  sj[4] = G.s4;
  cj[4] = G.c4;
  for (int j = 1; j < 4; ++j) {
    sj[j] = fma(sj[j - 1], G.cd, cj[j - 1] * G.sd);
    cj[j] = fma(cj[j - 1], G.cd, -(sj[j - 1] * G.sd));
  }
}
// 2 cos(pi g_i) of node i (the recurrence's multiplier)
__host__ __device__ inline double sin_tc(const ZGrid& G, int i) {
  double sj[5], cj[5];
  sin_rot(G, sj, cj);
  const double c = i == 0 ? cj[0] : i == 1 ? cj[1] : i == 2 ? cj[2] : i == 3 ? cj[3] : cj[4];
  return c + c;
}
__host__ __device__ inline void sin_table(const ZGrid& G, double (&S)[kSinK + 1][5]) {
  double sj[5], cj[5];
  sin_rot(G, sj, cj);
  for (int i = 0; i < 5; ++i) {
    const double tc = cj[i] + cj[i];
    S[0][i] = 0.0;
    S[1][i] = sj[i];
    for (int k = 2; k <= kSinK; ++k) S[k][i] = msub(tc, S[k - 1][i], S[k - 2][i]);
  }
}

// z grids of the engine, relative to the dyadic points P of [lb_z, ub_z]:
// kGridRoot {P0, P4, P8, P12, P16} (the root interval's lb, d, c, e, ub),
// kGridL1 {P2, P6, P10, P14, +1 unused} (the aux nodes of both halves),
// kGridL2L {P1, P3, P5, P7, P9}, kGridL2R {P7, P9, P11, P13, P15} (the aux
// nodes of the four quarters; P7 is taken from L2L, P9 from L2R). Five
// equally spaced points each, so tnode_pdf_sv_grid5 serves all four.
enum GridSel : int { kGridRoot = 0, kGridL1 = 1, kGridL2L = 2, kGridL2R = 3 };
// Dyadic point P_k (k = 0..kTreeW) of [lb, ub] as the reference's recursion
// computes it: every interval's midpoint is (ub + lb) / 2 of its own bounds
// and its aux nodes (lb + c) / 2, (c + ub) / 2 (integrate.pxi:94-104) are its
// children's midpoints, so P_k is the end of the chain of midpoints that
// bisects down to k (IEEE addition is commutative: operand order is moot).
__host__ __device__ inline double dyadic_point(double lb, double ub, int k) {
  if (k <= 0) return lb;
  if (k >= kTreeW) return ub;
  int lo = 0, hi = kTreeW;
  for (;;) {
    const int mid = (lo + hi) >> 1;
    const double c = (ub + lb) / 2.;
    if (k == mid) return c;
    if (k < mid) {
      hi = mid;
      ub = c;
    } else {
      lo = mid;
      lb = c;
    }
  }
}

__host__ __device__ inline ZGrid zgrid_of(double lb, double ub, int sel, double v, double sv,
                                          double a) {
  ZGrid G;
  const int k0 = sel == kGridRoot ? 0 : sel == kGridL1 ? 2 : sel == kGridL2L ? 1 : 7;
  const int dk = sel == kGridRoot ? 4 : sel == kGridL1 ? 4 : 2;
#pragma unroll
  for (int i = 0; i < 5; ++i) G.g[i] = dyadic_point(lb, ub, k0 + i * dk);
  // the unused fifth node of kGridL1 (P18, past ub <= 1 by sz / 8): any
  // finite coordinate of the same spacing
  if (sel == kGridL1) G.g[4] = G.g[3] + (G.g[3] - G.g[2]);
  sincospi01(G.g[0], G.s0, G.c0);
  sincospi01(G.g[4], G.s4, G.c4);
  sincospi01((G.g[4] - G.g[0]) * 0.25, G.sd, G.cd);
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    if (sv == 0) {
      G.A[i] = ((-v) * a) * G.g[i];
    } else {
      const double azsv = (a * G.g[i]) * sv;
      G.A[i] = (azsv * azsv) - (((2.0 * a) * v) * G.g[i]);
    }
  }
  G.h6 = (G.g[4] - G.g[0]) / 6;
  G.h12 = (G.g[4] - G.g[0]) / 12;
  return G;
}

// The root z grids of both boundaries alone (the lean level-0 pass): the
// same zgrid_of calls as eng_tables' G[flip][kGridRoot], so bit-identical.
struct RootGrids {
  ZGrid G[2];
  double S[2][kSinK + 1][5];  // their large-time sine tables (sin_table)
};
__host__ __device__ inline void root_grids(const Params& P, RootGrids& R) {
  for (int flip = 0; flip < 2; ++flip) {
    const double zf = flip ? 1. - P.z : P.z, vf = flip ? -P.v : P.v;
    R.G[flip] = zgrid_of(zf - P.sz / 2., zf + P.sz / 2., kGridRoot, vf, P.sv, P.a);
    sin_table(R.G[flip], R.S[flip]);
  }
}

}  // namespace wfpt
