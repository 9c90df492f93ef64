// Host program for tests/test_lean_tables_host.py (its own main; built with
// -fsanitize=address,undefined, never loaded into Python): the lean pass's
// uniform-wave table (uniform_tab) against the expressions a lane of
// small_grid2d evaluates, and the per-trial range test (uniform_guard)
// against small_grid2d's per-node `safe`.
//
// The lane's expressions are restated below from small_grid2d
// (hddm_amd/csrc/wfpt_grid.hpp), which is device code: the same operations
// in the same order, contraction off. m is formed as -0.5 / tt here (the
// device takes it from rsqrt: a few ulp apart, far inside the guard's margin).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../hddm_amd/csrc/wfpt_lean_tables.hpp"
#include "../../hddm_amd/csrc/wfpt_types.hpp"
#include "../../hddm_amd/csrc/wfpt_zgrid.hpp"

#pragma clang fp contract(off)

using namespace wfpt;

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int g_fail = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      if (g_fail < 20) {                    \
        std::printf("FAIL %s: ", #cond);    \
        std::printf(__VA_ARGS__);           \
        std::printf("\n");                  \
      }                                     \
      ++g_fail;                             \
    }                                       \
  } while (0)

// small_grid2d's prologue for one node: c[], the guard (`safe`).
struct LaneNode {
  double c[5];
  bool safe;
};
static LaneNode lane_node(const ZGrid& G, int K, double m, double vvx, double cden, double sv) {
  LaneNode L;
  const int lower = (int)(-floor((K - 1) / 2.));
  const int upper = (int)ceil((K - 1) / 2.);
  const double dv = (sv == 0) ? vvx * 0.5 : vvx, dm = (sv == 0) ? 1.0 : cden;
  double* c = L.c;
  for (int i = 0; i < 5; ++i) c[i] = (G.A[i] - dv) * dm;
  const double lo2 = (double)(2 * lower);
  const double u0 = G.g[0] + lo2, u4 = G.g[4] + (double)(2 * upper);
  const double h = G.g[1] - G.g[0];
  const double d1 = c[1] - c[0];
  const double d2 = (c[2] - c[1]) - d1;
  const double aR = m * (h * (2.0 * u0 + h)) + d1;
  const double aQj = (2.0 * m) * (h * h) + d2;
  const double aP = (4.0 * m) * (u0 + 1.0);
  const double aQk = 8.0 * m;
  const double aQjk = (4.0 * m) * h;
  const double cmax = fmax(fmax(fmax(c[0], c[1]), fmax(c[2], c[3])), c[4]);
  const double cmin = fmin(fmin(fmin(c[0], c[1]), fmin(c[2], c[3])), c[4]);
  const double U = fmax(fabs(u0), fabs(u4));
  const double km1 = (double)(K - 1);
  const double rmax = fmax(fmax(fabs(aR), fabs(aR + 3.0 * aQj)),
                           fmax(fabs(aR + km1 * aQjk), fabs((aR + 3.0 * aQj) + km1 * aQjk)));
  const double pmax = fmax(fabs(aP), fabs(aP + (km1 - 1.0) * aQk));
  const double qmax = fmax(fmax(fabs(aQj), fabs(aQk)), fabs(aQjk));
  constexpr double B = 640.0;
  L.safe = (cmax < B) & (m * (U * U) + cmin > -B) & (fmax(fmax(rmax, pmax), qmax) < B);
  return L;
}

struct Draw {
  double v, sv, a, z, sz, t, st;
};
static Draw draw(std::mt19937_64& rng, bool wide) {
  std::uniform_real_distribution<double> u(0.0, 1.0);
  Draw d;
  d.v = (wide ? 40.0 : 8.0) * (2.0 * u(rng) - 1.0);
  d.sv = u(rng) < 0.2 ? 0.0 : (wide ? 6.0 : 3.0) * u(rng);
  d.a = wide ? 0.1 + 12.0 * u(rng) : 0.3 + 3.7 * u(rng);
  d.z = 0.05 + 0.9 * u(rng);
  const double room = 2.0 * fmin(d.z, 1.0 - d.z);
  d.sz = (u(rng) < 0.1 ? 1.0 : u(rng)) * room;
  if (d.sz < 1e-3) d.sz = 1e-3;
  d.t = 0.05 + 0.6 * u(rng);
  d.st = u(rng) * 2.0 * d.t;
  if (d.st < 1e-3) d.st = 1e-3;
  return d;
}

int main() {
  std::mt19937_64 rng(20261020);
  std::uniform_real_distribution<double> u(0.0, 1.0);

  // 1. the table against the lane's expressions
  for (int it = 0; it < 1000; ++it) {
    const Draw d = draw(rng, it % 4 == 3);
    Params P{d.v, d.sv, d.a, d.z, d.sz, d.t, d.st, 0.05};
    RootGrids R;
    root_grids(P, R);
    UniformTabs T;
    uniform_tabs(R, T);
    for (int flip = 0; flip < 2; ++flip) {
      const ZGrid& G = R.G[flip];
      const UniformTab& U = T.U[flip];
      double am = 0.0;
      for (int i = 0; i < 5; ++i) am = fmax(am, fabs(G.A[i]));
      CHECK(same(U.amax, am), "amax");
      double prev = 0.0;
      for (int K = 1; K <= kUniK; ++K) {
        const int lower = (int)(-floor((K - 1) / 2.));
        const int upper = (int)ceil((K - 1) / 2.);
        CHECK(lower == -((K - 1) >> 1) && upper == (K >> 1), "K %d", K);
        CHECK(lower >= -4 && upper <= 4, "rows of K %d", K);
        const double lo2 = (double)(2 * lower);
        const double u0 = G.g[0] + lo2;
        const double h = G.g[1] - G.g[0];
        const UniformK& C = U.k[K];
        CHECK(same(C.u0u0, u0 * u0), "u0u0 K %d", K);
        CHECK(same(C.hh2, h * (2.0 * u0 + h)), "hh2 K %d", K);
        CHECK(same(C.hh, h * h), "hh K %d", K);
        CHECK(same(C.u0p1, u0 + 1.0), "u0p1 K %d", K);
        CHECK(same(C.h, h), "h K %d", K);
        CHECK(C.bound >= prev && C.bound >= 8.0, "bound K %d", K);
        prev = C.bound;
        // the term loop's multipliers: k2 runs lo2, lo2 + 2, ... as in the lane
        double k2 = lo2;
        for (int k = lower; k <= upper; ++k) {
          for (int i = 0; i < 5; ++i)
            CHECK(same(U.u[k + 4][i], G.g[i] + k2), "u[%d][%d] K %d", k, i, K);
          k2 = k2 + 2.0;
        }
      }
    }
  }

  // 2. uniform_guard passes => `safe` at every small-time node, |c| < 600 everywhere
  long passed = 0, refused = 0, unsafe_refused = 0;
  for (long it = 0; it < 1000000; ++it) {
    const Draw d = draw(rng, it % 3 == 2);
    Params P{d.v, d.sv, d.a, d.z, d.sz, d.t, d.st, 0.05};
    const int flip = (int)(it & 1);
    const double zf = flip ? 1. - P.z : P.z, vf = flip ? -P.v : P.v;
    const ZGrid G = zgrid_of(zf - P.sz / 2., zf + P.sz / 2., kGridRoot, vf, P.sv, P.a);
    UniformTab U;
    uniform_tab(G, U);
    const double lb = P.t - P.st / 2., ub = P.t + P.st / 2.;
    // x - ub from 1e-4 s to ~8 s, log-uniform
    const double x = ub + std::exp(std::log(1e-4) + u(rng) * std::log(8e4));
    if (!(x - ub > 0)) continue;
    const double ia2 = 1.0 / (P.a * P.a);
    int Kj[5], small[5], kmax = 0;
    for (int j = 0; j < 5; ++j) {
      Kj[j] = 1 + (int)(rng() % kUniK);
      small[j] = (rng() % 4) != 0;
      if (small[j] && Kj[j] > kmax) kmax = Kj[j];
    }
    const bool pass = uniform_guard((x - ub) * ia2, (vf * vf) * (x - lb), P.sv, U.k[kmax].bound,
                                    U.amax);
    const double c = (ub + lb) / 2.;
    const double tcs[5] = {lb, (lb + c) / 2., c, (c + ub) / 2., ub};
    bool all_safe = true;
    for (int j = 0; j < 5; ++j) {
      const double xx = x - tcs[j];
      const double tt = xx * ia2;
      const double m = -0.5 / tt;
      double cden = 0.0;
      if (P.sv != 0) cden = 0.5 / (((P.sv * P.sv) * xx) + 1.0);
      const double vvx = (vf * vf) * xx;
      const LaneNode L = lane_node(G, Kj[j], m, vvx, cden, P.sv);
      bool ok = true;
      for (int i = 0; i < 5; ++i) ok = ok && fabs(L.c[i]) < 600.0;
      if (small[j]) ok = ok && L.safe;
      all_safe = all_safe && ok;
      if (pass)
        CHECK(ok, "draw %ld node %d K %d small %d: v %g sv %g a %g z %g sz %g t %g st %g x %g", it,
              j, Kj[j], small[j], vf, P.sv, P.a, zf, P.sz, P.t, P.st, x);
    }
    if (pass) ++passed;
    else {
      ++refused;
      if (!all_safe) ++unsafe_refused;
    }
  }
  std::printf("guard: %ld passed, %ld refused (%ld of them unsafe at some node)\n", passed,
              refused, unsafe_refused);
  // the check is not vacuous: both outcomes occur, and the guard refuses real unsafe draws
  CHECK(passed > 100000, "passed %ld", passed);
  CHECK(unsafe_refused > 1000, "unsafe refused %ld", unsafe_refused);
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
