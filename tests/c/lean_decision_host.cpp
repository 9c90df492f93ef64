// Host program for tests/test_lean_decision_host.py (its own main; built with
// -fsanitize=address,undefined, never loaded into Python): the lean pass's
// series-decision table (decision_tab, hddm_amd/csrc/wfpt_lean_tables.hpp) against
// the reference's formula (pdf.pxi:36-60), restated below with the host libm
// (what the reference itself runs) together with decide64's ambiguity tests.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../hddm_amd/csrc/wfpt_lean_tables.hpp"
#include "../../hddm_amd/csrc/wfpt_zgrid.hpp"

#pragma clang fp contract(off)

using namespace wfpt;

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

// pdf.pxi:36-60 on tt, and decide64's four ambiguity tests (1e-12 relative).
struct Ref {
  int small, K;
  bool amb;
  double ks, kl;
};
static Ref reference(double tt, double err) {
  const double pi = 3.14159265358979323846;
  double kl, ks;
  const double sqt = std::sqrt(tt);
  const double ips = 1. / (pi * sqt);
  const double arg_l = (pi * tt) * err;
  const double arg_s = (2.0 * std::sqrt((2.0 * pi) * tt)) * err;
  if (arg_l < 1.0) {
    kl = std::sqrt((-2.0 * std::log(arg_l)) / ((pi * pi) * tt));
    kl = (kl < ips) ? ips : kl;
  } else {
    kl = ips;
  }
  if (arg_s < 1.0) {
    ks = 2.0 + std::sqrt((-2.0 * tt) * std::log(arg_s));
    const double b = sqt + 1.0;
    ks = (ks < b) ? b : ks;
  } else {
    ks = 2.0;
  }
  Ref R;
  R.small = ks < kl;
  const double kk = R.small ? ks : kl;
  R.K = (int)std::ceil(kk);
  const double tol = 1e-12;
  R.amb = std::fabs(arg_l - 1.0) <= tol || std::fabs(arg_s - 1.0) <= tol ||
          std::fabs(ks - kl) <= tol * kl || std::fabs(kk - std::rint(kk)) <= tol * kk;
  R.ks = ks;
  R.kl = kl;
  return R;
}
// the piece code the table should hold for a reference decision (0: K beyond the tables)
static unsigned code_of(const Ref& R) {
  if (R.K < 1 || R.K > (R.small ? kUniK : kSinK)) return 0u;
  return (R.small ? 16u : 0u) | (unsigned)R.K;
}

// The lookup as the kernel does it for a wave's extreme tt: the counts of
// edges <= tt are equal and odd, and the piece has a code.
static unsigned wave_lookup(const DecisionTab& T, double tmin, double tmax) {
  int n0, n1;
  const unsigned c0 = decision_lookup(T, tmin, &n0);
  decision_lookup(T, tmax, &n1);
  return (n0 == n1 && (n0 & 1) && c0 != 0u) ? c0 : 0u;
}

// whenever the table answers for tt_dev, the reference on tt_ref agrees and is not ambiguous
static void check_answer(const DecisionTab& T, double err, double tt_dev, double tt_ref,
                         long& answered) {
  const unsigned c = decision_lookup(T, tt_dev);
  if (c == 0u) return;
  ++answered;
  const Ref R = reference(tt_ref, err);
  CHECK(code_of(R) == c, "err %g tt %.17g: table %u, reference small %d K %d", err, tt_ref, c,
        R.small, R.K);
  CHECK(!R.amb, "err %g tt %.17g: ambiguous (ks %.17g kl %.17g)", err, tt_ref, R.ks, R.kl);
}

int main() {
  const double errs[6] = {1e-2, 1e-3, 1e-4, 1e-6, 1e-10, 1e-80};
  const int want_pieces[6] = {6, 6, 6, 8, 8, -1};
  std::mt19937_64 rng(20261021);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (int ie = 0; ie < 6; ++ie) {
    const double err = errs[ie];
    DecisionTab T;
    decision_tab(err, T);
    const double lo = kDecLo, hi = decision_hi(err);
    int np = 0;
    while (np < kDecPieces && T.code[np] != 0u) ++np;
    // the layout: strictly increasing edges, +inf past the last piece, codes in range
    for (int e = 0; e + 1 < 2 * np; ++e)
      CHECK(T.edge[e] < T.edge[e + 1], "err %g edge %d", err, e);
    for (int e = 2 * np; e < 2 * kDecPieces; ++e) CHECK(std::isinf(T.edge[e]), "err %g pad %d", err, e);
    for (int i = np; i < kDecPieces; ++i) CHECK(T.code[i] == 0u, "err %g code %d", err, i);
    CHECK(np > 0 && T.edge[0] >= lo && T.edge[2 * np - 1] <= hi, "err %g domain", err);

    // (a) a dense scan of the reference: its runs of equal (small, K), the
    // breakpoints between them (bisected here), ks nondecreasing and kl
    // nonincreasing on the domain
    const int N = 400000;
    std::vector<unsigned> runs;
    std::vector<double> bps;
    int all_runs = 0;
    double pt = lo;
    Ref pr = reference(pt, err);
    runs.push_back(code_of(pr));
    all_runs = 1;
    for (int i = 1; i <= N; ++i) {
      const double tt = i == N ? hi : lo * std::exp(std::log(hi / lo) * ((double)i / N));
      const Ref R = reference(tt, err);
      CHECK(R.ks >= pr.ks * (1.0 - 1e-13), "err %g ks not monotone at %.17g", err, tt);
      CHECK(R.kl <= pr.kl * (1.0 + 1e-13), "err %g kl not monotone at %.17g", err, tt);
      if (R.small != pr.small || R.K != pr.K) {
        ++all_runs;
        double l = pt, r = tt;
        for (;;) {
          const double m = l + (r - l) * 0.5;
          if (!(l < m && m < r)) break;
          const Ref M = reference(m, err);
          if (M.small == pr.small && M.K == pr.K) l = m;
          else r = m;
        }
        bps.push_back(r);
        if (code_of(R) != runs.back()) runs.push_back(code_of(R));
      }
      pt = tt;
      pr = R;
    }
    std::vector<unsigned> answered_runs;
    for (unsigned c : runs)
      if (c != 0u) answered_runs.push_back(c);
    CHECK((int)answered_runs.size() == np, "err %g: %d pieces, scan %d", err, np,
          (int)answered_runs.size());
    for (int i = 0; i < np && i < (int)answered_runs.size(); ++i)
      CHECK(T.code[i] == answered_runs[i], "err %g piece %d: %u, scan %u", err, i, T.code[i],
            answered_runs[i]);
    if (want_pieces[ie] > 0)
      CHECK(all_runs == want_pieces[ie] && np == want_pieces[ie], "err %g: %d runs, %d pieces", err,
            all_runs, np);
    else
      CHECK(all_runs > np, "err %g: no K beyond the tables (%d runs)", err, all_runs);
    std::printf("err %g: domain [%g, %g], %d pieces of %d runs:", err, lo, hi, np, all_runs);
    for (int i = 0; i < np; ++i)
      std::printf(" %s%u [%.6g, %.6g)", (T.code[i] & 16u) ? "s" : "l", T.code[i] & 15u,
                  T.edge[2 * i], T.edge[2 * i + 1]);
    std::printf("\n");

    // (b) interior answers
    long answered = 0;
    const int M = 2000000;
    for (int i = 0; i <= M; ++i) {
      const double tt = (lo / 2) * std::exp(std::log((4 * hi) / lo) * ((double)i / M));
      check_answer(T, err, tt, tt, answered);
    }
    CHECK(answered > M / 4, "err %g answered %ld", err, answered);
    for (int e = 0; e < 2 * np; ++e) {
      double dn = T.edge[e], up = T.edge[e];
      for (int k = 0; k < 4; ++k) {
        check_answer(T, err, dn, dn, answered);
        check_answer(T, err, up, up, answered);
        dn = std::nextafter(dn, 0.0);
        up = std::nextafter(up, 1e300);
      }
    }
    // tt as the lane forms it, (x - tc) * ia2, against the reference's xx / a2:
    // broad draws, and draws aimed within a few bands of an edge
    for (int it = 0; it < 400000; ++it) {
      const double a = 0.3 + 3.7 * u(rng), t = 0.05 + 0.6 * u(rng), st = u(rng) * 2.0 * t;
      const double lb = t - st / 2., ub = t + st / 2.;
      const double c = (ub + lb) / 2.;
      const double tcs[5] = {lb, (lb + c) / 2., c, (c + ub) / 2., ub};
      const double tc = tcs[rng() % 5];
      const double a2 = a * a, ia2 = 1.0 / a2;
      double x;
      if (it & 1) {
        const double e = T.edge[rng() % (2 * np)];
        x = tc + (a2 * e) * (1.0 + (4.0 * kDecBand) * (2.0 * u(rng) - 1.0));
      } else {
        x = tc + std::exp(std::log(1e-5) + u(rng) * std::log(1e6));
      }
      const double xx = x - tc;
      check_answer(T, err, xx * ia2, xx / a2, answered);
    }

    // (c) no answer inside a band, at its ends, or outside the domain
    for (int i = 0; i + 1 <= np; ++i) {
      const double h = T.edge[2 * i + 1];
      const double l = i + 1 < np ? T.edge[2 * i + 2] : h * 1.5;
      CHECK(decision_lookup(T, h) == 0u, "err %g hi_%d answers", err, i);
      if (i + 1 < np)
        CHECK(decision_lookup(T, std::nextafter(l, 0.0)) == 0u, "err %g below lo_%d", err, i + 1);
      for (int k = 0; k < 1000; ++k) {
        const double tt = h + (l - h) * u(rng);
        if (tt < l) CHECK(decision_lookup(T, tt) == 0u, "err %g band %d tt %.17g", err, i, tt);
      }
    }
    const double outside[] = {std::nextafter(T.edge[0], 0.0), lo / 2, 1e-300, 0.0, -1.0, hi,
                              std::nextafter(hi, 1e300), 2 * hi, 1e300, (double)INFINITY,
                              -(double)INFINITY, (double)NAN};
    for (double tt : outside)
      CHECK(decision_lookup(T, tt) == 0u, "err %g outside tt %g answers", err, tt);

    // (d) the wave's lookup never accepts an interval that holds a breakpoint
    long accepted = 0, straddling = 0;
    auto holds_bp = [&](double a, double b) {
      // (bps holds r of each bracket l < r of adjacent doubles: the decision
      // changes inside [a, b] iff a <= l and r <= b)
      const auto it = std::upper_bound(bps.begin(), bps.end(), a);
      return it != bps.end() && *it <= b;
    };
    for (int it = 0; it < 400000; ++it) {
      double a, b;
      const int kind = it % 4;
      if (kind == 0) {  // anywhere
        a = lo * std::exp(u(rng) * std::log(hi / lo));
        b = a * (1.0 + u(rng));
      } else if (kind == 1) {  // narrow, as a wave's 64 neighbouring |rt|
        a = lo * std::exp(u(rng) * std::log(hi / lo));
        b = a * (1.0 + 1e-3 * u(rng));
      } else {  // ends near two edges (the same one, or neighbours)
        const int e = (int)(rng() % (2 * np));
        const int f = std::min(2 * np - 1, e + (int)(rng() % 3));
        a = T.edge[e] * (1.0 + (2.0 * kDecBand) * (2.0 * u(rng) - 1.0));
        b = T.edge[f] * (1.0 + (2.0 * kDecBand) * (2.0 * u(rng) - 1.0));
        if (b < a) std::swap(a, b);
      }
      const bool bp = holds_bp(a, b);
      if (bp) ++straddling;
      const unsigned c = wave_lookup(T, a, b);
      if (c != 0u) {
        ++accepted;
        CHECK(!bp, "err %g: [%.17g, %.17g] accepted across a breakpoint", err, a, b);
        for (int k = 0; k <= 8; ++k) {
          const double tt = k == 8 ? b : a + (b - a) * (k / 8.0);
          CHECK(code_of(reference(tt, err)) == c, "err %g: [%.17g, %.17g] at %.17g", err, a, b, tt);
        }
      }
    }
    CHECK(accepted > 10000 && straddling > 10000, "err %g accepted %ld straddling %ld", err,
          accepted, straddling);
  }
  // a table that never answers: err outside (0, 1), and the cleared one
  for (double err : {0.0, -1.0, 1.0, 2.0, (double)NAN}) {
    DecisionTab T;
    decision_tab(err, T);
    for (double tt : {1e-6, 0.1, 1.0, 10.0}) CHECK(decision_lookup(T, tt) == 0u, "err %g", err);
  }
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
