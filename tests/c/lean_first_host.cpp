// Host program for tests/test_lean_first_host.py (its own main; built with
// -fsanitize=address,undefined, never loaded into Python): the lean pass's
// dispatch index and breakpoint search (lean_index, lean_chunk_of,
// lean_first_search, hddm_amd/csrc/wfpt_lean_tables.hpp) against a brute-force
// scan of every chunk's own [min, max] of |rt| per boundary.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "../../hddm_amd/csrc/wfpt_lean_tables.hpp"

#pragma clang fp contract(off)

using namespace wfpt;

static int g_fail = 0;
static long g_checked = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    ++g_checked;                            \
    if (!(cond)) {                          \
      if (g_fail < 20) {                    \
        std::printf("FAIL %s: ", #cond);    \
        std::printf(__VA_ARGS__);           \
        std::printf("\n");                  \
      }                                     \
      ++g_fail;                             \
    }                                       \
  } while (0)

// The stored order of a dataset (capi_core.cpp: order_key with upper_last):
// x <= 0 and NaN first (NaN last among them), then x > 0; |rt| ascending.
static std::vector<double> stored_order(std::vector<double> x) {
  auto key = [](double r) {
    const int grp = r > 0 ? 1 : 0;
    const bool nan = std::isnan(r);
    return std::make_tuple(grp, nan ? 1 : 0, nan ? 0.0 : std::fabs(r));
  };
  std::stable_sort(x.begin(), x.end(), [&](double a, double b) { return key(a) < key(b); });
  return x;
}

struct ChunkRange {
  double lo[2], hi[2];
  bool any[2];
};
// every chunk's own [min, max] of |rt| per boundary, from the data alone
static std::vector<ChunkRange> chunk_ranges(const std::vector<double>& x) {
  const int64_t n = (int64_t)x.size(), nw = (n + 63) / 64;
  std::vector<ChunkRange> R(nw);
  for (int64_t c = 0; c < nw; ++c) {
    for (int b = 0; b < 2; ++b) {
      R[c].any[b] = false;
      R[c].lo[b] = std::numeric_limits<double>::infinity();
      R[c].hi[b] = -std::numeric_limits<double>::infinity();
    }
    for (int64_t i = c * 64; i < std::min(n, c * 64 + 64); ++i) {
      if (std::isnan(x[i])) continue;
      const int b = x[i] > 0 ? 1 : 0;
      const double r = std::fabs(x[i]);
      R[c].any[b] = true;
      R[c].lo[b] = std::min(R[c].lo[b], r);
      R[c].hi[b] = std::max(R[c].hi[b], r);
    }
  }
  return R;
}
// Brute force over every chunk: the chunk that owns r for boundary b (the last
// chunk with trials of b whose min is <= r, if r is within b's data), -1
// otherwise; *inside: the number of chunks with min <= r <= max.
static int64_t brute_owner(const std::vector<ChunkRange>& R, int b, double r, int* inside,
                           bool* owner_inside) {
  int64_t own = -1;
  double top = -std::numeric_limits<double>::infinity();
  *inside = 0;
  *owner_inside = false;
  for (int64_t c = 0; c < (int64_t)R.size(); ++c) {
    if (!R[c].any[b]) continue;
    top = std::max(top, R[c].hi[b]);
    if (R[c].lo[b] <= r) own = c;
    if (R[c].lo[b] <= r && r <= R[c].hi[b]) ++*inside;
  }
  if (!(r <= top)) own = -1;
  if (own >= 0) *owner_inside = R[own].lo[b] <= r && r <= R[own].hi[b];
  return own;
}

static void t_nodes(double t, double st, double tc[5]) {
  const double lb = t - st / 2., ub = t + st / 2.;
  const double c = (ub + lb) / 2.;
  tc[0] = lb, tc[1] = (lb + c) / 2., tc[2] = c, tc[3] = (c + ub) / 2., tc[4] = ub;
}

// One dataset, one table, one (a, t, st): the search against the brute force.
// Returns the number of distinct owners (before the cut to kLeanFirstMax).
static int check_one(const char* what, const std::vector<double>& x, const DecisionTab& D, double a,
                     double t, double st) {
  const int64_t n = (int64_t)x.size(), nw = (n + 63) / 64;
  std::vector<double> first(std::max<int64_t>(nw, 1));
  LeanIndex I;
  lean_index(x.data(), n, first.data(), I);
  LeanFirst F;
  std::memset(&F, 0x5a, sizeof F);
  lean_first_search(D, I, a, t, st, F);
  const std::vector<ChunkRange> R = chunk_ranges(x);
  double tc[5];
  t_nodes(t, st, tc);
  std::set<int64_t> owners;
  for (int b = 0; b < 2; ++b)
    for (int j = 0; j < 5; ++j)
      for (int p = 0; p < kDecPieces; ++p) {
        const double e = D.edge[2 * p + 1];
        if (!(e < std::numeric_limits<double>::infinity())) continue;
        const double r = tc[j] + e * (a * a);
        int inside;
        bool oin;
        const int64_t own = brute_owner(R, b, r, &inside, &oin);
        CHECK(own == lean_chunk_of(I, b, r), "%s: b %d j %d piece %d r %.17g: brute %lld search %lld",
              what, b, j, p, r, (long long)own, (long long)lean_chunk_of(I, b, r));
        // a chunk whose own [min, max] holds r is the owner (or ties with it)
        CHECK(inside == 0 || oin, "%s: b %d r %.17g inside %d chunks, the owner not among them", what,
              b, r, inside);
        if (own >= 0) owners.insert(own);
      }
  std::vector<int64_t> want(owners.begin(), owners.end());
  if ((int)want.size() > kLeanFirstMax) want.erase(want.begin(), want.end() - kLeanFirstMax);
  CHECK(F.n == (int)want.size(), "%s: n %d, brute force %d", what, F.n, (int)want.size());
  for (int k = 0; k < F.n && k < (int)want.size(); ++k) {
    CHECK(F.c[k] == want[k], "%s: c[%d] = %d, brute force %lld", what, k, F.c[k], (long long)want[k]);
    CHECK(F.c[k] >= 0 && F.c[k] < nw && (k == 0 || F.c[k] > F.c[k - 1]), "%s: c[%d] = %d", what, k,
          F.c[k]);
  }
  for (int k = F.n; k < kLeanFirstMax; ++k) CHECK(F.c[k] == 0, "%s: c[%d] not cleared", what, k);
  return (int)owners.size();
}

// |rt| spread over [lo, hi] on both boundaries (frac_upper of them upper)
static std::vector<double> sample(std::mt19937_64& g, int64_t n, double lo, double hi,
                                  double frac_upper, int nans) {
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::vector<double> x(n);
  for (int64_t i = 0; i < n; ++i) {
    // denser at short RTs, as RT data is
    const double u = U(g), r = lo + (hi - lo) * u * u;
    x[i] = U(g) < frac_upper ? r : -r;
  }
  for (int k = 0; k < nans && k < n; ++k) x[(k * 977) % n] = std::numeric_limits<double>::quiet_NaN();
  return stored_order(x);
}

int main() {
  std::mt19937_64 g(20261021);
  const double errs[] = {1e-4, 1e-3, 1e-6};
  const double pars[][3] = {  // a, t, st
      {2.0, 0.3, 0.1}, {1.2, 0.25, 0.2}, {0.8, 0.4, 0.05}, {2.5, 0.3, 0.3}, {1.0, 0.2, 1e-3}};
  const int64_t sizes[] = {64 * 48, 3001};
  int nonempty = 0, with_dup = 0;
  for (double err : errs) {
    DecisionTab D;
    decision_tab(err, D);
    for (auto& p : pars)
      for (int64_t n : sizes)
        for (int variant = 0; variant < 5; ++variant) {
          // both boundaries; lower only; upper only; NaN RTs; a 7:3 mix whose
          // boundary switch falls inside a chunk
          const double fu = variant == 1 ? 0.0 : variant == 2 ? 1.0 : variant == 4 ? 0.7 : 0.5;
          const std::vector<double> x = sample(g, n, 0.36, 6.0, fu, variant == 3 ? 5 : 0);
          char what[96];
          std::snprintf(what, sizeof what, "err %g a %g t %g st %g n %lld v%d", err, p[0], p[1], p[2],
                        (long long)n, variant);
          const int k = check_one(what, x, D, p[0], p[1], p[2]);
          nonempty += k > 0;
          // st = 1e-3: the five nodes' breakpoints mostly share a chunk
          if (p[2] == 1e-3 && k > 0 && k < 5) ++with_dup;
        }
  }
  CHECK(nonempty > 100, "only %d searches found a chunk", nonempty);
  CHECK(with_dup > 0, "no case with breakpoints sharing a chunk");

  {  // empty lists: no data, no table, data inside one piece, breakpoints outside the data
    DecisionTab D, E;
    decision_tab(1e-4, D);
    decision_tab_clear(E);
    LeanIndex I{};
    LeanFirst F;
    F.n = 7;
    lean_first_search(D, I, 2.0, 0.3, 0.1, F);
    CHECK(F.n == 0, "no index: n %d", F.n);
    const std::vector<double> x = sample(g, 3001, 0.36, 6.0, 0.5, 0);
    CHECK(check_one("cleared table", x, E, 2.0, 0.3, 0.1) == 0, "a cleared table listed chunks");
    // a = 2, t = 0.3: K = 2 from tt 0.4492 to 1.546 is |rt| 2.15..6.43 at every node
    const std::vector<double> y = sample(g, 3001, 2.6, 5.9, 0.5, 0);
    CHECK(check_one("one piece", y, D, 2.0, 0.3, 0.1) == 0, "data inside one piece listed chunks");
    const std::vector<double> z = sample(g, 3001, 40.0, 90.0, 0.5, 0);
    CHECK(check_one("outside", z, D, 2.0, 0.3, 0.1) == 0, "breakpoints below the data listed chunks");
    std::vector<double> first(64);
    lean_index(y.data(), (int64_t)y.size(), first.data(), I);
    CHECK(lean_chunk_of(I, 0, 2.0) == -1 && lean_chunk_of(I, 1, 7.0) == -1 &&
              lean_chunk_of(I, 0, std::numeric_limits<double>::quiet_NaN()) == -1,
          "r outside the data");
    const std::vector<double> one = {0.5};
    CHECK(check_one("one trial", one, D, 2.0, 0.3, 0.1) >= 0, "one trial");
    const std::vector<double> nan3 = stored_order({std::nan(""), std::nan(""), std::nan("")});
    CHECK(check_one("only NaN", nan3, D, 2.0, 0.3, 0.1) == 0, "NaN RTs listed chunks");
  }

  {  // more than kLeanFirstMax candidates: a table of 32 narrow pieces, 20,000 trials
    DecisionTab D;
    decision_tab_clear(D);
    for (int p = 0; p < kDecPieces; ++p) {
      D.edge[2 * p] = 0.05 + 0.04 * p;
      D.edge[2 * p + 1] = 0.05 + 0.04 * p + 0.03;
      D.code[p] = 1u + (unsigned)(p % 3);
    }
    const std::vector<double> x = sample(g, 20000, 0.36, 6.0, 0.5, 3);
    const int k = check_one("32 pieces", x, D, 2.0, 0.3, 0.1);
    CHECK(k > kLeanFirstMax, "only %d candidates", k);
  }

  if (g_fail) {
    std::printf("%d of %ld checks failed\n", g_fail, g_checked);
    return 1;
  }
  std::printf("%ld checks: all checks passed\n", g_checked);
  return 0;
}
