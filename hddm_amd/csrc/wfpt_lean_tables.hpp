// wfpt_lean_tables.hpp — the host tables of the lean pass's uniform waves
// (wfpt_lean.hpp), with their claims and proofs: the (grid, K) operands of
// small_grid2d (UniformTab), the per-trial range test that replaces its
// per-node guard (uniform_guard) and the series decision as a breakpoint
// table over tt (DecisionTab). Host + device, no device-only code.
// Compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "wfpt_types.hpp"
#include "wfpt_zgrid.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// Per boundary: the small-time multipliers g_i + 2k of small_grid2d's term
// loop (k2 there is the exact integer 2k, so g_i + k2 is this sum), and per K
// the products of its prologue that depend on (grid, K) alone, in its own
// expressions (contraction off: the bits a lane computes).
constexpr int kUniK = 8;  // small_grid2d's K limit
static_assert(kSinK <= 15 && kUniK <= 15, "K packs into 4 bits per t node");
struct UniformK {
  double u0u0;   // u0 * u0,  u0 = g_0 + (double)(2 lower)
  double hh2;    // h * (2.0 * u0 + h),  h = g_1 - g_0
  double hh;     // h * h
  double u0p1;   // u0 + 1.0
  double h;
  double bound;  // uniform_guard's multiplier of |m| (nondecreasing in K)
};
struct UniformTab {
  double u[9][5];  // u[k + 4][i] = g_i + (double)(2 k), k = -4..4
  UniformK k[kUniK + 1];
  double amax;     // max_i |A_i|
};
__host__ __device__ inline void uniform_tab(const ZGrid& G, UniformTab& T) {
  for (int k = -4; k <= 4; ++k)
    for (int i = 0; i < 5; ++i) T.u[k + 4][i] = G.g[i] + (double)(2 * k);
  const double h = G.g[1] - G.g[0];
  double bound = 0.0;
  T.k[0] = UniformK{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int K = 1; K <= kUniK; ++K) {
    const int lower = (int)(-floor((K - 1) / 2.));
    const int upper = (int)ceil((K - 1) / 2.);
    const double lo2 = (double)(2 * lower);
    const double u0 = G.g[0] + lo2, u4 = G.g[4] + (double)(2 * upper);
    UniformK& C = T.k[K];
    C.u0u0 = u0 * u0;
    C.hh2 = h * (2.0 * u0 + h);
    C.hh = h * h;
    C.u0p1 = u0 + 1.0;
    C.h = h;
    // |m| times this bounds every m-part of small_grid2d's guarded exponents
    // at this K (uniform_guard); the running maximum makes it monotone in K
    const double U = fmax(fabs(u0), fabs(u4)), km1 = (double)(K - 1);
    double b = fmax(U * U, 8.0);
    b = fmax(b, fabs(C.hh2) + 6.0 * C.hh + (4.0 * km1) * fabs(h));
    b = fmax(b, 4.0 * fabs(C.u0p1) + 8.0 * fabs(km1 - 1.0));
    bound = fmax(bound, b);
    C.bound = bound;
  }
  double am = 0.0;
  for (int i = 0; i < 5; ++i) am = fmax(am, fabs(G.A[i]));
  T.amax = am;
}
struct UniformTabs {
  UniformTab U[2];  // per boundary, as RootGrids::G
};
__host__ __device__ inline void uniform_tabs(const RootGrids& R, UniformTabs& T) {
  for (int flip = 0; flip < 2; ++flip) uniform_tab(R.G[flip], T.U[flip]);
}

// One range test per trial in place of small_grid2d's `safe` at each of its
// t nodes (and of tnode_pdf_sv_grid5's `moderate`). It only selects which
// code evaluates the trial, never a value. Arguments: tt4 = tt of t node 4
// (the smallest of the five, > 0), vvx0 = v^2 (x - lb) (the largest v^2 xx),
// bound = UniformK::bound of the largest K among the trial's small-time
// nodes (0 if none), amax = UniformTab::amax.
//
// Claim: if this returns true, `safe` (limit 640) holds at every small-time
// node and |c_i| < 600 at every node. Proof, with M = max_j |m_j|,
// C = max_{i,j} |c_i| over the nodes j:
//   * m_j = -0.5 r^2, r = rsqrt(tt_j), tt_j >= tt4, so M <= (0.5 / tt4)(1 + 1e-15).
//   * c_i = (A_i - dv) dm with 0 <= dv <= v^2 xx <= vvx0 and 0 < dm <= 1
//     (sv = 0: dm = 1; else dm = 0.5 r^2, r = rsqrt(sv^2 xx + 1) <= 1 + 1e-15, so
//     dm <= 0.5 (1 + 1e-15)); rounding is monotone, so C <= Cb (1 + 1e-15) with
//     Cb = (amax + vvx0) (sv = 0 ? 1 : 0.5).
//   * small_grid2d's guarded quantities at a node with K terms, |d1| <= 2C,
//     |d2| <= 4C, h = g_1 - g_0:
//       cmax <= C;   |m U^2 + cmin| <= M U^2 + C;
//       rmax <= |aR| + 3 |aQj| + km1 |aQjk|
//            <= M (|h (2 u0 + h)| + 6 h^2 + 4 km1 |h|) + 14 C;
//       pmax <= |aP| + |km1 - 1| |aQk| = M (4 |u0 + 1| + 8 |km1 - 1|);
//       qmax <= max(2 M h^2 + 4 C, 8 M, 4 M |h|);
//     each is <= M bound_K + 14 C up to a few roundings (relative 1e-15), and
//     bound_K <= bound (the table's running maximum over K).
//   * The test below is (0.5 bound) / tt4 + 14 Cb < 600 multiplied by tt4 > 0,
//     a few roundings again. So every guarded quantity is below
//     600 (1 + 1e-14) < 640, and C <= 600 / 14 < 600.
// A NaN anywhere compares false: the trial then takes the per-node guards.
__host__ __device__ inline bool uniform_guard(double tt4, double vvx0, double sv, double bound,
                                              double amax) {
  const double Cb = (amax + vvx0) * (sv == 0 ? 1.0 : 0.5);
  return 0.5 * bound + (14.0 * Cb) * tt4 < 600.0 * tt4;
}

// The series decision as a table over tt. (small, K) of pdf.pxi:36-60 depends
// on (tt, err) alone and is piecewise constant in tt with a handful of pieces
// (err = 1e-4: small K = 3, small K = 4 from 0.0553, large K = 4 from 0.1537,
// K = 3 from 0.2161, K = 2 from 0.4492, K = 1 from 1.546). The host finds the
// breakpoints once per err (decision_tab) and a wave of the lean pass looks
// up the tt of its two extreme |rt| at each t node instead of estimating
// every lane's decision (table_decisions).
//
// edge[]: lo_0 < hi_0 < lo_1 < hi_1 < ... (unused entries +inf), code[i] =
// small << 4 | K of piece i. A piece whose K exceeds the uniform site's tables
// (kUniK small-time, kSinK large-time) is left out, so is everything outside
// the domain [kDecLo, decision_hi(err)]: the table does not answer there.
//
// Claim: for every tt with lo_i <= tt < hi_i the reference's decision
// (decide64's expressions on the reference's own xx / a2) is piece i's, and
// decide64 does not mark it ambiguous. Argument:
//   * decision_tab brackets every change of the decision between two adjacent
//     doubles l < r (bisection on the fp64 expressions with the host libm,
//     which is what the reference runs), so between two neighbouring brackets
//     the decision is constant, provided it does not leave a piece and come
//     back to it inside one cell of the log-spaced scan (several pieces in a
//     row inside one cell are found one by one). It cannot: on the domain ks
//     is nondecreasing and kl nonincreasing in tt, so `small` flips once and
//     K moves one way on either side; tests/c/lean_decision_host.cpp checks
//     that monotonicity and the pieces against a dense scan for the errs in
//     use.
//   * lo_i = r (1 + kDecBand), hi_i = l (1 - kDecBand) with kDecBand = 1e-6:
//     the lane's tt = (x - tc) * ia2 and the reference's xx / a2 differ by at
//     most 2 ulp (4.5e-16 relative), and a libm whose log differs by an ulp
//     moves a breakpoint by ~1e-15 relative; both are nine orders inside
//     the band. Conversely a tt at least 1e-6 (relative) from a breakpoint
//     leaves ks - kl and kk - rint(kk) further than ~1e-7 from zero (their
//     slopes in log tt are of order 0.1 to 10 on the domain), far outside
//     decide64's 1e-12 ambiguity zone; the host test checks that too.
//   * decide64's other two ambiguity tests, arg_l = 1 and arg_s = 1, are no
//     decision changes; the domain ends at half the smaller of the two tt
//     they occur at (decision_hi), so no tt of the table is near them.
// (kDecBand is below decide32's own 1e-5 zone for tidiness only.)
constexpr int kDecPieces = 32;  // 2 edges per piece: one edge per lane
constexpr double kDecLo = 1e-6, kDecHiMax = 1e3, kDecBand = 1e-6;
struct DecisionTab {
  double edge[2 * kDecPieces];
  unsigned code[kDecPieces];
};
inline void decision_tab_clear(DecisionTab& T) {
  for (int e = 0; e < 2 * kDecPieces; ++e) T.edge[e] = __builtin_inf();
  for (int i = 0; i < kDecPieces; ++i) T.code[i] = 0u;
}
// The reference's decision with the host libm, as a piece code: decide64's
// expressions; 0 for a K outside the uniform site's tables (or a NaN).
inline unsigned decision_code(double tt, double err) {
  double kl, ks;
  const double sqt = sqrt(tt);
  const double inv_pi_sqt = 1. / (kPi * sqt);
  const double arg_l = (kPi * tt) * err;
  const double arg_s = (2.0 * sqrt((2.0 * kPi) * tt)) * err;
  if (arg_l < 1.0) {
    kl = sqrt((-2.0 * log(arg_l)) / (kPi2 * tt));
    kl = (kl < inv_pi_sqt) ? inv_pi_sqt : kl;
  } else {
    kl = inv_pi_sqt;
  }
  if (arg_s < 1.0) {
    ks = 2.0 + sqrt((-2.0 * tt) * log(arg_s));
    const double b = sqt + 1.0;
    ks = (ks < b) ? b : ks;
  } else {
    ks = 2.0;
  }
  const bool small = ks < kl;
  const double ck = ceil(small ? ks : kl);
  if (!(ck >= 1.0 && ck <= (double)(small ? kUniK : kSinK))) return 0u;
  return (small ? 16u : 0u) | (unsigned)(int)ck;
}
// The table's upper end: half the smaller tt at which arg_l or arg_s reaches 1.
inline double decision_hi(double err) {
  return fmin(kDecHiMax, fmin(0.5 / (kPi * err), 0.5 / ((8.0 * kPi) * (err * err))));
}
inline void decision_tab(double err, DecisionTab& T) {
  decision_tab_clear(T);
  if (!(err > 0.0 && err < 1.0)) return;
  const double lo = kDecLo, hi = decision_hi(err);
  if (!(lo < hi)) return;
  constexpr int kCells = 2048;
  const double step = log(hi / lo) / kCells;
  int np = 0;
  bool full = false;
  auto emit = [&](double s, double e, unsigned code) {
    if (code == 0u || !(s < e)) return;
    if (np == kDecPieces) {
      full = true;
      return;
    }
    T.edge[2 * np] = s;
    T.edge[2 * np + 1] = e;
    T.code[np] = code;
    ++np;
  };
  double start = lo, a = lo;
  unsigned ca = decision_code(a, err);
  for (int i = 1; i <= kCells; ++i) {
    const double b = i == kCells ? hi : lo * exp(step * i);
    const unsigned cb = decision_code(b, err);
    while (ca != cb) {
      // adjacent doubles l < r with the piece's code at l and another at r
      double l = a, r = b;
      for (;;) {
        const double m = l + (r - l) * 0.5;
        if (!(l < m && m < r)) break;
        if (decision_code(m, err) == ca) l = m;
        else r = m;
      }
      emit(start, l * (1.0 - kDecBand), ca);
      start = r * (1.0 + kDecBand);
      a = r;
      ca = decision_code(r, err);
    }
    a = b;
  }
  emit(start, hi, ca);
  if (full) decision_tab_clear(T);  // more pieces than lanes: never answers
}
// The table's answer for one tt, as a wave forms it (table_decisions): the
// number of edges <= tt is odd inside a piece. The host tests use it.
inline unsigned decision_lookup(const DecisionTab& T, double tt, int* count = nullptr) {
  int n = 0;
  for (int e = 0; e < 2 * kDecPieces; ++e) n += T.edge[e] <= tt ? 1 : 0;
  if (count) *count = n;
  return (n & 1) ? T.code[(n >> 1) & (kDecPieces - 1)] : 0u;
}

// Dispatch order of the lean pass. A wave whose 64 |rt| straddle a breakpoint
// of the table at some t node cannot be uniform: it runs the per-lane site,
// about twice a uniform wave's time, and one dispatched in the launch's last
// round ends after every uniform wave. The host predicts those chunks from a
// small index of the dataset and the kernel dispatches them first
// (lean_kernel: LeanFirst). A prediction only: a chunk listed wrongly, or
// missed, changes nothing but the order in which chunks are taken.
constexpr int kLeanFirstMax = 64;
struct LeanFirst {
  int n;  // 0: chunks in their stored order
  int c[kLeanFirstMax];
};
// The index of a dataset in stored order (lower boundary first, |rt| ascending
// inside a boundary, NaN RTs last among the lower boundary's): the first |rt|
// of every 64-trial chunk and where the boundaries begin and end.
struct LeanIndex {
  const double* first;  // [nw] |rt| of trial 64 c
  int64_t nw;           // chunks
  int64_t lower_n;      // lower-boundary trials with a non-NaN RT: [0, lower_n)
  int64_t upper;        // the first upper-boundary trial (n: none), upper-boundary trials: [upper, n)
  int64_t n;
  double upper_first;   // |rt| of trial `upper`
  double last[2];       // the largest |rt| of each boundary
};
// x[n]: the trials in stored order; first: (n + 63) / 64 doubles the index keeps.
inline void lean_index(const double* x, int64_t n, double* first, LeanIndex& I) {
  const int64_t nw = (n + 63) / 64;
  for (int64_t w = 0; w < nw; ++w) first[w] = __builtin_fabs(x[w * 64]);
  int64_t up = 0;  // the lower boundary: x <= 0, and the NaN RTs
  while (up < n && !(x[up] > 0)) ++up;
  int64_t ln = up;
  while (ln > 0 && x[ln - 1] != x[ln - 1]) --ln;
  I.first = first;
  I.nw = nw;
  I.n = n;
  I.upper = up;
  I.lower_n = ln;
  I.upper_first = up < n ? __builtin_fabs(x[up]) : 0.0;
  I.last[0] = ln > 0 ? __builtin_fabs(x[ln - 1]) : 0.0;
  I.last[1] = up < n ? __builtin_fabs(x[n - 1]) : 0.0;
}
// The chunk of boundary b (0 lower, 1 upper) that owns |rt| = r: the last one
// whose first |rt| of that boundary is <= r; -1 outside the boundary's data.
// (Chunk c owns everything up to chunk c + 1's first |rt|, so an r between
// two neighbouring chunks' trials names the earlier chunk.)
inline int64_t lean_chunk_of(const LeanIndex& I, int b, double r) {
  int64_t lo, hi;  // chunks (lo, hi) are keyed by first[]; chunk lo by k0
  double k0;
  if (b == 0) {
    if (I.lower_n <= 0) return -1;
    lo = 0;
    hi = (I.lower_n + 63) / 64;
    k0 = I.first[0];
  } else {
    if (I.upper >= I.n) return -1;
    lo = I.upper / 64;
    hi = I.nw;
    k0 = I.upper_first;
  }
  if (!(r >= k0 && r <= I.last[b])) return -1;
  int64_t l = lo, h = hi;  // first[c] <= r for lo < c <= l, first[c] > r for c >= h
  while (h - l > 1) {
    const int64_t m = l + (h - l) / 2;
    if (I.first[m] <= r) l = m;
    else h = m;
  }
  return l;
}
// The chunks that hold a breakpoint: per boundary, t node (the five of
// table_decisions: lb = t - st / 2, ub = t + st / 2 and the three between) and
// finite upper edge of a piece, the chunk that owns tc_j + edge a^2. Sorted,
// without duplicates; of more than kLeanFirstMax the latest in stored order.
inline void lean_first_search(const DecisionTab& D, const LeanIndex& I, double a, double t,
                              double st, LeanFirst& F) {
  F.n = 0;
  for (int k = 0; k < kLeanFirstMax; ++k) F.c[k] = 0;
  if (!I.first || I.nw <= 0) return;
  const double lb = t - st / 2., ub = t + st / 2.;
  const double c = (ub + lb) / 2.;
  const double tc[5] = {lb, (lb + c) / 2., c, (c + ub) / 2., ub};
  const double a2 = a * a;
  int64_t cand[2 * 5 * kDecPieces];
  int nc = 0;
  for (int b = 0; b < 2; ++b)
    for (int j = 0; j < 5; ++j)
      for (int p = 0; p < kDecPieces; ++p) {
        const double e = D.edge[2 * p + 1];
        if (!(e < __builtin_inf())) continue;
        const int64_t ch = lean_chunk_of(I, b, tc[j] + e * a2);
        if (ch < 0) continue;
        int q = nc;  // insertion, ascending, no duplicates
        while (q > 0 && cand[q - 1] > ch) --q;
        if (q > 0 && cand[q - 1] == ch) continue;
        for (int s = nc; s > q; --s) cand[s] = cand[s - 1];
        cand[q] = ch;
        ++nc;
      }
  const int skip = nc > kLeanFirstMax ? nc - kLeanFirstMax : 0;
  F.n = nc - skip;
  for (int k = 0; k < F.n; ++k) F.c[k] = (int)cand[skip + k];
}

}  // namespace wfpt
