"""DMAT CDF kernels (cdfdif_kernels.hip) at every series tier, against the oracle.

The reference sums every series in one loop of up to 5000 terms; the kernels
split that loop into tiers (cdfdif_kernels.hip): the quad pass `dmat_cdf_kernel<4>`
(terms v < 48 from an LDS table, DPP quad broadcasts, the deferred list), and
the wave pass `cdf_wave_kernel` (rounds of 64 terms; a global table for v < 512
prefetched one round ahead, computed terms past it; one ballot per round; the
8-term tail round 4992..4999; the window branch's 36 + 6 series in chunks of
8 with rows v < 64 staged in LDS, a global table to 512 and computed terms past
it). tests/test_cdfdif.py's fixtures (a <= 2, no trial within 1e-4 of the
window edge) stop below every deep tier, and its absolute bars could not see
one: cutting the reference's series beyond the window at 512 terms moves F by
4e-10 at most. This module constructs the inputs that reach each tier and
holds the kernels to a bar scaled to the reference's own rounding.

Oracle. `oracle.cdf_probe` is oracle/cdfdif_oracle.c's cdfdif with the series
cap as a parameter (vcap = 5000 is the reference, bit for bit: the existing
entry points run through it, and test_probe_bit_equal_to_oracle_on_fixtures
pins it to both committed fixtures). It returns, per trial, the branch, the
index of the last term each series added (5000: never converged) and S, the
sum of the absolute values of every addend of the wrapper's output after its
multipliers: |p0 (1 - x)|, |p1 x|, every series term, the closed-form parts
(`ser`; sl and su), then |1 - P| and the outlier addend of the fold.
`oracle.dmat_cdf_array_ld` is the same source built in x86-64 long double: it
sums exactly the terms the double run summed, on the double run's branch, with
no test of its own, so the two differ by rounding alone.

Error measure. u(got) = |got - F_ld| / (2^-52 S) on the wrapper's output.
U_ref is the largest u of the oracle's own double build over a test's inputs,
measured where the test runs; the kernel bar is u <= 4 U_ref. Every
non-transcendental operation of the kernels is the reference's IEEE operation
in the reference's order; what differs is OCML's exp / log / sin / cos / sinh /
cosh, whose documented double-precision bounds are a few times glibc's sub-ulp
ones, hence the 4. U_ref is taken separately over a family's well-conditioned
rows (sz, st >= 0.05) and its other rows (see Ref). The absolute bars of
tests/test_cdfdif.py (1e-9 well conditioned, 1e-6 otherwise, against the
double oracle) hold on every comparison as well.

Each family has a CPU test that shows, with the oracle alone, (a) that the
stop indices cover the classes named below and (b) sensitivity: for each tier
boundary B at least 4 trials on each response boundary whose reference value
moves by >= 100 bars (100 * 4 U_ref 2^-52 S) when every series is cut at B, so
an error at that hand-off could not pass. The GPU tests assert the bars on
exactly those inputs.

Measured (glibc 2.35 host, MI355X): U_ref / GPU largest u / largest |dF|
  F1 beyond the window, 7 rows, 309 trials      13.5 / 13.5 / 4.4e-13
     its simple-DDM row (sz = st = 1e-10)       7.37e8 / 7.37e8 / 1.6e-9
  F2 window, drift nodes away from zero, 215    96.2 / 158.8 / 3.1e-14
  F3 window, a drift node at zero, 170          2.35 / 2.35 / 2.5e-12
  F4 edges of cdf_prepare                       |dF| <= 3.8e-15 (sz = st = 0 row: 1.4e-8)
  launch-geometry samples                       <= 3.2 / equal to U_ref / 7.8e-16
F2's 96.2 is the negative-drift row (-1.0, 0.3, 9.0, 0.55, ...) at x = +hi,
where F ~ 1e-3 of S; every other row of F2 is below 2.

Stop-index classes covered. F1: <= 43 and every value 44..51 (last quad step
and hand-off), 63 / 64 / 65, indices = 0 and = 1 mod 64 beyond 64 (128, 129,
192, 193), 127 and 191, 447 / 448 / 449 (last prefetched round), 511 / 512 /
513, 576..1100, 4928..4991, the tail round 4992..4999, and 52 trials that
never converge; sensitive to cuts at 48, 64, 512 and 4992 (the last through
the a = 15 rows: at a <= 4 the last 8 of 5000 terms carry 1e-14 of F, below
any bar). F2: longest series < 64, 64..511, = 7 and = 0 mod 8, every value
505..519 but 517 (no row reaches it), >= 600 (to 1067);
sensitive to cuts at 64 and 512. F3: all six nodes at zero (a = 10: 499 terms,
a = 12: 550) and exactly one node at zero next to 30 (m, i) series; sensitive
to cuts at 8 and, through the mixed rows' (m, i) series, 512. The zero-drift
series itself cannot be made sensitive to a cut at 512 (its terms fall as
v^-4; see F3_ROWS). F4: x = 0, the 0.001 minimum-RT switch to the ulp, hi and
its neighbours, t - st/2 = 0, z -+ sz/2 at 0 and 1, NaN.

The launch-geometry tests check exact equality between GPU results (every
small n against per-branch calls; the quad pass's grid-stride loop at
n = 8192 * 64 + 65; the wave pass's stride loop with 10,000 deferred trials;
calls of different n on one context and in a fresh process) and a sample of
>= 256 outputs of each against the oracle under the same bars.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CDF_ATOL = 1e-9       # tests/test_cdfdif.py: sz and st both >= 0.05
CDF_ATOL_ILL = 1e-6   # otherwise
EPS = 2.0 ** -52
MARGIN = 4            # kernel bar: u <= MARGIN * U_ref
SENS = 100            # a cut at a tier boundary must move F by >= SENS bars

SLOT_BEYOND = 42      # oracle.CDF_SLOT_BEYOND
NEVER = 5000          # oracle.CDF_VMAX as a stop index


def _tol(p):
    return CDF_ATOL if (p[4] >= 0.05 and p[6] >= 0.05) else CDF_ATOL_ILL


def _window(p):
    """(lo, hi) of the Ter window, the oracle's doubles (cdfdif.c:116-120 after
    the wrapper's st + 1e-10)."""
    t, st = p[5], p[6] + 1e-10
    return t - st / 2, t + st / 2


# --------------------------------------------------------------------------
# construction: a deterministic bisection on the offset against the probe's
# stop index (it falls with the offset, to within a term or two)
# --------------------------------------------------------------------------

def _stop_beyond(p, sign, off):
    import oracle
    x = np.array([sign * (_window(p)[1] + off)])
    return int(oracle.cdf_probe(x, *p).stop[0, SLOT_BEYOND])


def _stop_window(p, sign, off):
    import oracle
    x = np.array([sign * (_window(p)[0] + off)])
    return int(oracle.cdf_probe(x, *p).longest[0])


def _bisect(stop, lo, hi, kmin, kmax):
    """An offset in [lo, hi] whose stop index lies in [kmin, kmax], or None and
    the tightest bracket (off_above, stop_above, off_below, stop_below)."""
    slo, shi = stop(lo), stop(hi)
    if kmin <= slo <= kmax:
        return lo, slo
    if kmin <= shi <= kmax:
        return hi, shi
    if not (slo > kmax and shi < kmin):
        return None, (lo, slo, hi, shi)
    for _ in range(70):
        mid = (lo * hi) ** 0.5
        if mid == lo or mid == hi:
            break
        sm = stop(mid)
        if kmin <= sm <= kmax:
            return mid, sm
        if sm > kmax:
            lo, slo = mid, sm
        else:
            hi, shi = mid, sm
    return None, (lo, slo, hi, shi)


class Row:
    """One parameter row with its constructed x."""

    def __init__(self, p, x):
        self.p = tuple(float(q) for q in p)
        self.x = np.ascontiguousarray(x, dtype=np.float64)


# F1: beyond the window. Row 0 is the pinned full model, row 1 the a = 4 row;
# row 2 has a = 0.6 and row 3 p_outlier = 0.05 (z off centre in both, so the
# series has no alternating near-zero terms and reaches even and odd stop
# indices). Row 3's a = 15 is what makes a cut at 4992 visible: the terms
# fall as v^-4 only past v ~ 100 a g / pi, so the larger a and the drift, the
# larger the terms near v = 5000 against S; more drift than this and the
# reference's own sum cancels (S ~ 1e40 at v = 10) and its value is noise.
# Row 4 is the simple DDM, whose sz = st = 1e-10 window puts every offset
# below 1e-3 into branch 0. Rows 5 and 6 are row 3 at other start points:
# consecutive offsets skip stop indices (the terms' signs follow
# sin(pi v z / a)), and these two reach 448, 511 and 513, which row 3 skips.
F1_ROWS = [(0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 0.0, 0.1),
           (1.0, 0.3, 4.0, 0.5, 0.2, 0.4, 0.3, 0.0, 0.1),
           (0.5, 0.1, 0.6, 0.4, 0.1, 0.3, 0.1, 0.0, 0.1),
           (1.0, 0.1, 15.0, 0.45, 0.05, 0.4, 0.05, 0.05, 0.1),
           (0.5, 0.0, 2.0, 0.5, 0.0, 0.3, 0.0, 0.0, 0.1),
           (1.0, 0.1, 15.0, 0.4, 0.05, 0.4, 0.05, 0.0, 0.1),
           (1.0, 0.1, 15.0, 0.48, 0.05, 0.4, 0.05, 0.0, 0.1)]
F1_EXACT = (list(range(40, 53)) + [63, 64, 65, 127, 128, 129, 191, 192, 193, 447, 448, 449,
                                   511, 512, 513])
F1_RANGES = [(576, 1100), (4928, 4991), (4992, 4999)]
F1_NEVER_OFFS = (1e-8, 2e-8, 3e-8, 5e-8, 1e-7)
F1_BOUNDARIES = (48, 64, 512, 4992)


@functools.lru_cache(maxsize=None)
def _f1():
    """rows, and for each exact target that no (row, boundary) reaches the
    nearest reachable neighbours {k: [(row, sign, above, below), ...]}."""
    rows, missed = [], {}
    hit = set()
    for ri, p in enumerate(F1_ROWS):
        simple = p[6] == 0.0
        xs = []
        for sign in (1.0, -1.0):
            stop = functools.partial(_stop_beyond, p, sign)
            lo = 1.0000001e-3 if simple else 1e-9
            for kmin, kmax in [(k, k) for k in F1_EXACT] + F1_RANGES:
                off, info = _bisect(stop, lo, 0.5, kmin, kmax)
                if off is not None:
                    xs.append(sign * (_window(p)[1] + off))
                    hit.add(kmin)
                elif kmin == kmax:
                    missed.setdefault(kmin, []).append((ri, sign, info[1], info[3]))
            if simple:  # offsets below 1e-3: branch 0
                xs += [sign * (_window(p)[1] + o) for o in (1e-4, 9.99e-4)]
            else:
                xs += [sign * (_window(p)[1] + o) for o in F1_NEVER_OFFS]
            xs += [sign * (_window(p)[1] + o) for o in (1e-2, 0.1, 1.0)]  # the quad pass
        rows.append(Row(p, xs))
    return rows, {k: v for k, v in missed.items() if k not in hit}


# F2: inside the window, every drift node away from zero. a = 2, 5, 10, a
# negative-drift row with a = 9, and a = 15. The drift is kept moderate on
# purpose. exp((2x - 1) zz g 100) lifts every term and `ser` alike, so it does
# not make the tail past 512 larger against S; what does is a larger a (the
# terms fall as exp(-(pi v / a)^2 (t - lo) / 200)), hence row 4. More drift
# only makes the reference cancel: at (3.0, 0.5, 10.0, 0.4, 0.2, 0.4, 0.3),
# upper boundary, S = 3.3e9 against F < 1, the double oracle is 1.6e4 units
# (1e-2 in F) from its own long double twin, and a cut at 512 moves F by less
# than that. A row like it would only widen U_ref for every other row.
F2_ROWS = [(0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 0.0, 0.1),
           (1.5, 0.4, 5.0, 0.45, 0.15, 0.35, 0.2, 0.0, 0.1),
           (0.5, 0.5, 10.0, 0.4, 0.2, 0.4, 0.3, 0.0, 0.1),
           (-1.0, 0.3, 9.0, 0.55, 0.2, 0.4, 0.3, 0.0, 0.1),
           (0.5, 0.1, 15.0, 0.4, 0.2, 0.4, 0.3, 0.0, 0.1)]
F2_OFFS = (0.00101, 0.00102, 0.00105, 0.0011, 0.0012, 0.0013, 0.0015, 0.0017, 0.0025, 0.004,
           0.007, 0.012, 0.02, 0.035, 0.06)
F2_EXACT = list(range(505, 520))
F2_BOUNDARIES = (64, 512)


def _window_rows(params, offs, exact, with_hi=True):
    rows = []
    for p in params:
        lo, hi = _window(p)
        xs = []
        for sign in (1.0, -1.0):
            xs += [sign * (lo + o) for o in offs if lo + o < hi]
            if with_hi:
                xs += [sign * (lo + 0.5 * (hi - lo)), sign * hi]
            stop = functools.partial(_stop_window, p, sign)
            for k in exact:
                off, _ = _bisect(stop, 0.00101, hi - lo, k, k)
                if off is not None:
                    xs.append(sign * (lo + off))
        rows.append(Row(p, xs))
    return rows


@functools.lru_cache(maxsize=None)
def _f2():
    return _window_rows(F2_ROWS, F2_OFFS, F2_EXACT)


# F3: a drift node at zero inside the window. Rows 0 and 1: v = sv = 0, all six
# nodes at zero (a = 10 reaches 499 terms, a = 12 passes 512). Rows 2 and 3:
# sv = 1 and v on node 2 (row 3: -v, node 3) of the Gauss-Hermite rule, so
# exactly that node is at zero and lanes 36..41 work alongside lanes 0..35.
# Sensitivity: every row is sensitive to a cut at 8. The zero-drift series
# itself cannot be made sensitive to a cut at 512: its terms fall as v^-4, and
# even at a = 20, where it runs 830 terms, the part past 512 is below 100 bars.
# It is the (m, i) series of the mixed rows that carry a cut at 512: row 2 on
# the upper boundary, its mirror image row 3 on the lower one.
F3_V_MIXED = 1.41421356237309505 * 0.43607741192761650950 * (1.0 + 1e-9)
F3_ROWS = [(0.0, 0.0, 10.0, 0.5, 0.2, 0.4, 0.3, 0.0, 0.1),
           (0.0, 0.0, 12.0, 0.45, 0.2, 0.4, 0.3, 0.0, 0.1),
           (F3_V_MIXED, 1.0, 10.0, 0.7, 0.2, 0.4, 0.3, 0.0, 0.1),
           (-F3_V_MIXED, 1.0, 10.0, 0.3, 0.2, 0.4, 0.3, 0.0, 0.1)]
F3_EXACT = list(range(508, 517))
F3_BOUNDARIES = (8, 512)


@functools.lru_cache(maxsize=None)
def _f3():
    return _window_rows(F3_ROWS, F2_OFFS + (0.1, 0.2), F3_EXACT)


FAMILIES = {"F1": _f1, "F2": _f2, "F3": _f3}


def _rows(name):
    r = FAMILIES[name]()
    return r[0] if isinstance(r, tuple) else r


class Ref:
    """The oracle on a list of rows, computed once: per row the double probe at
    the reference's cap, the long double twin over the same terms and the
    oracle's own u. U_ref is the largest u over these inputs, taken separately
    over the well-conditioned rows (sz and st both >= 0.05, the rule of the
    absolute bars) and over the others: with sz or st replaced by 1e-10 the
    reference cancels inside each term, which S does not see, so its own u is
    ~1e8 there and one pooled figure would be no bar at all for the rest."""

    def __init__(self, rows):
        import oracle
        self.rows = rows
        self.probe = [oracle.cdf_probe(r.x, *r.p) for r in rows]
        self.ld = [oracle.dmat_cdf_array_ld(r.x, *r.p, probe=pr)
                   for r, pr in zip(rows, self.probe)]
        self.u = [_u(pr.out, ld, pr.S) for pr, ld in zip(self.probe, self.ld)]
        self.U = self._pool(True)
        self.U_ill = self._pool(False)

    def _pool(self, well):
        return max([float(np.nanmax(u)) for r, u in zip(self.rows, self.u)
                    if (_tol(r.p) == CDF_ATOL) == well], default=0.0)

    def U_of(self, row):
        return self.U if _tol(row.p) == CDF_ATOL else self.U_ill


def _u(got, ld, S):
    """|got - F_ld| / (2^-52 S) per trial (NaN where the output is NaN)."""
    d = np.abs(np.asarray(got, dtype=np.longdouble) - ld)
    return (d / (np.longdouble(EPS) * S.astype(np.longdouble))).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _ref(name):
    return Ref(_rows(name))


def _sensitive(name, boundaries):
    """Condition (b): per tier boundary B, the trials on each response boundary
    whose reference value moves by >= SENS bars when every series is cut at B.
    Returns {B: {sign: [(row, x, stop, move / bar), ...]}}."""
    import oracle
    ref = _ref(name)
    out = {}
    for B in boundaries:
        per = {1: [], -1: []}
        for ri, (r, pr) in enumerate(zip(ref.rows, ref.probe)):
            cut = oracle.cdf_probe(r.x, *r.p, vcap=B)
            bar = MARGIN * ref.U_of(r) * EPS * pr.S
            move = np.abs(cut.out - pr.out)
            for j in np.nonzero(move >= SENS * bar)[0]:
                per[1 if r.x[j] > 0 else -1].append(
                    (ri, float(r.x[j]), int(pr.longest[j]), float(move[j] / bar[j])))
        out[B] = per
    return out


def _report_sensitive(name, sens):
    for B, per in sens.items():
        for sign, tr in per.items():
            best = sorted(tr, key=lambda q: -q[3])[:4]
            print(f"{name} cut at {B:4d}, boundary {'upper' if sign > 0 else 'lower'}: "
                  f"{len(tr)} trials >= {SENS} bars; largest: "
                  + ", ".join(f"row {ri} x={x!r} stop {s} ({m:.3g} bars)" for ri, x, s, m in best))


def _assert_sensitive(name, sens, boundaries=None):
    for B in (boundaries or sens):
        for sign in (1, -1):
            assert len(sens[B][sign]) >= 4, (name, B, sign, len(sens[B][sign]))


def _report_ref(name):
    ref = _ref(name)
    for ri, (r, pr, u) in enumerate(zip(ref.rows, ref.probe, ref.u)):
        print(f"{name} row {ri} {r.p}: n={r.x.size} stops {int(pr.longest.min())}.."
              f"{int(pr.longest.max())} max S={pr.S.max():.3g} oracle max u={np.nanmax(u):.3g}")
    print(f"{name}: U_ref = {ref.U:.4g} (ill-conditioned rows: {ref.U_ill:.4g}) over "
          f"{sum(r.x.size for r in ref.rows)} trials")
    return ref


# --------------------------------------------------------------------------
# CPU tests: the probe, the twin, and per family coverage / sensitivity / U_ref
# --------------------------------------------------------------------------

def test_probe_bit_equal_to_oracle_on_fixtures(oracle_lib):
    """The probe at vcap = 5000 gives the existing oracle's outputs bit for bit
    on both committed fixtures (which test_cdfdif.py pins to the reference), a
    double replay of its record reproduces F and S bit for bit, and the long
    double twin agrees with the double build to rounding."""
    n = 0
    worst = 0.0
    for fn in ("cdfdif", "cdfdif_random"):
        g = np.load(os.path.join(ROOT, "tests", "golden", fn + ".npz"), allow_pickle=False)
        for p, x, y in zip(g["params"], g["x"], g["y"]):
            pr = oracle_lib.cdf_probe(x, *p)
            assert np.array_equal(pr.out, y, equal_nan=True), (fn, p)
            assert np.array_equal(pr.out, oracle_lib.dmat_cdf_array(x, *p), equal_nan=True)
            n += x.size
            if fn == "cdfdif" and _tol(p) == CDF_ATOL:
                ld = oracle_lib.dmat_cdf_array_ld(x, *p, probe=pr)
                ok = np.isfinite(pr.out)
                worst = max(worst, float(_u(pr.out, ld, pr.S)[ok].max()))
                assert np.abs(pr.out[ok] - ld[ok]).max() <= CDF_ATOL, (fn, p)
    assert n > 20000
    print(f"oracle double vs long double on cdfdif.npz, well-conditioned rows: max u = "
          f"{worst:.3g}")
    assert worst > 0
    # a replay of the record in double: the same F, S and prob
    v, sv, a, z, sz, t, st = 0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1
    par = [a / 10., t, sv / 10. + 1e-10, z * (a / 10.), sz * (a / 10.) + 1e-10, st + 1e-10, v / 10.]
    for tt, bnd in ((0.36, 1), (0.3500501, 0), (0.3, 1), (0.28, 0), (0.2, 1)):
        F, S, prob, branch, stop = oracle_lib.cdfdif_probe(tt, bnd, par)
        assert oracle_lib.cdfdif_probe(tt, bnd, par, replay=(branch, stop))[:3] == (F, S, prob)
        assert S >= abs(F)
    # a cap is a cap: no stop index reaches it, and 5000 is the reference's
    x = np.array([0.3501, -0.3501, 0.31, -0.26])
    p = (0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 0.0, 0.1)
    cut = oracle_lib.cdf_probe(x, *p, vcap=20)
    assert cut.stop.max() == NEVER and not np.array_equal(cut.out, oracle_lib.cdf_probe(x, *p).out)


def test_f1_beyond_window_reference(oracle_lib):
    """F1 with the oracle alone: (a) the stop indices cover every class of the
    quad pass, the hand-off and the wave pass's rounds; (b) cuts at 48, 64,
    512 and 4992 each move >= 4 trials per response boundary by >= 100 bars."""
    rows, missed = _f1()
    ref = _report_ref("F1")
    stops = np.concatenate([pr.stop[:, SLOT_BEYOND] for pr in ref.probe])
    have = set(int(s) for s in stops)
    for ri, pr in enumerate(ref.probe):
        assert np.all((pr.branch == 1) | (ri == 4)), ri
    assert np.sum(ref.probe[4].branch == 0) == 4 and np.sum(ref.probe[4].branch == 1) > 20
    assert min(have - {-1}) <= 43
    print("F1 exact targets that no row reaches, with their nearest neighbours:", missed)

    def shown(k):  # reached, or skipped by consecutive offsets with both neighbours in
        return k in have or any(above in have and below in have and above > k > below
                                for _, _, above, below in missed.get(k, []))
    for k in list(range(44, 52)) + [63, 64, 65, 447, 448, 449, 511, 512, 513]:
        assert shown(k), k
    assert any(k > 64 and k % 64 == 0 for k in have)       # last == 0
    assert any(k > 64 and k % 64 == 1 for k in have)       # last == 1
    assert 127 in have or 191 in have                      # last == 63
    assert any(576 <= k <= 1100 for k in have)
    assert any(4928 <= k <= 4991 for k in have)
    assert any(4992 <= k <= 4999 for k in have)            # the 8-term tail round
    assert int(np.sum(stops == NEVER)) >= 3
    sens = _sensitive("F1", F1_BOUNDARIES)
    _report_sensitive("F1", sens)
    _assert_sensitive("F1", sens)
    assert ref.U <= U_CEILING["F1"], ref.U


def test_f2_window_reference(oracle_lib):
    """F2 with the oracle alone: the longest series of the trials covers the
    staged rows (< 64), the global table (64..511), both chunk edges, both
    sides of kWinTerms and the computed branch (>= 600); cuts at 64 and 512
    each move >= 4 trials per response boundary by >= 100 bars."""
    ref = _report_ref("F2")
    for pr in ref.probe:
        assert np.all(pr.branch == 2)
        assert np.all(pr.stop[:, 36:] == -1) and np.all(pr.stop[:, :36] >= 0)
    longest = np.concatenate([pr.longest for pr in ref.probe])
    have = set(int(s) for s in longest)
    assert any(k < 64 for k in have)
    assert any(64 <= k <= 511 for k in have)
    assert any(k % 8 == 7 for k in have) and any(k % 8 == 0 for k in have)
    assert any(505 <= k <= 511 for k in have) and any(512 <= k <= 519 for k in have)
    assert 511 in have and 512 in have
    assert any(k >= 600 for k in have)
    for r in ref.rows:  # hi itself is in, on both boundaries
        assert _window(r.p)[1] in r.x and -_window(r.p)[1] in r.x
    sens = _sensitive("F2", F2_BOUNDARIES)
    _report_sensitive("F2", sens)
    _assert_sensitive("F2", sens)
    assert ref.U <= U_CEILING["F2"], ref.U


# U_ref is measured at run time (it moves a little with the host libm); these
# ceilings, four times the values in the module docstring, keep it from
# turning into a looser bar unnoticed.
U_CEILING = {"F1": 64.0, "F2": 512.0, "F3": 16.0}


def test_f3_zero_drift_node_reference(oracle_lib):
    """F3 with the oracle alone: rows 0 and 1 run only the zero-drift series
    (one per node, lanes 36..41), rows 2 and 3 exactly one of them next to 30
    (m, i) series; the zero-drift series reaches both sides of 512; cuts at 8
    and 512 each move >= 4 trials per response boundary by >= 100 bars."""
    ref = _report_ref("F3")
    gh = [-2.3506049736744922818, -1.3358490740136970132, -.43607741192761650950,
          .43607741192761650950, 1.3358490740136970132, 2.3506049736744922818]
    for ri, (r, pr) in enumerate(zip(ref.rows, ref.probe)):
        assert np.all(pr.branch == 2)
        zero = pr.stop[:, 36:42] >= 0
        if ri < 2:
            assert np.all(zero) and np.all(pr.stop[:, :36] == -1)
            continue
        # the oracle's |gk[m]| <= 1e-7 holds for exactly one m of a mixed row
        v, sv = r.p[0], r.p[1]
        gk = [1.41421356237309505 * g * (sv / 10. + 1e-10) + v / 10. for g in gh]
        assert [abs(g) <= 1e-7 for g in gk] == [m == ri for m in range(6)]
        assert np.all(zero.sum(axis=1) == 1) and np.all(zero[:, ri])
        assert np.all((pr.stop[:, :36] >= 0).sum(axis=1) == 30)
    zs = np.concatenate([pr.stop[:, 36:42].max(axis=1) for pr in ref.probe[:2]])
    have = set(int(s) for s in zs)
    assert any(k <= 511 for k in have) and any(k >= 512 for k in have)
    assert 499 in set(int(s) for s in ref.probe[0].stop[:, 36:42].max(axis=1))
    sens = _sensitive("F3", F3_BOUNDARIES)
    _report_sensitive("F3", sens)
    _assert_sensitive("F3", sens, F3_SENSITIVE)
    assert ref.U <= U_CEILING["F3"], ref.U


F3_SENSITIVE = (8, 512)


# F4: the edges of cdf_prepare. Every comparison is exact on the branch taken
# (the same IEEE comparisons on the same doubles), so the value is held to
# the ordinary bars; a wrong branch moves F by far more than either.
def _ulps(x, ks):
    out = []
    for k in ks:
        y = x
        for _ in range(abs(k)):
            y = np.nextafter(y, np.inf if k > 0 else -np.inf)
        out.append(float(y))
    return out


def _first_inside(p):
    """The smallest |x| that the reference does not put below the window (its
    t - Ter + st/2 > 0.001 in doubles), by bisection over the doubles."""
    import oracle
    lo = _window(p)[0]
    below, inside = lo + 0.0009, lo + 0.0011
    while np.nextafter(below, np.inf) < inside:
        mid = below + 0.5 * (inside - below)
        if oracle.cdf_probe(np.array([mid]), *p).branch[0] == 0:
            below = mid
        else:
            inside = mid
    return float(inside)


F4_ULPS = (-7, -3, -2, -1, 0, 1, 2, 3, 7)


@functools.lru_cache(maxsize=None)
def _f4():
    rows = []
    ks = F4_ULPS
    for p in [(0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 0.0, 0.1),       # the pinned model
              (0.5, 0.1, 2.0, 0.5, 0.1, 0.15, 0.3, 0.0, 0.1),      # t - st/2 = 0
              (0.5, 0.1, 2.0, 0.1, 0.2, 0.3, 0.1, 0.0, 0.1),       # z - sz/2 = 0
              (0.5, 0.1, 2.0, 0.9, 0.2, 0.3, 0.1, 0.05, 0.1),      # z + sz/2 = 1, outliers
              (-1.0, 0.0, 1.5, 0.5, 0.0, 0.3, 0.0, 0.0, 0.1)]:     # sz = st = 0
        lo, hi = _window(p)
        mag = ([0.0] + _ulps(_first_inside(p), ks) + _ulps(hi, ks)
               + [lo + 0.5 * (hi - lo), hi + 0.01, hi + 0.5, 1e-300, 4.9])
        if lo > 0:
            mag += [lo, 0.5 * lo]
        x = [s * m for m in mag for s in (1.0, -1.0)]
        if p[7] == 0:  # with p_outlier > 0 the wrapper's RT assertion rejects a NaN
            x.append(np.nan)
        rows.append(Row(p, x))
    return rows


def test_f4_prepare_edges_reference(oracle_lib):
    """F4 with the oracle alone: the inputs take all three branches on both
    sides of each edge, hi itself is inside the window, and NaN stays NaN."""
    for r in _f4():
        pr = oracle_lib.cdf_probe(r.x, *r.p)
        lo, hi = _window(r.p)
        ax = np.abs(r.x)
        # a window of st + 1e-10 <= 0.001 has no inside: below it up to hi, beyond past it
        inside = 2 if hi - lo > 0.001 else 0
        fin = ~np.isnan(r.x)
        assert set(pr.branch[fin]) == {0, 1, inside}
        assert np.all(pr.branch[ax == hi] == inside)
        assert np.all(pr.branch[ax == np.nextafter(hi, np.inf)] == (1 if inside else 0))
        assert np.all(pr.branch[ax == np.nextafter(hi, -np.inf)] == inside)
        edge = _ulps(_first_inside(r.p), F4_ULPS)
        assert abs(edge[4] - (lo + 0.001)) < 1e-15
        b = [int(pr.branch[np.nonzero(r.x == e)[0][0]]) for e in edge]
        # the switch, to the ulp (past a 1e-10 window it is into branch 1)
        assert b == [0 if k < 0 else (inside or 1) for k in F4_ULPS], b
        assert np.array_equal(np.isnan(pr.out), ~fin) and np.all(pr.branch[~fin] == 0)
        if r.p[7] == 0:  # F = 0 below the window: every such output is 1 - P(upper)
            assert np.sum(~fin) == 1
            assert np.all(pr.out[fin & (pr.branch == 0)] == pr.out[0])
        assert np.array_equal(pr.out, oracle_lib.dmat_cdf_array(r.x, *r.p), equal_nan=True)


# --------------------------------------------------------------------------
# GPU tests
# --------------------------------------------------------------------------

def _gpu_against(name, rows, ref):
    """The bars of the module docstring on `rows`: u <= MARGIN * U_ref against
    the long double twin and the absolute bars against the double oracle.
    Prints every figure, then asserts."""
    from hddm_amd import cdfdif_wrapper as cw
    bad = []
    top_u = top_d = 0.0
    for ri, (r, pr, ld) in enumerate(zip(rows, ref.probe, ref.ld)):
        got = cw.dmat_cdf_array(r.x, *r.p)
        u = _u(got, ld, pr.S)
        d = np.abs(got - pr.out)
        fin = ~np.isnan(pr.out)
        assert np.array_equal(np.isnan(got), ~fin), (name, ri)
        j, k = int(np.argmax(u[fin])), int(np.argmax(d[fin]))
        print(f"{name} row {ri}: GPU max u = {u[fin][j]:.4g} (x={float(r.x[fin][j])!r}, stop "
              f"{int(pr.longest[fin][j])}), max |dF| = {d[fin][k]:.3e} (x={float(r.x[fin][k])!r}); "
              f"bar u <= {MARGIN * ref.U_of(r):.4g}, |dF| <= {_tol(r.p):.0e}")
        top_u, top_d = max(top_u, float(u[fin][j])), max(top_d, float(d[fin][k]))
        for j in np.nonzero(fin & ((u > MARGIN * ref.U_of(r)) | (d > _tol(r.p))))[0]:
            bad.append((ri, float(r.x[j]), int(pr.longest[j]), float(u[j]), float(d[j])))
    print(f"{name}: U_ref = {ref.U:.4g}, GPU largest u = {top_u:.4g}, largest |dF| = {top_d:.3e}")
    assert not bad, f"{name}: (row, x, stop, u, |dF|) over the bars: {bad[:20]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["F1", "F2", "F3"])
def test_family_on_gpu(name):
    _gpu_against(name, _rows(name), _ref(name))


@pytest.mark.gpu
def test_f4_prepare_edges_on_gpu():
    import oracle
    from hddm_amd import cdfdif_wrapper as cw
    for ri, r in enumerate(_f4()):
        ref = oracle.dmat_cdf_array(r.x, *r.p)
        got = cw.dmat_cdf_array(r.x, *r.p)
        fin = ~np.isnan(r.x)
        assert np.array_equal(np.isnan(got), ~fin)
        d = np.abs(got[fin] - ref[fin])
        print(f"F4 row {ri}: max |dF| = {d.max():.3e} at x={float(r.x[fin][int(d.argmax())])!r}")
        assert d.max() <= _tol(r.p), (ri, r.x[fin][int(d.argmax())], d.max())
        below = fin & (oracle.cdf_probe(r.x, *r.p).branch == 0)
        if r.p[7] == 0:  # F = 0, no series ran: the output is 1 - P(upper), as at x = 0
            assert np.all(got[below] == got[0])


# launch geometry: the pinned model, the three branches interleaved so that a
# quad's neighbours, and the 16 trials of a wave, take different branches
GEO_P = (0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 0.0, 0.1)


def _mixed_pool(n, seed):
    """n distinct |x| with signs, cycling below / beyond (quick) / window /
    beyond (deferred: stop 48..135) / beyond (quick) by position."""
    rng = np.random.default_rng(seed)
    lo, hi = _window(GEO_P)
    kind = np.arange(n) % 5
    mag = np.where(kind == 0, rng.uniform(0.0, lo + 0.0009, n),
          np.where(kind == 1, hi + rng.uniform(0.02, 3.0, n),
          np.where(kind == 2, lo + rng.uniform(0.02, hi - lo, n),
          np.where(kind == 3, hi + rng.uniform(1e-3, 5e-3, n),
                   hi + rng.uniform(0.05, 1.0, n)))))
    return mag * rng.choice([-1.0, 1.0], n), kind


def _sample_against(name, x, got, p=GEO_P):
    """§2 on a sample: x[:] (>= 256 values) against the oracle."""
    import oracle
    assert x.size >= 256
    pr = oracle.cdf_probe(x, *p)
    ld = oracle.dmat_cdf_array_ld(x, *p, probe=pr)
    U = float(_u(pr.out, ld, pr.S).max())
    u = _u(got, ld, pr.S)
    d = np.abs(got - pr.out)
    print(f"{name}: sample of {x.size}: U_ref = {U:.4g}, GPU max u = {u.max():.4g}, "
          f"max |dF| = {d.max():.3e}")
    assert u.max() <= MARGIN * U, (name, float(x[int(u.argmax())]), u.max(), U)
    assert d.max() <= _tol(p), (name, float(x[int(d.argmax())]), d.max())


@pytest.mark.gpu
def test_every_small_size_is_position_independent():
    """n = 1..9, 63..65, 255..257 of interleaved branches: every output equals
    that x evaluated in a call of its own branch's array."""
    from hddm_amd import cdfdif_wrapper as cw
    x, kind = _mixed_pool(257, 11)
    own = np.empty_like(x)
    for k in (0, 2):
        own[kind == k] = cw.dmat_cdf_array(np.ascontiguousarray(x[kind == k]), *GEO_P)
    quick = (kind == 1) | (kind == 4)
    own[quick] = cw.dmat_cdf_array(np.ascontiguousarray(x[quick]), *GEO_P)
    own[kind == 3] = cw.dmat_cdf_array(np.ascontiguousarray(x[kind == 3]), *GEO_P)
    for n in list(range(1, 10)) + [63, 64, 65, 255, 256, 257]:
        got = cw.dmat_cdf_array(np.ascontiguousarray(x[:n]), *GEO_P)
        assert np.array_equal(got, own[:n]), (n, np.nonzero(got != own[:n])[0][:8])
        # and from the other end, so every value meets other neighbours
        got = cw.dmat_cdf_array(np.ascontiguousarray(x[257 - n:]), *GEO_P)
        assert np.array_equal(got, own[257 - n:]), n
    _sample_against("small sizes", x, own)


@pytest.mark.gpu
def test_quad_pass_grid_stride_loop():
    """n = 8192 * 64 + 65 > 8192 blocks of 64 trials: the quad pass strides.
    4,099 distinct values (prime: the tiling does not align with blocks), at
    most 1% deferred; every output equals its source element's from a
    4,099-long call."""
    import oracle
    from hddm_amd import cdfdif_wrapper as cw
    rng = np.random.default_rng(12)
    lo, hi = _window(GEO_P)
    m = 4099
    base = (hi + rng.uniform(0.02, 3.0, m)) * rng.choice([-1.0, 1.0], m)
    base[::7] = rng.uniform(0.0, lo + 0.0009, base[::7].size)              # below the window
    slow = rng.choice(m, 36, replace=False)
    base[slow[:18]] = lo + rng.uniform(0.02, hi - lo, 18)                  # window: deferred
    base[slow[18:]] = -(hi + rng.uniform(1e-3, 5e-3, 18))                  # stop >= 48: deferred
    pr = oracle.cdf_probe(base, *GEO_P)
    deferred = (pr.branch == 2) | (pr.stop[:, SLOT_BEYOND] >= 48)
    assert 30 <= deferred.sum() <= m // 100
    n = 8192 * 64 + 65
    src = np.arange(n) % m
    small = cw.dmat_cdf_array(base, *GEO_P)
    big = cw.dmat_cdf_array(np.ascontiguousarray(base[src]), *GEO_P)
    bad = np.nonzero(big != small[src])[0]
    assert bad.size == 0, (bad.size, bad[:8])
    pick = np.concatenate([np.nonzero(deferred)[0], np.arange(0, m, 18)])[:264]
    _sample_against("quad grid stride", np.ascontiguousarray(base[pick]), small[pick])


def _all_deferred(n, seed, window):
    rng = np.random.default_rng(seed)
    lo, hi = _window(GEO_P)
    x = (hi + rng.uniform(1e-3, 5e-3, n)) * rng.choice([-1.0, 1.0], n)
    w = np.nonzero(window)[0]
    x[w] = (lo + rng.uniform(0.02, hi - lo, w.size)) * rng.choice([-1.0, 1.0], w.size)
    x[w[::9]] = np.sign(x[w[::9]]) * hi                                    # hi itself
    return x


@pytest.mark.gpu
def test_wave_pass_stride_loop():
    """10,000 trials that all defer (stop 48..135; window trials at
    lo + 0.02 .. hi) on the 4096-wave grid: tiled from 257 distinct values and
    equal to the 257-long call; then a call whose first 9,000 trials are
    beyond the window, so every wave stages its window rows only after it has
    run beyond-window trials."""
    import oracle
    from hddm_amd import cdfdif_wrapper as cw
    m = 257
    base = _all_deferred(m, 13, np.arange(m) % 3 == 1)
    pr = oracle.cdf_probe(base, *GEO_P)
    assert np.all((pr.branch == 2) | (pr.stop[:, SLOT_BEYOND] >= 48))
    assert pr.longest.max() <= 140
    small = cw.dmat_cdf_array(base, *GEO_P)
    src = np.arange(10000) % m
    big = cw.dmat_cdf_array(np.ascontiguousarray(base[src]), *GEO_P)
    bad = np.nonzero(big != small[src])[0]
    assert bad.size == 0, (bad.size, bad[:8])
    _sample_against("wave stride", base, small)
    # beyond-window trials first, window trials only past the first 4096 deferred
    late = _all_deferred(10000, 14, np.arange(10000) >= 9000)
    got = cw.dmat_cdf_array(late, *GEO_P)
    pick = np.concatenate([np.arange(0, 9000, 60), np.arange(9000, 10000, 8)])
    each = cw.dmat_cdf_array(np.ascontiguousarray(late[pick]), *GEO_P)
    assert np.array_equal(got[pick], each)
    _sample_against("window after beyond", np.ascontiguousarray(late[pick]), got[pick])


SEQ_ROWS = [(0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 0.0, 0.1),
            (1.0, 0.3, 4.0, 0.5, 0.2, 0.4, 0.3, 0.0, 0.1),
            (-0.8, 0.2, 1.4, 0.45, 0.15, 0.25, 0.2, 0.05, 0.1)]
SEQ_B = [0.4000001, -0.7, 0.26]

_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from hddm_amd import cdfdif_wrapper as cw
x = np.array(json.loads(sys.argv[2]))
p = json.loads(sys.argv[3])
print(json.dumps([float(y).hex() for y in cw.dmat_cdf_array(x, *p)]))
"""


def _seq_x(n, p, seed):
    rng = np.random.default_rng(seed)
    lo, hi = _window(p)
    x = (lo + rng.gamma(2.0, 0.2, n)).clip(0.0, 4.5) * rng.choice([-1.0, 1.0], n)
    x[::50] = np.sign(x[::50]) * (hi + 2e-3)    # some deferred trials beyond the window
    return x


@pytest.mark.gpu
def test_call_sequence_on_one_context():
    """A (n = 50,000), B (n = 3), C (n = 50,001, p_outlier > 0), A, B on one
    context: the deferred count sits at defer[n], so its address moves with n
    and the buffers are reused. Each repeat is bit-equal to its first result,
    and B alone in a fresh process gives the same doubles."""
    from hddm_amd import cdfdif_wrapper as cw
    xa, xc = _seq_x(50000, SEQ_ROWS[0], 15), _seq_x(50001, SEQ_ROWS[2], 16)
    xb = np.array(SEQ_B)
    a1 = cw.dmat_cdf_array(xa, *SEQ_ROWS[0])
    b1 = cw.dmat_cdf_array(xb, *SEQ_ROWS[1])
    c1 = cw.dmat_cdf_array(xc, *SEQ_ROWS[2])
    a2 = cw.dmat_cdf_array(xa, *SEQ_ROWS[0])
    b2 = cw.dmat_cdf_array(xb, *SEQ_ROWS[1])
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
    assert np.array_equal(c1, cw.dmat_cdf_array(xc, *SEQ_ROWS[2]))
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(SEQ_B),
                        json.dumps(SEQ_ROWS[1])], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    fresh = np.array([float.fromhex(h) for h in json.loads(r.stdout.strip().splitlines()[-1])])
    assert np.array_equal(fresh, b1), (fresh, b1)
    for name, x, got, p in (("sequence A", xa, a1, SEQ_ROWS[0]), ("sequence C", xc, c1,
                                                                  SEQ_ROWS[2])):
        pick = np.arange(0, x.size, x.size // 256)[:260]
        _sample_against(name, np.ascontiguousarray(x[pick]), got[pick], p)
    import oracle
    assert np.abs(b1 - oracle.dmat_cdf_array(xb, *SEQ_ROWS[1])).max() <= CDF_ATOL
