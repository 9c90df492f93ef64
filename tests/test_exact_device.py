"""The exact path and its correctly rounded libm on the device.

tests/test_crlibm.py and tests/test_exact_path.py check hddm_amd/csrc/
wfpt_crlibm.hpp and wfpt_exact.hpp as gcc compiles them. The kernels run what
hipcc makes of the same source for gfx950, where frexp / ldexp, rint, the
double-to-int conversions, the seed log(m) of log_mant_dd, sqrt and / are
other instructions. Here the device build is held to the host build bit for
bit (int64 views, NaN equal to NaN), through
  * a probe library (tests/c/exact_device.hip, built by hddm_amd.build.
    build_probe with the library's flags): each cr_* function, sqrt and /
    one element per lane, and wfpt_x::full_pdf per trial with its evaluation
    count (equal counts: the same tree);
  * the product: the trials its kernels route to the exact path (densities
    at or below kExactBelow, near-tie stop tests, guard-band series
    decisions) must return the host build's double, and regression links
    must return the correctly rounded exp.
The host builds are compiled here with g++ (tests/c/exact_host.cpp). sqrt and
/ are also checked against exact integer / rational references that use no
libm. Every parameter set goes through the host build first and reaches the
device only if the host reports no depth or budget overflow.
"""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_crlibm import CASES, exact as exact_value
from test_lean_uniform import _open_ctx
from test_parity_strict import _flip, _nudges, _root_S
from test_reg import FAMILIES, reg_args, reg_kw, restate_pred

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "exact_host.cpp")

_D, _I, _I64 = ctypes.c_double, ctypes.c_int, ctypes.c_int64
_PD = ctypes.POINTER(ctypes.c_double)
_PI64 = ctypes.POINTER(ctypes.c_int64)
_PI32 = ctypes.POINTER(ctypes.c_int32)
_PDF_ARGS = [_PD, _I64] + [_D] * 8 + [_I, _I, _I, _D, _PD, _PI64, _PI32]

# the near-t sets of tests/test_exact_path.py::test_exact_path_subnormal_and_zero_densities
T0 = 0.3
NEAR_T = [(0.5, 0.0, 2.0, 0.5, 0.0, T0, 0.0), (0.5, 1.0, 2.0, 0.5, 0.0, T0, 0.0),
          (-1.0, 0.5, 2.0, 0.45, 0.2, T0, 0.0), (0.5, 0.0, 2.0, 0.5, 0.0, T0 + 0.001, 0.002),
          (0.5, 0.3, 2.0, 0.5, 0.1, T0 + 0.001, 0.002)]
KN = (1e-4, 2, 2, 1, 1e-3)  # err, n_st, n_sz, use_adaptive, simps_err (HDDM's)
ROUTED_BELOW = 5e-291  # inside kExactBelow = 1e-290 with a margin for the fast path's error
DEEP = 2.0 ** -1044    # one quantum below it moves the log by >= 2^-30 = 9.3e-10
LOG_BAR = 1e-11


def _pd(a):
    return a.ctypes.data_as(_PD)


class _Pdf:
    """full_pdf per trial through one C entry: (out, ne, ovf)."""

    def __init__(self, entry, returns_status):
        entry.argtypes = _PDF_ARGS
        entry.restype = _I if returns_status else None
        self.entry, self.returns_status = entry, returns_status

    def __call__(self, x, v, sv, a, z, sz, t, st, err, n_st=2, n_sz=2, ua=1, se=1e-3):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        ne = np.empty(x.size, dtype=np.int64)
        ovf = np.empty(x.size, dtype=np.int32)
        rc = self.entry(_pd(x), x.size, v, sv, a, z, sz, t, st, err, int(n_st), int(n_sz), int(ua),
                        se, _pd(out), ne.ctypes.data_as(_PI64), ovf.ctypes.data_as(_PI32))
        if self.returns_status:
            assert rc == 0, f"probe_exact_pdf: HIP error {rc}"
        return out, ne, ovf


class Host:
    """The g++ build of the two headers (tests/c/exact_host.cpp)."""

    def __init__(self, so):
        L = ctypes.CDLL(so)
        L.cr_fn_array.restype = None
        L.cr_fn_array.argtypes = [_I, _PD, _I64, _PD]
        self.L = L
        self.pdf = _Pdf(L.exact_pdf_array_ex, False)

    def fn(self, fn, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        self.L.cr_fn_array(fn, _pd(x), x.size, _pd(out))
        return out

    def pdf1(self, x, *args):
        return float(self.pdf(np.array([x], dtype=np.float64), *args)[0][0])


class Probe:
    """The gfx950 build (hddm_amd/lib/libwfpt_exact_probe.so)."""

    def __init__(self, so):
        L = ctypes.CDLL(so)
        L.probe_fn.restype = _I
        L.probe_fn.argtypes = [_I, _PD, _PD, _I64, _PD]
        self.L = L
        self.pdf = _Pdf(L.probe_exact_pdf, True)

    def fn(self, fn, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size <= 2_000_000
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64)
            assert y.shape == x.shape
        out = np.empty_like(x)
        rc = self.L.probe_fn(fn, _pd(x), _pd(y) if y is not None else None, x.size, _pd(out))
        assert rc == 0, f"probe_fn({fn}): HIP error {rc}"
        return out


def build_host(so, src=SRC):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                    "-shared", "-o", so, src, "-lm"], check=True)
    return Host(so)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("exact_device") / "libexact_host.so"))


@pytest.fixture(scope="module")
def probe(gpu):
    from hddm_amd import build
    assert os.path.exists(build.PROBE), "the exact-path probe is not built (hddm_amd.build.build_probe)"
    return Probe(build.PROBE)


@pytest.fixture(scope="module")
def lean_ctx(gpu):
    """Resident calls always take the lean level-0 pass (tests/test_lean_uniform.py)."""
    ctx = _open_ctx({"WFPT_LEAN_TREE": "1.0"})
    yield ctx
    ctx.close()


def same_bits(a, b):
    """Elementwise: the same double (NaN equal to NaN, -0.0 unequal to 0.0)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def hexes(*vals):
    return tuple(float(v).hex() for v in vals)


# --------------------------------------------------------------------------- (a) libm

def libm_disagreements(fn, x, dev, hst):
    """Indices where two builds differ, and for the first of them which build
    is misrounded (against decimal / fraction arithmetic rounded once)."""
    bad = np.flatnonzero(~same_bits(dev, hst))
    report = []
    for i in bad[:10]:
        e = exact_value(fn, x[i])
        who = [w for w, val in (("device", dev[i]), ("host", hst[i])) if val != e]
        report.append((hexes(x[i], dev[i], hst[i], e), "misrounded: " + "+".join(who)))
    return bad, report


@pytest.mark.gpu
@pytest.mark.parametrize("fn,name,gen", CASES, ids=[c[1] for c in CASES])
def test_libm_device_equals_host(host, probe, fn, name, gen):
    """cr_exp / cr_log / cr_sin / cr_cube: the gfx950 build returns the g++
    build's double on every input of test_crlibm.py's generators."""
    x = gen(np.random.default_rng(300 + fn), 200_000)
    assert fn != 2 or np.all(np.abs(x) < 2.0 ** 20)  # cr_sin's own range
    dev, hst = probe.fn(fn, x), host.fn(fn, x)
    bad, report = libm_disagreements(fn, x, dev, hst)
    print(f"cr_{name}: {bad.size} device/host disagreements in {x.size}")
    assert bad.size == 0, (name, bad.size, report)


@pytest.mark.gpu
@pytest.mark.parametrize("fn,name,gen", CASES, ids=[c[1] for c in CASES])
def test_libm_device_correctly_rounded(probe, fn, name, gen):
    """Independently of the host build: the device's value is the exact value
    rounded once."""
    x = gen(np.random.default_rng(100 + fn), 1500)
    dev = probe.fn(fn, x)
    bad = [hexes(xi, d, exact_value(fn, xi)) for xi, d in zip(x, dev) if d != exact_value(fn, xi)]
    assert not bad, f"{name}: {len(bad)} of {x.size} misrounded on the device, e.g. {bad[:3]}"


def libm_edges(fn):
    """Inputs at the places where the two builds run other instructions: the
    generators above rarely or never reach them. Subnormal arguments and
    results (frexp / ldexp), arguments whose reduction quotient is a tie or an
    integer (rint), the overflow and underflow thresholds, signed zeros,
    infinities, NaN, negative arguments."""
    rng = np.random.default_rng(500 + fn)
    tiny, big, eps = np.finfo(float).tiny, np.finfo(float).max, np.finfo(float).eps
    sub = random_doubles(rng, 4000, False)
    sub = sub[sub < tiny][:64]
    common = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 1e-320, tiny, tiny * (1 - eps), big, 1.0,
              1.0 - eps / 2, 1.0 + eps, -1.0, -tiny, -5e-324]
    if fn == 0:
        k = np.arange(-1080, 1030, dtype=np.float64)
        own = np.concatenate([k * math.log(2.0), (k + 0.5) * math.log(2.0),
                              np.nextafter((k + 0.5) * math.log(2.0), np.inf),
                              np.linspace(709.75, 709.80, 101), np.linspace(-746.5, -744.0, 251),
                              np.linspace(-708.5, -708.3, 101), sub, -sub])
    elif fn == 1:
        own = np.concatenate([sub, 2.0 ** np.arange(-1074, 1024, 7.0),
                              np.nextafter(2.0 ** np.arange(-1070, 1020, 11.0), 0.0),
                              math.sqrt(0.5) * (1 + eps * np.arange(-8, 9)),
                              math.sqrt(2.0) * (1 + eps * np.arange(-8, 9)),
                              1.0 + 2.0 ** -5 * (1 + eps * np.arange(-8, 9)),
                              1.0 - 2.0 ** -5 * (1 + eps * np.arange(-8, 9)),
                              1.0 + eps * np.arange(-40, 41)])
    elif fn == 2:
        k = np.concatenate([np.arange(0, 600.0), rng.integers(600, 660_000, 400).astype(float)])
        h = k * (np.pi / 2)
        own = np.concatenate([h, np.nextafter(h, np.inf), np.nextafter(h, 0.0), -h[:200],
                              (k + 0.5) * (np.pi / 2), sub, [np.nextafter(2.0 ** 20, 0.0), 1e-300]])
        common = [c for c in common if not abs(c) >= 2.0 ** 20]  # beyond: the platform's sin
    else:
        own = np.concatenate([sub, -sub, 10.0 ** rng.uniform(-108.5, -102.0, 300),
                              -(10.0 ** rng.uniform(-108.5, -102.0, 100)),
                              2.0 ** np.arange(-1074, 1024, 5.0), rng.uniform(-3, 0, 200),
                              np.cbrt(big) * (1 + eps * np.arange(-8, 9)),
                              np.cbrt(5e-324) * np.linspace(0.5, 1.5, 101)])
    return np.concatenate([np.array(common), own])


@pytest.mark.gpu
@pytest.mark.parametrize("fn,name,gen", CASES, ids=[c[1] for c in CASES])
def test_libm_edges_device_equals_host(host, probe, fn, name, gen):
    """The same at the edges (libm_edges), and where the exact value is defined
    (finite arguments inside the function's domain) both builds equal it."""
    x = libm_edges(fn)
    assert fn != 2 or np.all(np.abs(x[~np.isnan(x)]) < 2.0 ** 20)
    dev, hst = probe.fn(fn, x), host.fn(fn, x)
    bad = np.flatnonzero(~same_bits(dev, hst))
    assert bad.size == 0, (name, bad.size, [hexes(x[i], dev[i], hst[i]) for i in bad[:10]])
    # test_crlibm.exact's own limits: decimal's exponent range for exp, a
    # series cut at 1e-80 for sin; a cube beyond the largest double is inf
    dom = np.isfinite(x) & {0: np.abs(x) < 1000, 1: x > 0, 2: np.abs(x) > 1e-60, 3: True}[fn]
    idx = np.flatnonzero(dom)
    idx = idx[:: max(1, idx.size // 700)]

    def value(xi):
        try:
            return exact_value(fn, xi)
        except OverflowError:
            return math.copysign(math.inf, xi)
    wrong = [hexes(x[i], dev[i], value(x[i])) for i in idx if dev[i] != value(x[i])]
    assert not wrong, f"{name}: {len(wrong)} of {idx.size} edge inputs misrounded, e.g. {wrong[:3]}"


# --------------------------------------------------------------------------- (b) sqrt and /

def random_doubles(rng, n, signed):
    """Uniform exponent field 0..2046 (subnormals to the largest binade, both
    parities) and uniform fraction bits."""
    b = (rng.integers(0, 2047, n, dtype=np.uint64) << np.uint64(52)) | rng.integers(
        0, 1 << 52, n, dtype=np.uint64)
    if signed:
        b |= rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)
    return b.view(np.float64)


def sqrt_exact(d):
    """The double nearest to sqrt(d), d a positive finite double, by integer
    arithmetic alone (math.isqrt; the remainder decides the rounding)."""
    mant, ex = math.frexp(d)
    M, E = int(mant * 9007199254740992.0), ex - 53  # d = M 2^E exactly
    if E & 1:
        M, E = M << 1, E - 1
    k = max(0, (114 - M.bit_length()) // 2)  # the root gets >= 56 bits
    M, E = M << (2 * k), E - 2 * k
    r = math.isqrt(M)
    rem = M - r * r
    shift = r.bit_length() - 53
    q, low, half = r >> shift, r & ((1 << shift) - 1), 1 << (shift - 1)
    if low > half or (low == half and (rem > 0 or (q & 1))):
        q += 1
    return math.ldexp(float(q), shift + E // 2)  # sqrt of a double is never subnormal


def test_sqrt_exact_reference():
    """The integer reference itself, where the answer is known."""
    assert sqrt_exact(4.0) == 2.0 and sqrt_exact(2.0) == math.sqrt(2.0)
    assert sqrt_exact(5e-324) == math.ldexp(1.0, -537)
    m = (1 << 53) - 1
    assert sqrt_exact(float(m) * float(m)) == math.sqrt(float(m) * float(m))
    # 4 m (m + 1) lies just below (2 m + 1)^2, a midpoint of two doubles: down
    m = (1 << 52) + 12345
    assert sqrt_exact(float(4 * m * (m + 1))) in (float(2 * m), float(2 * m + 2))
    rng = np.random.default_rng(5)
    for d in random_doubles(rng, 2000, False):
        if d > 0:
            r = sqrt_exact(float(d))
            lo, hi = Fraction(np.nextafter(r, 0.0)), Fraction(np.nextafter(r, np.inf))
            fr = Fraction(r)
            # r is nearest: ((lo + r) / 2)^2 <= d <= ((r + hi) / 2)^2
            assert ((lo + fr) / 2) ** 2 <= Fraction(float(d)) <= ((fr + hi) / 2) ** 2, d


def hard_sqrt_inputs(rng, n):
    """For n random 53-bit integers m: the doubles nearest to m^2, m (m + 1)
    and (m + 1/2)^2 (as 4 m^2, 4 m (m + 1), (2 m + 1)^2: roots at or next to a
    double or a midpoint of two doubles) and their two neighbours, each scaled
    by an even and by an odd power of two (some into the subnormal range)."""
    out = []
    ms = rng.integers(1 << 52, 1 << 53, n)
    se = 2 * rng.integers(-590, 455, n)
    so = 2 * rng.integers(-590, 455, n) + 1
    for m, s_even, s_odd in zip(ms.tolist(), se.tolist(), so.tolist()):
        for N in (4 * m * m, 4 * m * (m + 1), (2 * m + 1) ** 2):
            d0 = float(N)
            for d in (math.nextafter(d0, 0.0), d0, math.nextafter(d0, math.inf)):
                out.append(math.ldexp(d, s_even))
                out.append(math.ldexp(d, s_odd))
    return np.array(out)


def hard_div_pairs(rng, n):
    """Pairs (x, y) with x = fl(q y) and its two neighbours: q a 53-bit value
    (the quotient sits next to a double) or a 54-bit odd one (next to a
    midpoint of two doubles). A quarter of the quotients are subnormal."""
    xs, ys = [], []
    Y = rng.integers(1 << 52, 1 << 53, n).tolist()
    Q = rng.integers(1 << 52, 1 << 53, n).tolist()
    tq = np.where(np.arange(n) % 4 == 3, rng.integers(-1073, -1021, n),
                  rng.integers(-1000, 1000, n)).tolist()
    u = rng.random(n).tolist()
    for i in range(n):
        q = Q[i] if i % 2 == 0 else 2 * Q[i] + 1
        # x / y = q 2^(ex - ey) near 2^tq; x ~ 2^(106 + ex) and y ~ 2^(53 + ey) stay normal
        d = tq[i] - q.bit_length()
        lo, hi = max(-1000, -1120 - d), min(900, 910 - d)
        ey = lo + int(u[i] * (hi - lo))
        ex = ey + d
        x0 = float(q * Y[i])
        for xv in (math.nextafter(x0, 0.0), x0, math.nextafter(x0, math.inf)):
            xs.append(math.ldexp(xv, ex))
            ys.append(math.ldexp(float(Y[i]), ey))
    return np.array(xs), np.array(ys)


@pytest.mark.gpu
def test_sqrt_on_device(probe):
    """The plain sqrt of wfpt_exact.hpp as compiled for gfx950 (the term counts
    kl and ks are ceil of a sqrt): correctly rounded on 2,000,000 random
    doubles (against the host's) and on 360,000 hard cases (against isqrt)."""
    rng = np.random.default_rng(41)
    x = random_doubles(rng, 2_000_000, False)
    bad = np.flatnonzero(~same_bits(probe.fn(4, x), np.sqrt(x)))
    print(f"sqrt random: {bad.size} mismatches in {x.size}")
    assert bad.size == 0, (bad.size, [hexes(x[i], np.sqrt(x[i])) for i in bad[:5]])
    h = hard_sqrt_inputs(rng, 20_000)
    assert h.size == 360_000 and np.all(h > 0) and np.all(np.isfinite(h))
    want = np.array([sqrt_exact(d) for d in h.tolist()])
    got = probe.fn(4, h)
    bad = np.flatnonzero(~same_bits(got, want))
    print(f"sqrt hard cases: {bad.size} mismatches in {h.size}")
    assert bad.size == 0, (bad.size, [hexes(h[i], got[i], want[i]) for i in bad[:5]])


@pytest.mark.gpu
def test_division_on_device(probe):
    """The plain / of wfpt_exact.hpp as compiled for gfx950: correctly rounded
    on 2,000,000 random pairs (half of them with finite, partly subnormal
    quotients) and on 60,000 hard pairs against exact rationals."""
    rng = np.random.default_rng(43)
    n = 2_000_000
    x = random_doubles(rng, n, True)
    y = random_doubles(rng, n, True)
    # second half: the quotient's exponent uniform over the finite range
    ex = (x[n // 2:].view(np.uint64) >> np.uint64(52)) & np.uint64(2047)
    ey = np.clip(ex.astype(np.int64) - rng.integers(-1080, 1031, n - n // 2), 1, 2046)
    yb = y[n // 2:].view(np.uint64)
    yb &= ~(np.uint64(2047) << np.uint64(52))
    yb |= ey.astype(np.uint64) << np.uint64(52)
    with np.errstate(all="ignore"):
        want = x / y
    assert np.sum(np.isfinite(want) & (want != 0)) > n // 2
    assert np.sum((np.abs(want) < np.finfo(float).tiny) & (want != 0)) > 10_000
    got = probe.fn(5, x, y)
    bad = np.flatnonzero(~same_bits(got, want))
    print(f"division random: {bad.size} mismatches in {n}")
    assert bad.size == 0, (bad.size, [hexes(x[i], y[i], got[i], want[i]) for i in bad[:5]])
    hx, hy = hard_div_pairs(rng, 20_000)
    want = np.array([float(Fraction(a) / Fraction(b)) for a, b in zip(hx.tolist(), hy.tolist())])
    assert np.all(np.isfinite(want)) and np.all(want > 0)
    assert np.sum(want < np.finfo(float).tiny) > 10_000
    got = probe.fn(5, hx, hy)
    bad = np.flatnonzero(~same_bits(got, want))
    print(f"division hard cases: {bad.size} mismatches in {hx.size}")
    assert bad.size == 0, (bad.size, [hexes(hx[i], hy[i], got[i], want[i]) for i in bad[:5]])


# --------------------------------------------------------------------------- (c) full_pdf

def golden_sets():
    g = np.load(os.path.join(ROOT, "tests", "golden", "full_pdf_grid.npz"), allow_pickle=False)
    for r, x in zip(g["params"], g["x"]):
        yield x, tuple(float(q) for q in r[:8]) + (int(r[8]), int(r[9]), int(r[10]), float(r[11]))


def near_t_x():
    xx = np.concatenate([np.linspace(2e-4, 2e-3, 400), np.geomspace(1e-5, 2e-4, 100)])
    return np.concatenate([T0 + xx, -(T0 + xx)])


def near_t_sets():
    for p in NEAR_T:
        yield near_t_x(), p + (1e-4, 2, 2, 1, 1e-3)


def random_family_sets():
    """The 40 sets of tests/test_exact_path.py::test_exact_path_random_families."""
    rng = np.random.default_rng(31)
    for _ in range(40):
        p = (rng.uniform(-4, 4), rng.choice([0.0, rng.uniform(0, 2.5)]), rng.uniform(0.5, 2),
             rng.uniform(0.4, 0.6), rng.choice([0.0, rng.uniform(0, 0.4)]),
             rng.uniform(0.2, 0.5), rng.choice([0.0, rng.uniform(0, 0.35)]))
        err = 10 ** rng.uniform(-10, -1)
        n = int(rng.choice([2, 4, 6]))
        se = 10 ** rng.uniform(-6, -2)
        x = rng.choice([-1.0, 1.0], 64) * (p[5] - p[6] / 2 + rng.gamma(1.5, 0.5, 64))
        yield x, tuple(float(q) for q in p) + (err, n, n, 1, se)


FAMILY_SETS = {"golden": (golden_sets, 168), "near_t": (near_t_sets, 5),
               "random": (random_family_sets, 40)}


def compare_full_pdf(host, device_pdf, sets):
    """Host first; the device only where the host reports no overflow.
    Returns (sets compared, trials compared, sets skipped)."""
    n_sets = n_trials = skipped = 0
    for x, args in sets:
        assert args[7] >= 1e-10 and args[11] >= 2.7e-8, args  # bounded series and trees
        want, ne, ovf = host.pdf(x, *args)
        if np.any(ovf != 0):
            skipped += 1
            continue
        got, ne_d, ovf_d = device_pdf(x, *args)
        bad = np.flatnonzero(~same_bits(got, want))
        assert bad.size == 0, (args, bad.size,
                               [hexes(x[i], got[i], want[i]) for i in bad[:5]])
        assert np.array_equal(ne_d, ne), (args, np.flatnonzero(ne_d != ne)[:5])
        assert np.array_equal(ovf_d, ovf), args
        n_sets += 1
        n_trials += x.size
    return n_sets, n_trials, skipped


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILY_SETS))
def test_full_pdf_device_equals_host(host, probe, family):
    """wfpt_x::full_pdf per trial: the same double, the same number of pdf_sv
    evaluations (the same tree) and the same overflow flags from both builds
    of one header. No exception rate: the 1% allowance of test_exact_path.py
    is glibc's, and glibc is not involved here."""
    sets, count = FAMILY_SETS[family]
    n_sets, n_trials, skipped = compare_full_pdf(host, probe.pdf, sets())
    print(f"{family}: {n_sets} sets, {n_trials} trials compared, {skipped} sets skipped (host ovf)")
    assert n_sets + skipped == count
    assert n_trials <= 100_000
    # from the host build alone: none of these sets overflows its depth or budget
    assert skipped == 0


# --------------------------------------------------------------------------- (d) routed trials

def _crossing(host, p, sign, above):
    """The smallest distance |x| - (t - st/2), to bisection accuracy, at which
    the host build's density exceeds `above`."""
    base = p[5] - p[6] / 2

    def f(d):
        return host.pdf1(sign * (base + d), *p, *KN)
    lo, hi = 0.0, 2e-3
    assert not f(lo) > above and f(hi) > above
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if f(mid) > above:
            hi = mid
        else:
            lo = mid
    return hi


@pytest.fixture(scope="module")
def ramps(host):
    """Per near-t set: 2 x 2,200 RTs (both boundaries): 2,000 evenly between
    the distance at which the density leaves 0 and the one at which it crosses
    5e-291, and 200 below (exact zeros); with the host build's densities."""
    out = []
    tiny = np.finfo(float).tiny
    for p in NEAR_T:
        base = p[5] - p[6] / 2
        xs = []
        for sign in (1.0, -1.0):
            d0, d1 = _crossing(host, p, sign, 0.0), _crossing(host, p, sign, ROUTED_BELOW)
            assert 0 < d0 < d1
            dist = np.concatenate([np.linspace(d0, d1, 2000), np.linspace(0, d0, 200, endpoint=False)])
            x = sign * (base + dist)
            want = host.pdf(x, *p, *KN)[0]
            pos = (want > 0) & (want <= ROUTED_BELOW)
            # the test cannot become vacuous
            assert pos[:2000].sum() >= 1900 and (pos & (want < tiny)).sum() >= 600, (p, sign)
            assert np.all(want[2000:] == 0) and np.all(want[:2000] <= 1e-290), (p, sign)
            xs.append(x)
        x = np.concatenate(xs)
        want, _, ovf = host.pdf(x, *p, *KN)
        assert not np.any(ovf)
        out.append((p, x, want))
    return out


@pytest.mark.gpu
def test_routed_densities_equal_host(gpu, ramps):
    """pdf_array (densities, no mixture) on trials at or below 5e-291 and on
    exact zeros: each is recomputed on the device's exact path and must be the
    host build's double, subnormal ones to the quantum."""
    for p, x, want in ramps:
        got = gpu.pdf_array(x, *p, 1e-4, 0, 2, 2, 1, 1e-3, 0, 0)
        bad = np.flatnonzero(~same_bits(got, want))
        print(f"pdf_array {p}: {bad.size} of {x.size} differ")
        assert bad.size == 0, (p, bad.size, [hexes(x[i], got[i], want[i]) for i in bad[:5]])


def check_terms(terms, want, what):
    """Log terms of routed trials: -inf where the host density is 0, within
    1e-11 of math.log of the host density where that is below 2^-1044 (one
    quantum moves the log by >= 9.3e-10 there; the log's own rounding is
    ~1e-13). Returns the number of trials below 2^-1044."""
    terms = np.asarray(terms)
    zero = want == 0
    assert np.all(np.isneginf(terms[zero])), (what, np.flatnonzero(zero & ~np.isneginf(terms))[:5])
    deep = np.flatnonzero((want > 0) & (want < DEEP))
    ref = np.array([math.log(w) for w in want[deep].tolist()])
    d = np.abs(terms[deep] - ref)
    assert d.size and np.all(np.isfinite(terms[deep])) and d.max() < LOG_BAR, (
        what, float(np.nanmax(d)), deep[np.nanargmax(d)])
    return deep.size


def _site_trials(gpu, ctx, ramp):
    p, x, want = ramp
    ds = gpu.Dataset(x, ctx=ctx)
    counts, paths = [], []
    for call in range(2):  # the full sequence, then the predicted one
        _, terms = ds.wiener_like_trials(*p, *KN, 0, 0)
        counts.append(check_terms(terms, want, ("trials", p, call)))
        paths.append(ds.ctx.last_path())
    ds.close()
    return counts[0], paths


def _site_small(gpu, ramp):
    """Datasets of <= 256 trials. The one-launch small kernel runs when the
    dataset's last call deferred no trial, and it leaves every routed trial to
    the deferred pass: so each dataset is first scored with t = 0.05 (ordinary
    densities, nothing deferred), then with the ramp's own t (small kernel,
    mispredicted, then the deferred pass), then once more (the full sequence)."""
    from hddm_amd import _lib
    p, x, want = ramp
    sel = np.flatnonzero((want < DEEP))  # the deep trials and the zeros
    count, paths = 0, []
    for lo in range(0, sel.size, 256):
        idx = sel[lo:lo + 256]
        ds = gpu.Dataset(x[idx])
        _, warm = ds.wiener_like_trials(*p[:5], 0.05, p[6], *KN, 0, 0)
        assert np.all(np.isfinite(warm)), (p, lo)
        for call in range(2):
            _, terms = ds.wiener_like_trials(*p, *KN, 0, 0)
            if np.any(want[idx] > 0):
                c = check_terms(terms, want[idx], ("small", p, lo, call))
            else:
                assert np.all(np.isneginf(terms))
                c = 0
            paths.append(_lib.context().last_path())
        count += c
        ds.close()
    return count, paths


def _site_multi(gpu, ramp):
    p, x, want = ramp
    v = np.full(x.size, p[0])
    _, terms = gpu.wiener_like_multi_terms(x, v, *p[1:], 1e-4, ["v"], 2, 2, 1, 1e-3, 0, 0)
    return check_terms(terms, want, ("multi", p)), []


@pytest.mark.gpu
@pytest.mark.parametrize("site", ["trials", "trials_lean", "trials_small", "multi_terms"])
def test_routed_log_terms(gpu, ramps, lean_ctx, site):
    """The same ramps through the other kernels that settle a trial on the
    exact path and return log terms (p_outlier = 0: no mixture absorbs the
    density)."""
    from hddm_amd import _lib
    seen = 0
    for ramp in ramps:
        if site == "trials":
            n, paths = _site_trials(gpu, _lib.context(), ramp)
        elif site == "trials_lean":
            n, paths = _site_trials(gpu, lean_ctx, ramp)
        elif site == "trials_small":
            n, paths = _site_small(gpu, ramp)
        else:
            n, paths = _site_multi(gpu, ramp)
        for q in paths:
            seen |= q
        print(f"{site} {ramp[0]}: {n} trials below 2^-1044, paths {sorted(set(paths))}")
        assert n >= 200, (site, ramp[0], n)
        if site == "trials_small":
            assert any(q & _lib.PATH_SMALL for q in paths), (ramp[0], paths)
    if site == "trials_lean":
        assert seen & _lib.PATH_LEAN, seen


@pytest.mark.gpu
def test_routed_log_terms_nodes(gpu, ramps):
    """wiener_like_nodes(trials=True) with the five sets as nodes."""
    x = np.concatenate([r[1] for r in ramps])
    node = np.repeat(np.arange(len(ramps), dtype=np.int32), [r[1].size for r in ramps])
    params = np.array([r[0] + (0.0,) for r in ramps])
    ds = gpu.Dataset(x, node_id=node, n_nodes=len(ramps))
    for call in range(2):
        _, terms = ds.wiener_like_nodes(params, *KN, 0.0, trials=True)
        for k, (p, _, want) in enumerate(ramps):
            n = check_terms(terms[node == k], want, ("nodes", p, call))
            print(f"nodes {p}: {n} trials below 2^-1044")
            assert n >= 200, (p, n)
    ds.close()


# --------------------------------------------------------------------------- (e) near-ties

def near_tie_cases(oracle_lib, mode):
    """The construction of tests/test_parity_strict.py::test_near_tie_stop_test."""
    rng = np.random.default_rng(21)
    for _ in range(12):
        v, sv, a = rng.uniform(-2, 2), rng.uniform(0, 1.5), rng.uniform(0.8, 2.0)
        z, t = rng.uniform(0.4, 0.6), rng.uniform(0.25, 0.4)
        sz, st = (0.0, rng.uniform(0.1, 0.3)) if mode == "t" else (rng.uniform(0.1, 0.3), 0.0)
        x = rng.choice([-1.0, 1.0]) * (t + st / 2 + rng.uniform(0.05, 0.6))
        xa, vv, zz = _flip(x, v, z)
        err = 1e-4
        if mode == "t":
            lb, ub = t - st / 2., t + st / 2.
            ZT = ub - lb
            c = (ub + lb) / 2.
            pts = [lb, (lb + c) / 2., c, (c + ub) / 2., ub]
            f = [oracle_lib.pdf_sv(xa - q, vv, sv, a, zz, err) / ZT for q in pts]
        else:
            lb, ub = zz - sz / 2., zz + sz / 2.
            ZT = ub - lb
            c = (ub + lb) / 2.
            pts = [lb, (lb + c) / 2., c, (c + ub) / 2., ub]
            f = [oracle_lib.pdf_sv(xa - t, vv, sv, a, q, err) / ZT for q in pts]
        S, S2 = _root_S(f, lb, ub)
        if not abs(S2 - S) > 0:
            continue
        for se in _nudges(abs(S2 - S) / 15):
            yield float(x), (v, sv, a, z, sz, t, st, err, 2, 2, 1, float(se))


def guard_band_cases():
    """The construction of test_parity_strict.py::test_series_decision_guard_band."""
    for tt in (0.2, 0.3, 0.45):
        for K in (1, 2):
            err0 = math.exp(-(K * K) * math.pi ** 2 * tt / 2) / (math.pi * tt)
            for err in _nudges(err0, 6):
                a, t = 1.0, 0.3
                for w in (0.3, 0.5, 0.7):
                    yield -(t + tt * a * a), (0.4, 0.0, a, w, 0.0, t, 0.0, float(err), 2, 2, 1, 1e-3)


def assert_full_pdf_bits(gpu, host, cases, at_least):
    checked, bad = 0, []
    for x, args in cases:
        want, _, ovf = host.pdf(np.array([x]), *args)
        if ovf[0]:
            continue
        got = gpu.full_pdf(x, *args)
        if not same_bits(np.array([got]), want)[0]:
            bad.append((x, args, hexes(got, want[0])))
        checked += 1
    assert checked >= at_least, checked
    assert not bad, (len(bad), checked, bad[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["t", "z"])
def test_near_tie_bits(gpu, host, oracle_lib, mode):
    """Stop tests within 0-4 ulps of their threshold (normal-range densities):
    the kernels route the trial to the exact path, so full_pdf is the host
    build's double. An unrouted trial, or a device exact path one ulp off,
    fails here; the 1e-12 bar of test_parity_strict.py does not see either."""
    assert_full_pdf_bits(gpu, host, near_tie_cases(oracle_lib, mode), 60)


@pytest.mark.gpu
def test_guard_band_bits(gpu, host):
    """Series term counts within a few ulps of an integer: the same."""
    assert_full_pdf_bits(gpu, host, guard_band_cases(), 3 * 2 * 13 * 3)


# --------------------------------------------------------------------------- (f) cr_exp, product

@pytest.mark.gpu
@pytest.mark.parametrize("link", ["exp", "invlogit"])
def test_reg_links_over_the_whole_exp_range(gpu, link):
    """The regression kernel's cr_exp (reg_kernels.hip) over exp's whole finite
    range, subnormal results and overflow included: the predictions of a
    one-column design with coefficient 1.0 are the correctly rounded links.
    (The drift these predictions feed is mostly absurd; only the predictions
    are read.)"""
    rng = np.random.default_rng(47)
    eta = np.concatenate([rng.uniform(-745.2, 709.7, 3072), rng.uniform(-1, 1, 1022),
                          [-745.2, 709.7]])
    assert eta.size == 4096
    X = np.ascontiguousarray(eta[:, None])
    rt = rng.choice([-1.0, 1.0], eta.size) * (0.15 + rng.gamma(2.0, 0.25, eta.size))
    F = FAMILIES["simple"]
    ds = gpu.RegDataset(rt, X)
    _, _, pred = ds.wiener_like_reg([("v", 0, 1, link)], [1.0], *reg_args(F, a=1.8, t=0.1),
                                    **reg_kw(F), terms=True)
    ds.close()
    want = restate_pred(X, [1.0], 0, 1, link)
    bad = np.flatnonzero(~same_bits(pred["v"], want))
    assert bad.size == 0, (link, bad.size, [hexes(eta[i], pred["v"][i], want[i]) for i in bad[:5]])
