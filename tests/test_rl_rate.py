"""The learning rate of a regressed alpha (rl_update.hpp: rl_rate over
wfpt_crlibm.hpp: cr_pow_rlbase), host build, no GPU.

cr_pow_rlbase(x) is B**x rounded once, B the double nearest the reference's
literal 2.718281828459 (wfpt.pyx:123, :317). It is checked here against
`decimal` at 80 digits, rounded once to double, on every argument: equality,
not a tolerance. Against glibc's pow (the route the non-regressed learning
rates keep) no value may differ by more than one ulp; the shares of differing
powers and rates are printed (DESIGN.md §25 records them) and not asserted.
"""
import ctypes
import math
import os
import subprocess
from decimal import Decimal, getcontext

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PD = ctypes.POINTER(ctypes.c_double)
RL_BASE = 2.718281828459


def build_rate_host(so):
    """The g++ build of tests/c/rl_rate_host.cpp: {name: array function}."""
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                    "-shared", "-o", so, os.path.join(ROOT, "tests", "c", "rl_rate_host.cpp"),
                    "-lm"], check=True)
    L = ctypes.CDLL(so)

    def wrap(name):
        f = getattr(L, name)
        f.restype = None
        f.argtypes = [_PD, ctypes.c_int64, _PD]

        def call(x):
            x = np.ascontiguousarray(x, dtype=np.float64)
            out = np.empty_like(x)
            f(x.ctypes.data_as(_PD), x.size, out.ctypes.data_as(_PD))
            return out
        return call
    return {n: wrap(n + "_array") for n in ("cr_pow_rlbase", "rl_rate", "libm_pow_rlbase",
                                            "libm_rl_rate")}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_rate_host(str(tmp_path_factory.mktemp("rl_rate") / "librl_rate_host.so"))


def arguments():
    """40,000 seeded arguments over the ranges a learning rate's alpha meets and
    the whole finite range of the power, plus edge values."""
    rng = np.random.default_rng(20261021)
    ln_b = math.log(RL_BASE)
    over, under = math.log(sys_max()) / ln_b, (-1075 * math.log(2.0)) / ln_b
    edges = [0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1e-300, -1e-300, 2.0 ** -60, -2.0 ** -60,
             2.0 ** -53, -2.0 ** -53, 0.5, -0.5, 708.0, -708.0, -1022 * math.log(2.0) / ln_b]
    for c in (over, under):  # the thresholds and their neighbours
        edges += [c, np.nextafter(c, 0.0), np.nextafter(c, 2 * c), c - 1e-9, c + 1e-9,
                  c - 0.25, c + 0.25]
    return np.concatenate([rng.uniform(-12, 12, 20000), rng.normal(0, 3, 10000),
                           rng.uniform(-700, 700, 10000),
                           rng.uniform(-746, -708, 1000),  # subnormal results
                           np.array(edges, dtype=np.float64)])


def sys_max():
    return float(np.finfo(np.float64).max)


def exact_pow(x):
    """B**x by decimal at 80 digits, rounded once to the nearest double."""
    getcontext().prec = 80
    ln_b = Decimal(RL_BASE).ln()  # of the literal's double value, not of the decimal string
    out = np.empty(x.size)
    for i, v in enumerate(x.tolist()):
        out[i] = float((Decimal(v) * ln_b).exp())
    return out


def ulps_apart(a, b):
    """Distance in representable doubles between same-sign finite a and b."""
    ia = np.ascontiguousarray(a).view(np.int64)
    ib = np.ascontiguousarray(b).view(np.int64)
    return np.abs(ia - ib)


def test_cr_pow_rlbase_is_correctly_rounded(host):
    x = arguments()
    assert x.size >= 40000
    got = host["cr_pow_rlbase"](x)
    want = exact_pow(x)
    bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, [(float(x[i]).hex(), float(got[i]).hex(), float(want[i]).hex())
                           for i in bad[:5]]
    # the set reaches both ends of the range
    assert np.isinf(got).any() and (got == 0).any() and ((got > 0) & (got < 2.3e-308)).any()


def test_special_values(host):
    x = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, 1e308, -1e308])
    p = host["cr_pow_rlbase"](x)
    assert np.isnan(p[0]) and p[1] == np.inf and p[2] == 0.0 and p[3] == 1.0
    assert p[4] == RL_BASE and p[5] == np.inf and p[6] == 0.0
    r = host["rl_rate"](x)
    assert np.isnan(r[0]) and np.isnan(r[1])  # inf / inf, as in the reference
    assert r[2] == 0.0 and r[3] == 0.5 and np.isnan(r[5]) and r[6] == 0.0
    assert r[4] == RL_BASE / (1 + RL_BASE)


def test_rate_is_two_more_roundings(host):
    x = arguments()
    e = host["cr_pow_rlbase"](x)
    with np.errstate(invalid="ignore"):
        want = e / (1.0 + e)
    got = host["rl_rate"](x)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_against_libm(host):
    """glibc's pow is within one ulp of the correctly rounded power; the shares
    of differing powers and rates are reported, not asserted."""
    x = arguments()
    e, e_m = host["cr_pow_rlbase"](x), host["libm_pow_rlbase"](x)
    r, r_m = host["rl_rate"](x), host["libm_rl_rate"](x)
    fin = np.isfinite(e) & np.isfinite(e_m)
    assert np.array_equal(np.isfinite(e), np.isfinite(e_m))
    d = ulps_apart(e[fin], e_m[fin])
    nan = np.isnan(r)
    assert np.array_equal(nan, np.isnan(r_m))
    dr = ulps_apart(r[~nan], r_m[~nan])
    print(f"\nrl_rate vs libm over {x.size} arguments: powers differing {int((d > 0).sum())} "
          f"({(d > 0).mean():.3%}), max {int(d.max())} ulp; rates differing "
          f"{int((dr > 0).sum())} ({(dr > 0).mean():.3%}), max {int(dr.max())} ulp")
    assert d.max() <= 1
