"""Batched quantile objectives: cdfdif_wrapper.dmat_cdf_rows and hddm_amd.quantiles.

One launch scores R rows, each with its own parameters, E signed RT edges and
E + 1 observed bin counts (the chi-square / G-square objectives of
hddm/likelihoods.py:200-239). Checked here:

* cdf[r] is bit for bit dmat_cdf_array(x[r], *params[r]) on the same device,
  and within tests/test_cdfdif.py's bars of the oracle (1e-9 where sz and st
  are both >= 0.05, 1e-6 otherwise);
* chisq is bit for bit `_reduce` (the host restatement of the kernel's
  reduction loop) of the kernel's own cdf: both are IEEE operations in the same
  order;
* gsq is within 8 * 2^-52 * sum_k |2 f_k log p_k| of `_reduce`: the device's
  and NumPy's log are each within 1 ulp, so a term differs by at most 2 ulp of
  itself, and the remaining 6 cover how those differences travel through at
  most 65 same-order additions. Measured on MI355X over the batches below: 0,
  the device's log returned NumPy's doubles on every bin;
* a row's results depend on neither its position in the batch nor R;
* a row outside the support gives +inf / -inf / NaN and changes no other row.

Every batch has at least one bin at the 1e-6 floor of the proportions (an edge
far in the tail), asserted from the kernel's own values.
"""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
W_OUTLIER = 0.1
CDF_ATOL, CDF_ATOL_ILL = 1e-9, 1e-6  # tests/test_cdfdif.py


def _tol(p):
    return CDF_ATOL if (p[4] >= 0.05 and p[6] >= 0.05) else CDF_ATOL_ILL


def _reduce(cdf, freq, n):
    """The reduction loop of the row kernel on the host: theo = [0, cdf, 1],
    p_k = theo[k + 1] - theo[k] floored at 1e-6, chisq the sequential Pearson
    sum, gsq twice the sequential sum of f_k log p_k. Returns (chisq, gsq,
    bins at the floor, sum_k |2 f_k log p_k|)."""
    theo = np.concatenate(([0.0], np.asarray(cdf, dtype=np.float64), [1.0]))
    chisq, gs, floored, mag = 0.0, 0.0, 0, 0.0
    n = float(n)
    for k in range(theo.size - 1):
        p = theo[k + 1] - theo[k]
        if p <= 1e-6:
            p = 1e-6
            floored += 1
        f = float(freq[k])
        ex = p * n
        chisq += ((f - ex) * (f - ex)) / ex
        term = f * float(np.log(p))
        gs += term
        mag += abs(2 * term)
    return chisq, 2 * gs, floored, mag


# ---------------------------------------------------------------- CPU tests

def _mquantiles(x, q):
    """scipy.stats.mstats.mquantiles with its defaults (alphap = betap = 0.4),
    written out."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    out = []
    for p in q:
        aleph = n * p + 0.4 + p * (1 - 0.4 - 0.4)
        k = int(np.floor(min(max(aleph, 1), n - 1)))
        g = min(max(aleph - k, 0.0), 1.0)
        out.append((1 - g) * x[k - 1] + g * x[k])
    return np.array(out)


def _trials(seed, n=400):
    rng = np.random.default_rng(seed)
    rt = 0.3 + rng.gamma(2.0, 0.25, n)
    return np.where(rng.uniform(size=n) < 0.3, -rt, rt)


def test_quantile_stats_against_numpy_restatement():
    from hddm_amd.quantiles import quantile_stats
    rt = _trials(5)
    q = (.1, .3, .5, .7, .9)
    s = quantile_stats(rt, q)
    lo, up = -rt[rt < 0], rt[rt > 0]
    assert lo.size > 50 and up.size > 50
    np.testing.assert_allclose(s["q_lower"], _mquantiles(lo, q), rtol=0, atol=1e-15)
    np.testing.assert_allclose(s["q_upper"], _mquantiles(up, q), rtol=0, atol=1e-15)
    assert s["n_samples"] == 400 and s["p_upper"] == up.size / 400
    assert s["emp_rt"].shape == (11,) and s["emp_rt"][5] == 0.0
    assert np.all(np.diff(s["emp_rt"]) > 0)
    np.testing.assert_array_equal(s["emp_rt"][:5], -s["q_lower"][::-1])
    np.testing.assert_array_equal(s["emp_rt"][6:], s["q_upper"])
    prop = np.array([.1, .2, .2, .2, .2, .1])
    np.testing.assert_allclose(s["freq_obs"], np.concatenate((lo.size * prop, up.size * prop)),
                               rtol=1e-15)
    assert abs(s["freq_obs"].sum() - 400) < 1e-9
    # other quantiles: E = 2 nq + 1
    s3 = quantile_stats(rt, (.25, .5, .75))
    assert s3["emp_rt"].shape == (7,) and s3["freq_obs"].shape == (8,)
    with pytest.raises(ValueError, match="wfpt.3"):
        quantile_stats(np.abs(rt), q, name="wfpt.3")
    with pytest.raises(ValueError, match="upper"):
        quantile_stats(-np.abs(rt), q)
    for bad in (np.nan, 999.0, -999.0):
        with pytest.raises(NotImplementedError):
            quantile_stats(np.append(rt, bad), q)


def test_pool_stats_arithmetic():
    from hddm_amd.quantiles import pool_stats, quantile_stats
    stats = [quantile_stats(_trials(s, n)) for s, n in ((1, 300), (2, 400), (3, 500))]
    pooled = pool_stats(stats)
    assert pooled["n_samples"] == 1200
    np.testing.assert_array_equal(pooled["freq_obs"],
                                  stats[0]["freq_obs"] + stats[1]["freq_obs"]
                                  + stats[2]["freq_obs"])
    np.testing.assert_allclose(pooled["emp_rt"],
                               (stats[0]["emp_rt"] + stats[1]["emp_rt"] + stats[2]["emp_rt"]) / 3,
                               rtol=1e-15)
    assert abs(pooled["p_upper"] - np.mean([s["p_upper"] for s in stats])) < 1e-15
    np.testing.assert_array_equal(pooled["q_upper"], pooled["emp_rt"][6:])
    np.testing.assert_array_equal(pooled["q_lower"], -pooled["emp_rt"][:5][::-1])
    one = pool_stats(stats[:1])
    np.testing.assert_array_equal(one["emp_rt"], stats[0]["emp_rt"])
    with pytest.raises(ValueError):
        pool_stats([])


def test_reduce_restatement():
    """_reduce against the vectorised formulas, its floor and its NaN."""
    from hddm_amd.quantiles import reduce_stats
    rng = np.random.default_rng(7)
    cdf = np.sort(rng.uniform(0.01, 0.99, 11))
    cdf[4] = cdf[3] + 5e-7  # one bin under the floor
    freq = rng.uniform(1, 40, 12)
    n = freq.sum()
    chisq, gsq, floored, mag = _reduce(cdf, freq, n)
    p = np.diff(np.concatenate(([0.], cdf, [1.])))
    assert floored == 1 and p[4] < 1e-6
    p[p <= 1e-6] = 1e-6
    assert abs(chisq - np.sum((freq - p * n) ** 2 / (p * n))) <= 1e-12 * chisq
    assert abs(gsq - 2 * np.sum(freq * np.log(p))) <= 1e-12 * abs(gsq)
    assert mag >= abs(gsq)
    assert reduce_stats(cdf, freq, n) == (chisq, gsq)
    bad = _reduce(np.full(11, np.nan), freq, n)
    assert np.isnan(bad[0]) and np.isnan(bad[1])


def test_argument_errors_before_device_work():
    from hddm_amd import cdfdif_wrapper as cw
    P = np.array([[0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 0.0]])
    x = np.array([[-0.5, 0.0, 0.6]])
    f, n = np.ones((1, 4)), np.array([4.0])
    with pytest.raises(ValueError, match="E"):
        cw.dmat_cdf_rows(np.zeros((1, 65)), P, W_OUTLIER)
    with pytest.raises(ValueError, match="E"):
        cw.dmat_cdf_rows(np.zeros((1, 0)), P, W_OUTLIER)
    with pytest.raises(ValueError, match="R"):
        cw.dmat_cdf_rows(np.zeros((0, 3)), np.zeros((0, 8)), W_OUTLIER)
    with pytest.raises(ValueError):
        cw.dmat_cdf_rows(x, P[:, :7], W_OUTLIER)
    with pytest.raises(ValueError):
        cw.dmat_cdf_rows(x, np.tile(P, (2, 1)), W_OUTLIER)
    with pytest.raises(ValueError):
        cw.dmat_cdf_rows(x, P, W_OUTLIER, freq_obs=f)
    with pytest.raises(ValueError):
        cw.dmat_cdf_rows(x, P, W_OUTLIER, freq_obs=np.ones((1, 3)), n_samples=n)
    with pytest.raises(ZeroDivisionError):
        cw.dmat_cdf_rows(x, P, 0.0, f, n)
    Po = P.copy()
    Po[0, 7] = 0.05
    with pytest.raises(AssertionError):  # cdfdif_wrapper.pyx:20-21: |x| >= 1 / (2 w_outlier)
        cw.dmat_cdf_rows(np.array([[-0.5, 0.0, 5.0]]), Po, W_OUTLIER, f, n)
    with pytest.raises(AssertionError):  # any row with p_outlier > 0, any |x| of the call
        cw.dmat_cdf_rows(np.array([[-0.5, 0.0, 0.6], [-6.0, 0.0, 0.6]]), np.vstack((Po, P)),
                         W_OUTLIER)
    assert cw.ROWS_GRID >= 1 and cw.MAX_EDGES == 64


# ---------------------------------------------------------------- GPU batches

def _golden_params():
    g = np.load(os.path.join(ROOT, "tests", "golden", "cdfdif.npz"), allow_pickle=False)
    return g["params"]


def _freq(seed, R, E):
    rng = np.random.default_rng(seed)
    f = rng.uniform(1.0, 60.0, (R, E + 1))
    return f, f.sum(axis=1)


FAR = 30.0
# the special rows of batch B2 (p_outlier = 0): v, sv, a, z, sz, t, st, p_outlier
ROW_BRANCHES = (0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.3, 0.0)   # window 0.15 .. 0.45
ROW_SIMPLE = (0.5, 0.0, 2.0, 0.5, 0.0, 0.3, 0.0, 0.0)     # sz = st = 0: the 1e-10 substitution
ROW_ZERO_DRIFT = (0.0, 0.0, 1.5, 0.5, 0.2, 0.3, 0.2, 0.0)  # every drift node ~ 0: window_m0
ROW_WIDE = (0.5, 0.1, 9.0, 0.5, 0.1, 0.3, 0.1, 0.0)       # a = 9: series past 64 terms
X_BRANCHES = [-FAR, -1.0, -0.5, -0.3, -0.1, 0.0, 0.1, 0.2, 0.4, 0.8, FAR]
X_SIMPLE = [-FAR, -1.0, -0.6, -0.4, -0.32, 0.0, 0.31, 0.4, 0.6, 1.0, FAR]
X_ZERO_DRIFT = [-FAR, -1.0, -0.5, -0.35, -0.25, 0.0, 0.25, 0.3, 0.5, 1.0, FAR]
X_WIDE = [-300.0, -3.0, -1.0, -0.5, -0.36, 0.0, 0.32, 0.36, 0.5, 1.0, 300.0]
X_GOLDEN = [-FAR, -1.2, -0.7, -0.5, -0.38, 0.0, 0.36, 0.45, 0.6, 1.1, FAR]
GOLDEN_ROWS = (6, 10, 16)   # full models of tests/golden/cdfdif.npz with w_outlier = 0.1


def _batch_a():
    """R = 1, E = 1."""
    return np.array([[FAR]]), np.array([ROW_BRANCHES]), _freq(20, 1, 1)


def _batch_b():
    """R = 3, E = 11: rows of the committed fixture."""
    g = _golden_params()
    assert np.all(g[list(GOLDEN_ROWS), 8] == W_OUTLIER) and np.all(g[list(GOLDEN_ROWS), 7] == 0)
    P = np.ascontiguousarray(g[list(GOLDEN_ROWS), :8])
    return np.tile(X_GOLDEN, (3, 1)), P, _freq(21, 3, 11)


def _batch_b2():
    """R = 4, E = 11: the three branches in one row, sz = st = 0, zero drift, a = 9."""
    P = np.array([ROW_BRANCHES, ROW_SIMPLE, ROW_ZERO_DRIFT, ROW_WIDE])
    x = np.array([X_BRANCHES, X_SIMPLE, X_ZERO_DRIFT, X_WIDE])
    return x, P, _freq(22, 4, 11)


def _batch_c():
    """R = 1, E = 64, p_outlier > 0 (fixture row 21): every |x| < 1 / (2 w_outlier);
    the floor is reached between two edges 1e-6 apart at the far end."""
    g = _golden_params()
    assert g[21, 7] == 0.05 and g[21, 8] == W_OUTLIER
    lo = -np.geomspace(4.9, 0.2, 32)
    up = np.concatenate((np.geomspace(0.25, 4.5, 29), [4.9, 4.9 + 1e-6]))
    x = np.concatenate((lo, [0.0], up))[None]
    assert x.shape == (1, 64) and np.all(np.diff(x[0]) > 0) and np.abs(x).max() < 5
    return x, np.ascontiguousarray(g[21:22, :8]), _freq(23, 1, 64)


def _check_batch(name, x, P, fn):
    """Every assertion of the module docstring on one batch; returns the
    kernel's (cdf, chisq, gsq) and the largest gsq deviation in units of the bar."""
    import oracle
    from hddm_amd import cdfdif_wrapper as cw
    f, n = fn
    cdf, chisq, gsq = cw.dmat_cdf_rows(x, P, W_OUTLIER, f, n)
    only = cw.dmat_cdf_rows(x, P, W_OUTLIER)
    assert np.array_equal(only, cdf), name  # the CDF-only call: the same values
    floored_any, worst_g, worst_d = 0, 0.0, 0.0
    for r in range(x.shape[0]):
        own = cw.dmat_cdf_array(np.ascontiguousarray(x[r]), *P[r], W_OUTLIER)
        assert np.array_equal(cdf[r], own), (name, r, cdf[r] - own)
        ref = oracle.dmat_cdf_array(np.ascontiguousarray(x[r]), *P[r], W_OUTLIER)
        d = float(np.abs(cdf[r] - ref).max())
        worst_d = max(worst_d, d)
        assert d <= _tol(P[r]), (name, r, d)
        c, g, floored, mag = _reduce(cdf[r], f[r], n[r])
        floored_any += floored
        assert chisq[r] == c, (name, r, chisq[r], c)
        dev = abs(gsq[r] - g) / (EPS * mag)
        worst_g = max(worst_g, dev)
        assert dev <= 8, (name, r, gsq[r], g, dev)
        assert np.isfinite(chisq[r]) and np.isfinite(gsq[r])
    print(f"{name}: R={x.shape[0]} E={x.shape[1]} max |dF| vs oracle = {worst_d:.3e}, "
          f"max |gsq - _reduce| = {worst_g:.3f} x 2^-52 sum|2 f log p| (bar 8), "
          f"{floored_any} bins at the floor")
    assert floored_any >= 1, name
    return cdf, chisq, gsq


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["a", "b", "b2", "c"])
def test_rows_match_array_path_and_reduction(batch):
    x, P, fn = {"a": _batch_a, "b": _batch_b, "b2": _batch_b2, "c": _batch_c}[batch]()
    if batch == "b2":
        import oracle
        # the a = 9 row's series beyond the window runs past one round of 64 terms
        pr = oracle.cdf_probe(np.array(X_WIDE), *ROW_WIDE, W_OUTLIER)
        assert np.any(pr.stop[:, 42] > 64), pr.stop[:, 42]
        # and the first row's edges take all three branches
        assert set(oracle.cdf_probe(np.array(X_BRANCHES), *ROW_BRANCHES,
                                    W_OUTLIER).branch) == {0, 1, 2}
        # window edges of the zero-drift row run the drift-node-at-zero series
        zs = oracle.cdf_probe(np.array(X_ZERO_DRIFT), *ROW_ZERO_DRIFT, W_OUTLIER)
        assert np.any(zs.stop[:, 36:42] >= 0)
    _check_batch(batch, x, P, fn)


def _seven():
    xb, Pb, _ = _batch_b()
    x2, P2, _ = _batch_b2()
    return np.vstack((xb, x2)), np.vstack((Pb, P2))


@pytest.mark.gpu
def test_grid_stride_and_batch_independence():
    """R = one more than the launcher's grid: the stride loop runs, and every
    row equals the same row evaluated alone (cdf, chisq and gsq, bit for bit)."""
    from hddm_amd import cdfdif_wrapper as cw
    x7, P7 = _seven()
    f7, n7 = _freq(24, 7, 11)
    R = cw.ROWS_GRID + 1
    src = np.arange(R) % 7
    cdf, chisq, gsq = cw.dmat_cdf_rows(x7[src], P7[src], W_OUTLIER, f7[src], n7[src])
    floored = 0
    for r in range(7):
        c1, s1, g1 = cw.dmat_cdf_rows(x7[r:r + 1], P7[r:r + 1], W_OUTLIER, f7[r:r + 1],
                                      n7[r:r + 1])
        sel = src == r
        assert np.all(cdf[sel] == c1[0]) and np.all(chisq[sel] == s1[0]) \
            and np.all(gsq[sel] == g1[0]), r
        floored += _reduce(c1[0], f7[r], n7[r])[2]
    assert floored >= 1
    # the last row is the one block 0 takes in its second turn
    assert src[-1] == (R - 1) % 7 and np.isfinite(chisq[-1])


INVALID = {"a = 0": (2, 0.0), "z + sz/2 > 1": (3, 0.97), "t - st/2 < 0": (6, 1.0),
           "NaN v": (0, np.nan), "p_outlier = 1.5": (7, 1.5)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(INVALID))
def test_invalid_rows_do_not_touch_the_others(kind):
    """R = 5: rows 1 and 3 made invalid (one, the other, both); they give
    +inf / -inf / NaN, rows 0, 2 and 4 the all-valid batch's values bit for bit."""
    from hddm_amd import cdfdif_wrapper as cw
    x7, P7 = _seven()
    pick = [3, 0, 4, 1, 5]  # rows 1 and 3: fixture rows with sz > 0 and st > 0
    x, P = x7[pick].copy(), P7[pick].copy()
    assert np.all(P[[1, 3], 4] > 0.06) and np.all(P[[1, 3], 5] < 0.5)
    x[:, 0], x[:, -2:] = -4.9, [4.9 - 1e-7, 4.9]  # p_outlier = 1.5 asks for |x| < 5
    f, n = _freq(25, 5, 11)
    good = cw.dmat_cdf_rows(x, P, W_OUTLIER, f, n)
    assert sum(_reduce(good[0][r], f[r], n[r])[2] for r in range(5)) >= 1
    col, val = INVALID[kind]
    for bad in ((1,), (3,), (1, 3)):
        Q = P.copy()
        Q[list(bad), col] = val
        cdf, chisq, gsq = cw.dmat_cdf_rows(x, Q, W_OUTLIER, f, n)
        for r in range(5):
            if r in bad:
                assert np.all(np.isnan(cdf[r])) and chisq[r] == np.inf and gsq[r] == -np.inf
            else:
                assert np.array_equal(cdf[r], good[0][r]) and chisq[r] == good[1][r] \
                    and gsq[r] == good[2][r], (kind, bad, r)
        only = cw.dmat_cdf_rows(x, Q, W_OUTLIER)
        assert np.array_equal(only, cdf, equal_nan=True)
