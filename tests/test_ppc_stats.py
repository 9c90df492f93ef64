"""Per-row RT statistics on the device (wfpt_rt_stats_rows and the fused
sampler entries, stats_kernels.hip), hddm_amd.ppc and HDDM.post_pred_stats.

Reference: a NumPy restatement of gen_ppc_stats (hddm/utils.py:241-265) for one
row, whose percentile rule is first held against scipy.stats.scoreatpercentile
itself. Tolerances:
  * n, n_ub, n_lb, accuracy and every percentile, on every tier; fused against
    unfused; a row against itself under another launch shape: none
    (assert_array_equal, NaN positions equal);
  * mean, against a long-double two-pass restatement: (m + 1) 2^-53 mean(|x|),
    the worst case of any summation order of m doubles plus the division;
  * std, against the same: (m + 8) 2^-52 (ref + mean(|x|)); the mean(|x|) term
    covers a row of equal values, where the rounded mean's error is what is
    left.
"""
import sys
import types

import numpy as np
import pytest

from test_sim import COUNT_MIX, PARAM_ROWS, counts_of

DEFAULT_Q = (10, 30, 50, 70, 90)
Q_LISTS = {"default": DEFAULT_Q, "none": (), "ends": (0, 100), "ci": (2.5, 97.5),
           "sixteen": tuple(np.linspace(0, 100, 16))}
WAVE_MAX, BLOCK_MAX = 256, 4096  # the tier boundaries
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
KINDS = ("mixed", "all_upper", "all_lower", "one_upper", "one_lower", "ties", "equal",
         "zeros_nan", "span")


# ---------------------------------------------------------------- restatement

def percentile(s, q):
    """scipy's 'fraction' rule restated on the sorted values s."""
    idx = q / 100. * (s.shape[0] - 1)
    i = int(idx)
    if i == idx:
        return s[i]
    w0, w1 = (i + 1) - idx, idx - i
    return (s[i] * w0 + s[i + 1] * w1) / (w0 + w1)


def row_ref(x, quantiles):
    """One row's K statistics by NumPy on the split values."""
    x = np.asarray(x, dtype=np.float64)
    ub, lb = x[x > 0], x[x < 0]
    nan = float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        out = [x.size, ub.size, lb.size, np.float64(ub.size) / np.float64(x.size)]
    for part, vals in ((ub, np.sort(ub)), (lb, np.sort(np.abs(lb)))):
        out += [np.mean(part) if part.size else nan, np.std(part) if part.size else nan]
        out += [percentile(vals, q) if part.size else nan for q in quantiles]
    return np.array(out, dtype=np.float64)


def moments_ref(vals):
    """(mean, std, mean|x|) in long double, two-pass."""
    v = np.asarray(vals, dtype=np.longdouble)
    mean = v.sum() / v.size
    return mean, np.sqrt(((v - mean) ** 2).sum() / v.size), np.abs(v).sum() / v.size


def check_rows(got, rows, quantiles):
    """got (R, K) against the restatement of every row: exact columns equal,
    means and standard deviations inside the derived bounds."""
    nq = len(quantiles)
    assert got.shape == (len(rows), 8 + 2 * nq)
    exact = [0, 1, 2, 3] + list(range(6, 6 + nq)) + list(range(8 + nq, 8 + 2 * nq))
    for r, x in enumerate(rows):
        ref = row_ref(x, quantiles)
        np.testing.assert_array_equal(got[r, exact], ref[exact], err_msg=f"row {r} (n={len(x)})")
        for c, part in ((4, x[x > 0]), (6 + nq, x[x < 0])):
            m = part.size
            if m == 0:
                assert np.isnan(got[r, c]) and np.isnan(got[r, c + 1]), (r, c)
                continue
            mean, std, scale = moments_ref(part)
            assert abs(got[r, c] - mean) <= (m + 1) * 2.0 ** -53 * scale, (r, c, m, got[r, c], mean)
            assert abs(got[r, c + 1] - std) <= (m + 8) * 2.0 ** -52 * (std + scale), \
                (r, c, m, got[r, c + 1], std)


def make_row(kind, n, rng):
    mag = 0.3 + rng.gamma(2.0, 0.4, n)
    sign = np.where(rng.random(n) < 0.65, 1.0, -1.0)
    if kind == "mixed":
        return sign * mag
    if kind == "all_upper":
        return mag
    if kind == "all_lower":
        return -mag
    if kind in ("one_upper", "one_lower"):
        x = -mag if kind == "one_upper" else mag
        if n:
            x[rng.integers(n)] *= -1
        return x
    if kind == "ties":
        return np.round(sign * mag, 2)
    if kind == "equal":
        return np.full(n, 0.73) * (sign if n % 2 else 1.0)
    if kind == "zeros_nan":
        x = np.round(sign * mag, 2)
        x[0::5] = 0.0
        x[1::7] = -0.0
        x[2::11] = np.nan
        return x
    assert kind == "span"
    return sign * 10.0 ** rng.uniform(-3, 3, n)


def pack(rows):
    off = np.r_[0, np.cumsum([len(x) for x in rows])].astype(np.int64)
    return (np.concatenate(rows) if rows else np.empty(0)), off


_CACHE = {}


def synthetic(max_len):
    """Every row length up to max_len in every kind of content, built once."""
    if max_len not in _CACHE:
        rng = np.random.default_rng(20261020)
        _CACHE[max_len] = [make_row(k, n, rng) for n in LENGTHS if n <= max_len for k in KINDS]
    return _CACHE[max_len]


def mix_table():
    """300 rows with test_sim's COUNT_MIX: several rows share a block."""
    if "mix" not in _CACHE:
        rng = np.random.default_rng(300)
        _CACHE["mix"] = [make_row("ties" if r % 3 else "zeros_nan", int(n), rng)
                         for r, n in enumerate(counts_of(300))]
    return _CACHE["mix"]


# ------------------------------------------------------------------------ CPU

def test_percentile_rule_is_scipys_and_gen_ppc_stats_agrees():
    from scipy.stats import scoreatpercentile
    from hddm_amd import ppc
    rng = np.random.default_rng(1)
    qs = (0, 2.5, 10, 30, 33.3, 50, 70, 90, 97.5, 100)
    for n in (1, 2, 3, 4, 7, 10, 64, 65, 101, 250):
        for decimals in (1, 2, 6):
            s = np.sort(np.round(0.3 + rng.gamma(2.0, 0.4, n), decimals))
            for q in qs:
                assert percentile(s, q) == scoreatpercentile(s, q), (n, decimals, q)
                assert ppc.scoreatpercentile(s[::-1], q) == scoreatpercentile(s, q)
    names = ["accuracy", "mean_ub", "std_ub"] + [f"{q}q_ub" for q in DEFAULT_Q] + \
            ["mean_lb", "std_lb"] + [f"{q}q_lb" for q in DEFAULT_Q]
    stats = ppc.gen_ppc_stats()
    assert list(stats) == names
    for kind in ("mixed", "ties", "zeros_nan", "span", "one_upper"):
        x = make_row(kind, 97, rng)
        ref = row_ref(x, DEFAULT_Q)
        np.testing.assert_array_equal([stats[k](x) for k in names], ref[3:])
    with np.errstate(invalid="ignore"), pytest.warns(RuntimeWarning):
        only_ub = [stats[k](np.array([0.5, 0.7])) for k in names]
    np.testing.assert_array_equal(only_ub, row_ref([0.5, 0.7], DEFAULT_Q)[3:])


def test_rt_stats_names():
    from hddm_amd import wfpt
    assert wfpt.rt_stats_names() == [
        "n", "n_ub", "n_lb", "accuracy", "mean_ub", "std_ub", "10q_ub", "30q_ub", "50q_ub",
        "70q_ub", "90q_ub", "mean_lb", "std_lb", "10q_lb", "30q_lb", "50q_lb", "70q_lb", "90q_lb"]
    assert wfpt.rt_stats_names(()) == ["n", "n_ub", "n_lb", "accuracy", "mean_ub", "std_ub",
                                       "mean_lb", "std_lb"]
    assert wfpt.rt_stats_names((2.5,))[6] == "2.5q_ub"
    for q in Q_LISTS.values():
        assert len(wfpt.rt_stats_names(q)) == 8 + 2 * len(q)


def test_summarize_on_a_hand_made_array():
    from hddm_amd import ppc
    names = ["accuracy", "mean_lb"]
    observed = np.array([[0.5, -0.9], [0.8, np.nan]])
    sampled = np.array([[[0.4, -1.0], [0.7, np.nan]],
                        [[0.6, np.nan], [0.9, np.nan]],
                        [[0.8, -0.6], [0.8, np.nan]],
                        [[0.2, -0.8], [1.0, np.nan]]])
    t = ppc.summarize(observed, sampled, names, nodes=["a", "b"])
    assert list(t.index.names) == ["node", "stat"]
    assert list(t.columns) == ["observed", "mean", "std", "SEM", "MSE", "credible", "quantile",
                               "mahalanobis"]
    assert list(t.index) == [("a", "accuracy"), ("a", "mean_lb"), ("b", "accuracy"),
                             ("b", "mean_lb")]
    row = t.loc[("a", "accuracy")]
    s = sampled[:, 0, 0]
    assert row["observed"] == 0.5 and row["mean"] == np.mean(s) and row["std"] == np.std(s)
    assert row["SEM"] == (0.5 - np.mean(s)) ** 2 and row["MSE"] == np.mean((s - 0.5) ** 2)
    assert row["credible"] and row["quantile"] == 50.0
    assert row["mahalanobis"] == abs(0.5 - np.mean(s)) / np.std(s)
    row = t.loc[("a", "mean_lb")]  # one sweep never reached the lower boundary
    s = np.array([-1.0, -0.6, -0.8])
    assert row["mean"] == np.mean(s) and row["std"] == np.std(s)
    assert row["MSE"] == np.mean((s + 0.9) ** 2) and row["quantile"] == 100.0 / 3
    lo, hi = np.percentile(s, [2.5, 97.5])
    assert row["credible"] == (lo <= -0.9 <= hi)
    row = t.loc[("b", "mean_lb")]  # no sweep and no observed trial did
    assert np.isnan(row[["observed", "mean", "std", "SEM", "MSE", "quantile", "mahalanobis"]]
                    .to_numpy(dtype=float)).all() and not row["credible"]
    row = t.loc[("b", "accuracy")]
    lo, hi = np.percentile([.7, .9, .8, 1.], [2.5, 97.5])
    assert row["credible"] == (lo <= 0.8 <= hi) and row["quantile"] == 50.0
    with pytest.raises(ValueError):
        ppc.summarize(observed, sampled)  # K = 2 is not the default statistics: names needed
    with pytest.raises(ValueError):
        ppc.summarize(observed, sampled[:, :1], names)


def test_argument_checks_before_any_device_work():
    """Python-level ValueErrors, and the C ABI's WFPT_ERR_ARG with a NULL
    context: a bad argument is reported before the context is looked at."""
    import ctypes
    from hddm_amd import _lib, wfpt
    x, off = np.array([0.5, -0.4, 0.7]), np.array([0, 2, 3], dtype=np.int64)
    for bad in ((101,), (-1,), (float("nan"),), tuple(range(17))):
        with pytest.raises(ValueError):
            wfpt.rt_stats_rows(x, off, bad)
        with pytest.raises(ValueError):
            wfpt.gen_rts_stats_nodes(PARAM_ROWS[:1], 5, quantiles=bad, seed=1)
    for bad_off in ([0, 3, 2], [1, 2, 3], [0], [0, 2, 4]):
        with pytest.raises(ValueError):
            wfpt.rt_stats_rows(x, np.array(bad_off, dtype=np.int64))
    with pytest.raises(ValueError):
        wfpt.rt_stats_rows(x, off, tier=4)
    with pytest.raises(ValueError):
        wfpt.gen_rts_stats_nodes(PARAM_ROWS[:1], 5, method="exact", seed=1)
    with pytest.raises(TypeError):
        wfpt.gen_rts_stats_nodes(PARAM_ROWS[:1], 5, seed=1, max_t=1.0)  # a drift keyword

    out = np.empty(2 * 18)
    q = np.array(DEFAULT_Q, dtype=np.float64)
    pd_, pi = _lib.dptr, lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    def call(x=x, off=off, R=2, q=q, nq=5, tier=0, out=out):
        rc = _lib.wfpt_rt_stats_rows_ex(None, pd_(x) if x is not None else None,
                                        pi(off) if off is not None else None, R,
                                        pd_(q) if q is not None else None, nq, tier,
                                        pd_(out) if out is not None else None)
        return rc, _lib.wfpt_last_error()
    assert call(nq=17) == (2, b"rt_stats_rows: nq outside 0..16")
    assert call(nq=-1)[0] == 2
    assert call(q=np.array([10, 30, 101, 70, 90.]))[1] == \
        b"rt_stats_rows: percentile 2 outside [0, 100]"
    assert b"percentile 0" in call(q=np.array([np.nan] * 5))[1]
    assert b"off falls at row 1" in call(off=np.array([0, 3, 2], dtype=np.int64))[1]
    assert b"off[0]" in call(off=np.array([1, 2, 3], dtype=np.int64))[1]
    for kw in ({"x": None}, {"off": None}, {"q": None}, {"out": None}):
        rc, msg = call(**kw)
        assert rc == 2 and b"null pointer" in msg and b"context" not in msg, kw
    assert call(R=0)[0] == 2 and b"tier outside" in call(tier=5)[1]
    long_off = np.array([0, WAVE_MAX + 1], dtype=np.int64)
    long_x = np.ones(WAVE_MAX + 1)
    assert b"more than the forced tier 1 holds" in call(x=long_x, off=long_off, R=1, tier=1)[1]
    assert call(x=long_x, off=long_off, R=1, tier=2) == (2, b"null pointer (context)")
    assert call() == (2, b"null pointer (context)")  # everything else was in order

    # the fused entries: the statistics' arguments are checked with the sampler's
    grid = np.arange(-5, 5, 0.5)
    row = _lib.make_params(*PARAM_ROWS[0])
    cnt = np.array([5], dtype=np.int64)
    nun = ctypes.c_int64()
    for nq_, q_, so, want in ((17, q, out, b"nq outside"), (5, None, out, b"null pointer"),
                              (5, q, None, b"null pointer"),
                              (5, np.array([0, 1, 2, 3, 100.5]), out, b"percentile 4")):
        pq, ps = (pd_(q_) if q_ is not None else None), (pd_(so) if so is not None else None)
        assert _lib.wfpt_gen_rts_nodes_stats(None, pd_(grid), grid.size, ctypes.byref(row), 1,
                                             pi(cnt), None, None, 1, 0, None, pq, nq_, ps) == 2
        assert want in _lib.wfpt_last_error()
        assert _lib.wfpt_gen_rts_drift_nodes_stats(None, ctypes.byref(row), 1, None, pi(cnt), 1e-2,
                                                   1.0, 100, 1, None, ctypes.byref(nun), pq, nq_,
                                                   ps) == 2
        assert want in _lib.wfpt_last_error()
    # out == NULL is allowed there: the call gets as far as the missing context
    assert _lib.wfpt_gen_rts_nodes_stats(None, pd_(grid), grid.size, ctypes.byref(row), 1, pi(cnt),
                                         None, None, 1, 0, None, pd_(q), 5, pd_(out)) == 2
    assert _lib.wfpt_last_error() == b"null pointer (context)"
    assert _lib.wfpt_gen_rts_nodes(None, pd_(grid), grid.size, ctypes.byref(row), 1, pi(cnt), None,
                                   None, 1, 0, None) == 2
    assert _lib.wfpt_last_error() == b"null pointer (out)"  # the plain entry still needs it


def test_install_rebinds_post_pred_stats_and_restores():
    from hddm_amd import integration, ppc

    def theirs(data, sim_datasets, **kw):
        return "reference"
    utils = types.ModuleType("hddm.utils")
    utils.post_pred_stats = theirs
    utils.gen_ppc_stats = "untouched"
    keep = {k: sys.modules.get(k) for k in ("wfpt", "cdfdif_wrapper", "hddm.utils")}
    inst = integration.install(utils_module=utils)
    try:
        assert utils.post_pred_stats is ppc.post_pred_stats
        assert utils.gen_ppc_stats == "untouched"
        assert "hddm.utils" not in sys.modules or sys.modules["hddm.utils"] is keep["hddm.utils"]
    finally:
        inst.uninstall()
    assert utils.post_pred_stats is theirs
    # found in sys.modules when not given; absent: nothing happens
    sys.modules["hddm.utils"] = utils
    try:
        inst = integration.install()
        assert utils.post_pred_stats is ppc.post_pred_stats
        inst.uninstall()
        assert utils.post_pred_stats is theirs
    finally:
        del sys.modules["hddm.utils"]
    inst = integration.install()
    assert "hddm.utils" not in sys.modules
    inst.uninstall()
    for k, v in keep.items():
        assert sys.modules.get(k) is v


def test_chains_and_regressor_refuse_post_pred_stats():
    from hddm_amd.hierarchical import HDDMChains
    from hddm_amd.regression import HDDMRegressor
    for cls in (HDDMChains, HDDMRegressor):
        with pytest.raises(NotImplementedError):
            cls.post_pred_stats(object())


# ------------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("tier", (0, 1, 2, 3))
@pytest.mark.parametrize("qname", list(Q_LISTS))
def test_rows_on_every_tier(gpu, tier, qname):
    """Every length (0 .. one past each tier boundary) in every kind of
    content; a forced tier scores the rows it admits, tier 3 all of them (the
    global tier's lower end)."""
    rows = synthetic({0: max(LENGTHS), 1: WAVE_MAX, 2: BLOCK_MAX, 3: max(LENGTHS)}[tier])
    if tier == 3 and qname != "default":
        rows = [x for x in rows if len(x) <= 257 or len(x) == 4097]  # fewer launches
    rts, off = pack(rows)
    got = gpu.rt_stats_rows(rts, off, Q_LISTS[qname], tier=tier)
    check_rows(got, rows, Q_LISTS[qname])


@pytest.mark.gpu
def test_tiers_agree_exactly_where_they_overlap(gpu):
    nq = len(DEFAULT_Q)
    exact = [0, 1, 2, 3] + list(range(6, 6 + nq)) + list(range(8 + nq, 8 + 2 * nq))
    rows = synthetic(WAVE_MAX)
    rts, off = pack(rows)
    by_tier = [gpu.rt_stats_rows(rts, off, tier=t) for t in (0, 1, 2, 3)]
    for other in by_tier[1:]:
        np.testing.assert_array_equal(other[:, exact], by_tier[0][:, exact])
    np.testing.assert_array_equal(by_tier[1], by_tier[0])  # tier 0 took the wave tier here


@pytest.mark.gpu
def test_row_is_independent_of_neighbours_and_launch_shape(gpu):
    rows = mix_table()
    assert sorted({len(x) for x in rows}) == sorted(COUNT_MIX)
    rts, off = pack(rows)
    got = gpu.rt_stats_rows(rts, off)
    check_rows(got, rows, DEFAULT_Q)
    perm = np.random.default_rng(9).permutation(len(rows))
    rts_p, off_p = pack([rows[i] for i in perm])
    np.testing.assert_array_equal(gpu.rt_stats_rows(rts_p, off_p), got[perm])
    for r, x in enumerate(rows):
        alone = gpu.rt_stats_rows(x, np.array([0, len(x)], dtype=np.int64))
        np.testing.assert_array_equal(alone[0], got[r], err_msg=f"row {r}")


def product_table():
    """PARAM_ROWS x COUNT_MIX: every parameter row with every count."""
    R = len(PARAM_ROWS) * len(COUNT_MIX)
    P = PARAM_ROWS[np.arange(R) % len(PARAM_ROWS)]
    cnt = np.array([COUNT_MIX[(r // len(PARAM_ROWS)) % len(COUNT_MIX)] for r in range(R)],
                   dtype=np.int64)
    return P, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ((-5, 5, 0.5), (-6, 6, 1e-2)))
def test_fused_cdf_sampler_equals_unfused(gpu, grid):
    P, cnt = product_table()
    kw = dict(cdf_lb=grid[0], cdf_ub=grid[1], dt=grid[2])
    rts0, off0 = gpu.gen_rts_from_cdf_nodes(P, cnt, seed=77, **kw)
    stats, off, rts = gpu.gen_rts_stats_nodes(P, cnt, "cdf", seed=77, return_draws=True, **kw)
    np.testing.assert_array_equal(off, off0)
    np.testing.assert_array_equal(rts, rts0)
    np.testing.assert_array_equal(stats, gpu.rt_stats_rows(rts0, off0))
    check_rows(stats, [rts0[off0[r]:off0[r + 1]] for r in range(len(cnt))], DEFAULT_Q)
    lean, off2 = gpu.gen_rts_stats_nodes(P, cnt, "cdf", seed=77, **kw)
    np.testing.assert_array_equal(lean, stats)
    np.testing.assert_array_equal(off2, off0)
    m = np.arange(*grid).size - 1
    tiled, _ = gpu.gen_rts_stats_nodes(P, cnt, "cdf", seed=77, max_workspace=5 * 8 * m, **kw)
    np.testing.assert_array_equal(tiled, stats)
    other = gpu.gen_rts_stats_nodes(P, cnt, "cdf", quantiles=(2.5, 97.5), seed=77, **kw)[0]
    np.testing.assert_array_equal(other, gpu.rt_stats_rows(rts0, off0, (2.5, 97.5)))
    # supplied uniforms and the global RNG follow the sampler's rules too
    u = np.random.default_rng(3).random(int(off0[-1]))
    a, _ = gpu.gen_rts_from_cdf_nodes(P, cnt, u=u, u_delay=u[::-1].copy(), **kw)
    b = gpu.gen_rts_stats_nodes(P, cnt, u=u, u_delay=u[::-1].copy(), return_draws=True, **kw)[2]
    np.testing.assert_array_equal(a, b)
    np.random.seed(12)
    a, _ = gpu.gen_rts_from_cdf_nodes(P, cnt, **kw)
    np.random.seed(12)
    b = gpu.gen_rts_stats_nodes(P, cnt, return_draws=True, **kw)[2]
    np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_fused_drift_sampler_equals_unfused_and_counts_unfinished_walks(gpu):
    P, n = PARAM_ROWS, 65
    kw = dict(dt=1e-2, max_t=0.6, unfinished="nan")
    rts0, off0 = gpu.gen_rts_from_drift_nodes(P, n, seed=5, **kw)
    nan = np.isnan(rts0)
    assert 0 < nan.sum() < rts0.size  # some walks ran out of steps
    stats, off, rts = gpu.gen_rts_stats_nodes(P, n, "drift", seed=5, return_draws=True, **kw)
    np.testing.assert_array_equal(off, off0)
    np.testing.assert_array_equal(rts, rts0)
    np.testing.assert_array_equal(stats, gpu.rt_stats_rows(rts0, off0))
    rows = [rts0[off0[r]:off0[r + 1]] for r in range(len(P))]
    check_rows(stats, rows, DEFAULT_Q)
    # an unfinished walk counts in n and in neither boundary
    np.testing.assert_array_equal(stats[:, 0], n)
    np.testing.assert_array_equal(stats[:, 0] - stats[:, 1] - stats[:, 2],
                                  [np.isnan(x).sum() for x in rows])
    lean, _ = gpu.gen_rts_stats_nodes(P, n, "drift", seed=5, **kw)
    np.testing.assert_array_equal(lean, stats)
    # ... and is counted on the device when the draws stay there
    with pytest.raises(RuntimeError, match=f"{nan.sum()} of {rts0.size} draws"):
        gpu.gen_rts_stats_nodes(P, n, "drift", seed=5, dt=1e-2, max_t=0.6)
    with pytest.raises(RuntimeError, match=f"{nan.sum()} of {rts0.size} draws"):
        gpu.gen_rts_stats_nodes(P, n, "drift", seed=5, dt=1e-2, max_t=0.6, return_draws=True)
    done = gpu.gen_rts_stats_nodes(P, n, "drift", seed=5, dt=1e-2)[0]  # default max_t: all cross
    np.testing.assert_array_equal(done[:, 1] + done[:, 2], n)
    np.testing.assert_array_equal(
        done, gpu.rt_stats_rows(*gpu.gen_rts_from_drift_nodes(P, n, seed=5, dt=1e-2)))
    empty = gpu.gen_rts_stats_nodes(P[:2], 0, "drift", seed=5, dt=1e-2)[0]  # no draw at all
    np.testing.assert_array_equal(empty[:, :3], 0)
    assert np.isnan(empty[:, 3:]).all()


@pytest.mark.gpu
def test_failures_write_nothing_and_leave_the_context_usable(gpu):
    from hddm_amd import _lib
    import ctypes
    rows = synthetic(WAVE_MAX)[:20]
    rts, off = pack(rows)
    good = gpu.rt_stats_rows(rts, off)

    def still_good():
        np.testing.assert_array_equal(gpu.rt_stats_rows(rts, off), good)
    bad = PARAM_ROWS[:3].copy()
    bad[1, 2] = 0.0  # a == 0: the row has no CDF
    for draws in (False, True):
        with pytest.raises(RuntimeError, match="row 1 has no CDF"):
            gpu.gen_rts_stats_nodes(bad, 10, "cdf", seed=1, return_draws=draws, cdf_lb=-5,
                                    cdf_ub=5, dt=0.5)
        still_good()
    # ... and the C entry leaves both outputs as they were
    grid = np.arange(-5, 5, 0.5)
    table = np.zeros((3, 8))
    table[:, :7] = bad
    cnt = np.full(3, 10, dtype=np.int64)
    out, stats = np.full(30, -7.0), np.full(3 * 18, -7.0)
    q = np.array(DEFAULT_Q, dtype=np.float64)
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    ctx = _lib.context()
    rc = _lib.wfpt_gen_rts_nodes_stats(ctx.handle, _lib.dptr(grid), grid.size,
                                       table.ctypes.data_as(_lib._PP), 3, pi(cnt), None, None, 1,
                                       0, _lib.dptr(out), _lib.dptr(q), 5, _lib.dptr(stats))
    assert rc == 4 and (out == -7.0).all() and (stats == -7.0).all()
    still_good()
    for call in (lambda: gpu.rt_stats_rows(rts, off, (50, 101)),
                 lambda: gpu.rt_stats_rows(rts, np.r_[off[:-1], off[-2] - 1]),
                 lambda: gpu.rt_stats_rows(np.ones(WAVE_MAX + 1), [0, WAVE_MAX + 1], tier=1),
                 lambda: gpu.rt_stats_rows(np.ones(BLOCK_MAX + 1), [0, BLOCK_MAX + 1], tier=2)):
        with pytest.raises(ValueError):
            call()
        still_good()
    rc = _lib.wfpt_rt_stats_rows(ctx.handle, _lib.dptr(rts), pi(off), len(rows),
                                 _lib.dptr(np.zeros(17)), 17, _lib.dptr(stats))
    assert rc == 2 and (stats == -7.0).all()
    still_good()
    with pytest.raises(RuntimeError, match="cannot be simulated"):
        gpu.gen_rts_stats_nodes(bad, 10, "drift", seed=1, dt=1e-2)
    still_good()


@pytest.mark.gpu
def test_model_post_pred_stats(gpu):
    import pandas as pd
    from hddm_amd import ppc
    from hddm_amd.hierarchical import HDDM, HDDMChains, gen_data
    data, _ = gen_data(n_subj=3, n_trials=40, seed=3)
    m = HDDM(data, depends_on={"v": "cond"}, include=("st",), seed=4)
    m.sample(30, burn=10)
    seed = 21
    table, sampled = m.post_pred_stats(samples=5, seed=seed, dt=1e-2, return_sampled=True)
    names = gpu.rt_stats_names()
    K = len(names)
    assert sampled.shape == (5, m.n_nodes, K)
    # the fused path against the data sets it never materialised
    frame = m.post_pred_gen(samples=5, seed=seed, dt=1e-2)
    observed_frame = pd.DataFrame({"rt": m.signed_rt, "node": m.node_codes})
    table2, sampled2 = ppc.post_pred_stats(observed_frame, frame, return_sampled=True)
    np.testing.assert_array_equal(sampled, sampled2)
    pd.testing.assert_frame_equal(table, table2)
    assert m.post_pred_stats(samples=5, seed=seed, dt=1e-2).equals(table)
    # observed: the restatement on each node's own RTs
    observed = table["observed"].to_numpy().reshape(m.n_nodes, K)
    check_rows(observed, [m.signed_rt[m.node_codes == k] for k in range(m.n_nodes)], DEFAULT_Q)
    assert list(table.index[:K]) == [(0, nm) for nm in names]
    # the summary columns: a direct NumPy computation
    obs = observed.reshape(-1)
    sam = sampled.reshape(5, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(table["mean"], np.nanmean(sam, axis=0))
        np.testing.assert_array_equal(table["std"], np.nanstd(sam, axis=0))
        np.testing.assert_array_equal(table["SEM"], (obs - np.nanmean(sam, axis=0)) ** 2)
        np.testing.assert_array_equal(table["MSE"], np.nanmean((sam - obs) ** 2, axis=0))
        lo, hi = np.nanpercentile(sam, [2.5, 97.5], axis=0)
        np.testing.assert_array_equal(table["credible"], (obs >= lo) & (obs <= hi))
        np.testing.assert_array_equal(table["quantile"], 100. * np.sum(sam <= obs, axis=0)
                                      / np.sum(~np.isnan(sam), axis=0))
        np.testing.assert_array_equal(
            table["mahalanobis"], np.abs(obs - np.nanmean(sam, axis=0)) / np.nanstd(sam, axis=0))
    # the drift method and other quantiles go the same way
    t3, s3 = m.post_pred_stats(samples=2, seed=seed, dt=1e-2, method="drift",
                               quantiles=(25, 75), return_sampled=True)
    f3 = m.post_pred_gen(samples=2, seed=seed, dt=1e-2, method="drift")
    np.testing.assert_array_equal(
        s3, ppc.post_pred_stats(observed_frame, f3, (25, 75), return_sampled=True)[1])
    assert s3.shape == (2, m.n_nodes, 12) and t3.index[6] == (0, "25q_ub")
    with pytest.raises(NotImplementedError):
        HDDMChains.post_pred_stats(m)
