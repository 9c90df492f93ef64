"""Regression likelihoods: RegDataset.wiener_like_reg / wiener_like_reg_groups
(reg_kernels.hip: reg_fill_kernel; hddm_regression.py:26-36 into
wfpt.pyx:244-274).

The predictor has a defined order (left to right, every product and sum
rounded separately) and correctly rounded links, so the predicted parameters
are checked bit for bit against a plain-Python restatement; the densities are
checked against the oracle's wiener_like_multi at the device's own predictions
with the project's bars (max|dlogp| < 1e-6 per trial, the total within 1e-9
relative of math.fsum, tests/test_rl.py::test_rlddm_terms_and_sum).
"""
import ctypes
import decimal
import functools
import inspect
import math

import numpy as np
import pytest

HDDM_KNOBS = dict(err=1e-4, n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3)
FAMILIES = {
    "simple": dict(sv=0.0, z=0.5, sz=0.0, st=0.0, p_outlier=0.05, w_outlier=0.1, **HDDM_KNOBS),
    "full": dict(sv=0.3, z=0.5, sz=0.2, st=0.1, p_outlier=0.05, w_outlier=0.1, **HDDM_KNOBS),
    "fixed": dict(sv=0.3, z=0.5, sz=0.2, st=0.1, p_outlier=0.05, w_outlier=0.1, err=1e-4,
                  n_st=2, n_sz=2, use_adaptive=0, simps_err=1e-3),
}
KNOB = ("n_st", "n_sz", "use_adaptive", "simps_err", "p_outlier", "w_outlier")
# the fixture's model: v ~ 1 + cov + C(cond) (identity), a ~ 1 + cov (exp),
# t ~ 1 + cov (exp); columns 0-3, 4-5, 6-7 of the design matrix
MODEL = [("v", 0, 4, "identity"), ("a", 4, 2, "exp"), ("t", 6, 2, "exp")]
COEF = np.array([0.7, 0.45, -0.3, 0.25, 0.55, 0.08, -1.3, 0.1])
SIZES = (1, 255, 256, 257, 231)  # around the 256-trial scoring and sum blocks


def cr_exp(x):
    """exp(x) with decimal at 60 digits, rounded to double once."""
    with decimal.localcontext(decimal.Context(prec=60)):
        return float(decimal.Decimal(x).exp())


def restate_pred(X, b, col0, ncol, link):
    """The predictor's contract in plain Python floats: one product and one
    sum per column, left to right; then the link."""
    out = np.empty(X.shape[0])
    for i in range(X.shape[0]):
        eta = float(X[i, col0]) * float(b[col0])
        for c in range(1, ncol):
            prod = float(X[i, col0 + c]) * float(b[col0 + c])
            eta = eta + prod
        if link == "exp":
            eta = cr_exp(eta)
        elif link == "invlogit":
            eta = 1.0 / (1.0 + cr_exp(-eta))
        out[i] = eta
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    """1000 trials in five groups of sizes 1, 255, 256, 257, 231 (ids shuffled
    over the trials). Trial 0 is 999, trial 1 is -999 (missing responses) and
    trial 2 lies at half its predicted t (zero density without outliers)."""
    rng = np.random.default_rng(20240611)
    n = sum(SIZES)
    group = np.repeat(np.arange(len(SIZES), dtype=np.int32), SIZES)
    rng.shuffle(group)
    cov = rng.normal(size=n)
    cond = rng.integers(0, 3, size=n)
    X = np.column_stack([np.ones(n), cov, cond == 1, cond == 2, np.ones(n), cov, np.ones(n),
                         cov]).astype(np.float64)
    t = restate_pred(X, COEF, 6, 2, "exp")
    rt = (t + 0.05 + rng.gamma(2.0, 0.25, size=n)) * rng.choice([-1.0, 1.0], size=n,
                                                                p=[0.25, 0.75])
    rt[0], rt[1], rt[2] = 999.0, -999.0, 0.5 * t[2]
    for a in (rt, X, group):
        a.setflags(write=False)
    return rt, X, group


def reg_args(F, v=0.0, a=0.0, t=0.0):
    """Positional v, sv, a, z, sz, t, st, err of wiener_like_reg."""
    return (v, F["sv"], a, F["z"], F["sz"], t, F["st"], F["err"])


def reg_kw(F):
    return {k: F[k] for k in KNOB}


def oracle_multi(oracle, rt, pred, F, multi):
    vals = dict(v=0.0, sv=F["sv"], a=0.0, z=F["z"], sz=F["sz"], t=0.0, st=F["st"])
    vals.update({k: pred[k] for k in multi})
    return oracle.wiener_like_multi(
        rt, *[vals[k] for k in ("v", "sv", "a", "z", "sz", "t", "st")], F["err"], multi=multi,
        **reg_kw(F), terms=True)


# ---------------------------------------------------------------------------
# CPU tests

def test_reg_signatures():
    from hddm_amd import wfpt
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(wfpt.RegDataset.__init__)[1:] == [
        ("rt", E), ("design", E), ("group_id", None), ("n_groups", None), ("device", None),
        ("ctx", None)]
    assert sig(wfpt.RegDataset.wiener_like_reg)[1:] == [
        ("model", E), ("coef", E), ("v", E), ("sv", E), ("a", E), ("z", E), ("sz", E), ("t", E),
        ("st", E), ("err", E), ("n_st", 10), ("n_sz", 10), ("use_adaptive", 1),
        ("simps_err", 1e-3), ("p_outlier", 0), ("w_outlier", 0), ("terms", False)]
    # after coef: wiener_like_multi's order and defaults (minus x and multi)
    ref = [p for p in sig(wfpt.wiener_like_multi) if p[0] not in ("x", "multi")]
    assert sig(wfpt.RegDataset.wiener_like_reg)[3:-1] == ref
    assert sig(wfpt.RegDataset.wiener_like_reg_groups)[1:] == [
        ("model", E), ("coef_table", E), ("params", E), ("err", 1e-4), ("n_st", 2), ("n_sz", 2),
        ("use_adaptive", 1), ("simps_err", 1e-3), ("w_outlier", 0.1), ("terms", False)]
    for name in ("close", "__len__", "__del__"):
        assert hasattr(wfpt.RegDataset, name)


def test_reg_shape_errors_without_gpu():
    from hddm_amd import wfpt
    with pytest.raises(ValueError):
        wfpt.RegDataset(np.ones(3), np.ones(3))  # 1-D design
    with pytest.raises(ValueError):
        wfpt.RegDataset(np.ones(3), np.ones((4, 2)))  # rows != trials
    with pytest.raises(ValueError):
        wfpt.RegDataset(np.ones(3), np.ones((3, 0)))  # no columns
    with pytest.raises(ValueError):
        wfpt.RegDataset(np.ones(3), np.ones((3, 2)), group_id=[0, 1])  # ids != trials
    with pytest.raises(ValueError):
        wfpt.RegDataset(np.ones(3), np.ones((3, 2)), group_id=[0, 1, 5], n_groups=2)
    # the term list is checked before any device work
    for bad in ([("q", 0, 1, "identity")], [("v", 0, 1, "identity"), ("v", 1, 1, "identity")],
                [("v", 0, 0, "identity")], [("v", 1, 2, "identity")], [("v", -1, 1, "identity")],
                [("v", 0, 1, "log")], [("v", 0, 1)]):
        with pytest.raises(ValueError):
            wfpt._reg_terms(bad, 2)
    T, nt = wfpt._reg_terms([("t", 1, 1, "exp"), ("sz", 0, 2, "invlogit")], 2)
    assert nt == 2 and (T[0].param, T[0].link, T[0].col0, T[0].ncol) == (5, 1, 1, 1)
    assert (T[1].param, T[1].link, T[1].col0, T[1].ncol) == (4, 2, 0, 2)


def test_reg_entry_points_reject_bad_arguments_without_gpu():
    """Every regression entry point validates before touching a device:
    WFPT_ERR_ARG with a message for null pointers and for invalid terms."""
    from hddm_amd import _lib
    two = 2
    assert _lib.wfpt_reg_dataset_create(None, None, 0, None, 1, None, 0, None) == two
    assert b"null" in _lib.wfpt_last_error()
    _lib.wfpt_reg_dataset_destroy(None)
    good = (_lib.RegTerm * 1)(_lib.RegTerm(0, 0, 0, 1))
    calls = ((_lib.wfpt_wiener_like_reg, ()), (_lib.wfpt_wiener_like_reg_ex, (None, None)),
             (_lib.wfpt_wiener_like_reg_groups, ()),
             (_lib.wfpt_wiener_like_reg_groups_ex, (None, None)))
    for fn, tail in calls:
        assert fn(None, None, None, 1, None, None, None, None, *tail) == two
        assert b"null" in _lib.wfpt_last_error()
        assert fn(None, None, good, 1, None, None, None, None, *tail) == two
        assert b"null" in _lib.wfpt_last_error()
        for term, word in ((_lib.RegTerm(7, 0, 0, 1), b"outside 0..6"),
                           (_lib.RegTerm(-1, 0, 0, 1), b"outside 0..6"),
                           (_lib.RegTerm(0, 0, 0, 0), b"ncol < 1"),
                           (_lib.RegTerm(0, 0, -1, 1), b"column range"),
                           (_lib.RegTerm(0, 3, 0, 1), b"link")):
            bad = (_lib.RegTerm * 1)(term)
            assert fn(None, None, bad, 1, None, None, None, None, *tail) == two
            assert word in _lib.wfpt_last_error(), (term.param, _lib.wfpt_last_error())
        twice = (_lib.RegTerm * 2)(_lib.RegTerm(2, 0, 0, 1), _lib.RegTerm(2, 0, 1, 1))
        assert fn(None, None, twice, 2, None, None, None, None, *tail) == two
        assert b"twice" in _lib.wfpt_last_error()
        assert fn(None, None, good, 8, None, None, None, None, *tail) == two


def test_fixture_terms_are_finite_on_the_oracle(oracle_lib):
    """What the GPU tests rely on: with p_outlier = 0.05 every one of the 1000
    terms is finite (both families); with p_outlier = 0 exactly trial 2 is
    -inf."""
    rt, X, _ = fixture()
    pred = {m[0]: restate_pred(X, COEF, m[1], m[2], m[3]) for m in MODEL}
    for fam in ("simple", "full"):
        _, terms = oracle_multi(oracle_lib, rt, pred, FAMILIES[fam], ["v", "a", "t"])
        assert np.all(np.isfinite(terms)), fam
    F = dict(FAMILIES["simple"], p_outlier=0.0)
    _, terms = oracle_multi(oracle_lib, rt, pred, F, ["v", "a", "t"])
    assert np.flatnonzero(~np.isfinite(terms)).tolist() == [2] and terms[2] == -np.inf


# ---------------------------------------------------------------------------
# GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize("grouped", [False, True])
def test_predictor_bits(gpu, grouped):
    rt, X, group = fixture()
    n = 300  # more than one block, not a multiple of it
    gid = group[:n] if grouped else None
    F = FAMILIES["simple"]
    # the 8-column model, all three links
    model = [("v", 0, 4, "identity"), ("a", 4, 2, "exp"), ("z", 6, 2, "invlogit")]
    coef = COEF.copy()
    coef[6:] = (0.2, -0.4)
    ds = gpu.RegDataset(rt[:n], X[:n], group_id=gid, n_groups=5 if grouped else None)
    _, _, pred = ds.wiener_like_reg(model, coef, *reg_args(F, t=0.1), **reg_kw(F), terms=True)
    for name, c0, nc, link in model:
        assert np.array_equal(pred[name], restate_pred(X[:n], coef, c0, nc, link)), name
    # per-group coefficient rows that differ
    G = ds.n_groups
    table = coef[None, :] * (1.0 + 0.07 * np.arange(G))[:, None]
    params = np.tile([0.0, F["sv"], 0.0, 0.5, F["sz"], 0.1, F["st"], 0.05], (G, 1))
    _, _, pred = ds.wiener_like_reg_groups(model, table, params, terms=True)
    rows = group[:n] if grouped else np.zeros(n, dtype=np.int64)
    for name, c0, nc, link in model:
        want = np.empty(n)
        for g in range(G):
            sel = rows == g
            want[sel] = restate_pred(X[:n][sel], table[g], c0, nc, link)
        assert np.array_equal(pred[name], want), name
    ds.close()
    # C = 1
    x1 = np.ascontiguousarray(X[:n, 1:2])
    ds = gpu.RegDataset(rt[:n], x1, group_id=gid, n_groups=5 if grouped else None)
    for link in ("identity", "exp", "invlogit"):
        _, _, pred = ds.wiener_like_reg([("v", 0, 1, link)], [0.45], *reg_args(F, a=1.8, t=0.1),
                                        **reg_kw(F), terms=True)
        assert np.array_equal(pred["v"], restate_pred(x1, [0.45], 0, 1, link)), link
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["simple", "full", "fixed"])
def test_reg_terms_and_totals(gpu, oracle_lib, family):
    rt, X, group = fixture()
    F = FAMILIES[family]
    ds = gpu.RegDataset(rt, X, group_id=group, n_groups=5)
    total, terms, pred = ds.wiener_like_reg(MODEL, COEF, *reg_args(F), **reg_kw(F), terms=True)
    _, want = oracle_multi(oracle_lib, rt, pred, F, ["v", "a", "t"])
    d = float(np.max(np.abs(terms - want)))
    ref_total = math.fsum(want)
    print(f"{family}: max|dlogp|={d:.3e} total={total!r} fsum={ref_total!r}")
    assert np.all(np.isfinite(want))  # the +-999 trials and trial 2 take part
    assert d < 1e-6
    assert abs(total - ref_total) < 1e-9 * abs(ref_total)
    assert ds.wiener_like_reg(MODEL, COEF, *reg_args(F), **reg_kw(F)) == total
    ds.close()


@pytest.mark.gpu
def test_reg_regressed_st_takes_the_generic_path(gpu, oracle_lib):
    rt, X, group = fixture()
    F = FAMILIES["full"]
    # st ~ 1 + cov through invlogit: invlogit(-3 + 0.1 cov), about 0.05
    Xw = np.ascontiguousarray(np.column_stack([X, np.ones(len(rt)), X[:, 1]]))
    model = MODEL + [("st", 8, 2, "invlogit")]
    coef = np.append(COEF, [-3.0, 0.1])
    ds = gpu.RegDataset(rt, Xw, group_id=group, n_groups=5)
    total, terms, pred = ds.wiener_like_reg(model, coef, *reg_args(F), **reg_kw(F), terms=True)
    assert np.array_equal(pred["st"], restate_pred(Xw, coef, 8, 2, "invlogit"))
    _, want = oracle_multi(oracle_lib, rt, pred, F, ["v", "a", "t", "st"])
    d = float(np.max(np.abs(terms - want)))
    ref_total = math.fsum(want)
    print(f"st regressed: max|dlogp|={d:.3e} total={total!r} fsum={ref_total!r}")
    assert d < 1e-6
    assert abs(total - ref_total) < 1e-9 * abs(ref_total)
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["simple", "full", "fixed"])
def test_reg_same_bits_as_the_per_trial_parameter_pass(gpu, family):
    """Ungrouped: sum and terms are those of Dataset.wiener_like_multi given
    the same predicted arrays."""
    rt, X, _ = fixture()
    F = FAMILIES[family]
    ds = gpu.RegDataset(rt, X)
    total, terms, pred = ds.wiener_like_reg(MODEL, COEF, *reg_args(F), **reg_kw(F), terms=True)
    plain = gpu.Dataset(rt, input_order=True)
    want, want_terms = plain.wiener_like_multi(
        pred["v"], F["sv"], pred["a"], F["z"], F["sz"], pred["t"], F["st"], F["err"],
        multi=["v", "a", "t"], **reg_kw(F), trials=True)
    assert total == want
    assert np.array_equal(terms, want_terms)
    ds.close()
    plain.close()


def _group_tables(G, F, two_pairs):
    table = COEF[None, :] * (1.0 + 0.03 * np.arange(G))[:, None]
    params = np.tile([0.3, F["sv"], 1.7, 0.5, F["sz"], 0.2, F["st"], F["p_outlier"]], (G, 1))
    params[:, 1] = F["sv"] + 0.01 * np.arange(G)
    params[:, 3] = 0.5 - 0.01 * np.arange(G)
    if two_pairs:  # groups 2.. take another (sz, st): two runs
        params[2:, 4] = F["sz"] + 0.05
        params[2:, 6] = F["st"] + 0.02
    return table, params


@pytest.mark.gpu
@pytest.mark.parametrize("family,two_pairs", [("simple", False), ("full", False), ("full", True),
                                               ("fixed", False)])
def test_reg_group_sums(gpu, family, two_pairs):
    """Row g of the groups call is bit for bit the single call on group g's
    trials alone with row g; the added empty sixth group sums to 0.0."""
    rt, X, group = fixture()
    F = FAMILIES[family]
    G = 6
    ds = gpu.RegDataset(rt, X, group_id=group, n_groups=G)
    table, params = _group_tables(G, F, two_pairs)
    kw = {k: F[k] for k in ("err", "n_st", "n_sz", "use_adaptive", "simps_err", "w_outlier")}
    sums, terms, _ = ds.wiener_like_reg_groups(MODEL, table, params, **kw, terms=True)
    assert sums.shape == (G,) and sums[5] == 0.0
    for g in range(5):
        sel = group == g
        assert int(sel.sum()) == SIZES[g]
        one = gpu.RegDataset(rt[sel], X[sel])
        v, sv, a, z, sz, t, st, po = params[g]
        want, want_terms, _ = one.wiener_like_reg(MODEL, table[g], v, sv, a, z, sz, t, st,
                                                  F["err"], **dict(reg_kw(F), p_outlier=po),
                                                  terms=True)
        assert sums[g] == want, (g, sums[g], want)
        assert np.array_equal(terms[sel], want_terms), g
        one.close()
    assert np.array_equal(ds.wiener_like_reg_groups(MODEL, table, params, **kw), sums)
    params[3, 7] = 0.1
    with pytest.raises(NotImplementedError):
        ds.wiener_like_reg_groups(MODEL, table, params, **kw)
    ds.close()


@pytest.mark.gpu
def test_reg_minus_inf_rule(gpu):
    rt, X, group = fixture()
    F = dict(FAMILIES["simple"], p_outlier=0.0)
    ds = gpu.RegDataset(rt, X, group_id=group, n_groups=5)
    total, terms, _ = ds.wiener_like_reg(MODEL, COEF, *reg_args(F), **reg_kw(F), terms=True)
    assert total == -np.inf
    assert np.flatnonzero(~np.isfinite(terms)).tolist() == [2]
    table = np.tile(COEF, (5, 1))
    params = np.tile([0.0, F["sv"], 0.0, 0.5, F["sz"], 0.0, F["st"], 0.0], (5, 1))
    sums = ds.wiener_like_reg_groups(MODEL, table, params)
    hit = int(group[2])
    assert sums[hit] == -np.inf
    assert np.all(np.isfinite(np.delete(sums, hit)))
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 257])
def test_reg_sizes(gpu, oracle_lib, n):
    rt, X, group = fixture()
    F = FAMILIES["full"]
    lo = 3  # past the missing responses and the early trial
    ds = gpu.RegDataset(rt[lo:lo + n], X[lo:lo + n])
    assert len(ds) == n
    total, terms, pred = ds.wiener_like_reg(MODEL, COEF, *reg_args(F), **reg_kw(F), terms=True)
    sums = ds.wiener_like_reg_groups(
        MODEL, COEF[None, :], [[0.0, F["sv"], 0.0, F["z"], F["sz"], 0.0, F["st"], 0.05]])
    if n == 0:
        assert total == 0.0 and sums[0] == 0.0 and terms.shape == (0,)
    else:
        _, want = oracle_multi(oracle_lib, rt[lo:lo + n], pred, F, ["v", "a", "t"])
        assert float(np.max(np.abs(terms - want))) < 1e-6
        ref_total = math.fsum(want)
        assert abs(total - ref_total) < 1e-9 * abs(ref_total)
        assert sums[0] == total
    ds.close()


@pytest.mark.gpu
def test_reg_c_entries_check_against_the_data_set(gpu):
    """The checks that need a data set, through the C ABI: a column range past
    C and a data set of another context are WFPT_ERR_ARG; the context stays
    usable."""
    from hddm_amd import _lib
    rt, X, _ = fixture()
    F = FAMILIES["simple"]
    ds = gpu.RegDataset(rt[:64], X[:64])
    P = _lib.make_params(0.0, F["sv"], 1.8, 0.5, F["sz"], 0.1, F["st"], 0.05)
    K = _lib.make_knobs(1e-4, 2, 2, 1, 1e-3, 0.1)
    out = ctypes.c_double()
    coef = np.ascontiguousarray(COEF)
    past = (_lib.RegTerm * 1)(_lib.RegTerm(0, 0, 6, 3))  # columns [6, 9) of 8
    for fn in (_lib.wfpt_wiener_like_reg, _lib.wfpt_wiener_like_reg_groups):
        assert fn(ds.ctx.handle, ds.handle, past, 1, _lib.dptr(coef), ctypes.byref(P),
                  ctypes.byref(K), ctypes.byref(out)) == 2
        assert b"column range" in _lib.wfpt_last_error()
    other = _lib.Context(ds.ctx.device)
    good = (_lib.RegTerm * 1)(_lib.RegTerm(0, 0, 0, 4))
    assert _lib.wfpt_wiener_like_reg(other.handle, ds.handle, good, 1, _lib.dptr(coef),
                                     ctypes.byref(P), ctypes.byref(K), ctypes.byref(out)) == 2
    assert b"another context" in _lib.wfpt_last_error()
    other.close()
    assert _lib.wfpt_wiener_like_reg(ds.ctx.handle, ds.handle, good, 1, _lib.dptr(coef),
                                     ctypes.byref(P), ctypes.byref(K), ctypes.byref(out)) == 0
    assert np.isfinite(out.value)
    ds.close()


@pytest.mark.gpu
def test_other_paths_unchanged_by_regression_calls(gpu):
    """A resident wiener_like, a wiener_like_multi call and an RLDataset call
    give the same bits before and after a series of regression calls on the
    same context."""
    rt, X, group = fixture()
    F = FAMILIES["full"]
    x = np.ascontiguousarray(rt[3:603])
    rng = np.random.default_rng(5)
    response = (x > 0).astype(np.int64)
    feedback = rng.integers(0, 2, x.size).astype(np.float64)
    split_by = rng.integers(0, 3, x.size).astype(np.int64)
    vs = rng.normal(1.0, 0.3, x.size)
    plain = gpu.Dataset(x)
    rl = gpu.RLDataset(x, response, feedback, split_by)

    def others():
        return (plain.wiener_like(1.1, 0.2, 1.9, 0.5, 0.1, 0.15, 0.05, 1e-4, n_st=2, n_sz=2,
                                  simps_err=1e-3, p_outlier=0.05),
                gpu.wiener_like_multi(x, vs, 0.2, 1.9, 0.5, 0.1, 0.15, 0.05, 1e-4, multi=["v"],
                                      n_st=2, n_sz=2, p_outlier=0.05, w_outlier=0.1),
                rl.wiener_like_rlddm(0.5, 0.2, 100.0, 1.5, 0.2, 1.9, 0.5, 0.1, 0.15, 0.05, 1e-4,
                                     n_st=2, n_sz=2, simps_err=1e-3, p_outlier=0.05,
                                     w_outlier=0.1))

    before = others()
    ds = gpu.RegDataset(rt, X, group_id=group, n_groups=5)
    table, params = _group_tables(5, F, True)
    for _ in range(3):
        ds.wiener_like_reg(MODEL, COEF, *reg_args(F), **reg_kw(F), terms=True)
        ds.wiener_like_reg_groups(MODEL, table, params)
    assert others() == before
    ds.close()
    assert others() == before
    plain.close()
    rl.close()
