"""HDDM.optimize: 'ML', 'chisquare' and 'gsquare' point fits and the lockstep
bootstrap (hddm/models/base.py:47-308; the reference's own checks are
hddm/tests/test_optimization.py).

Recovery bars are the reference's: every fitted parameter within 0.1 of the
generating value for one subject started at the truth (test_optimization.py:91).
The fitted model is the one that generated the data: gen_data draws no
outliers, so the models here have p_outlier = 0. With the class default of 0.05
the fit is that of a misspecified model, a 5 % uniform contaminant over 10 s on
clean data: measured with the oracle's CDF on four simulated sets of 2 x 1000
trials it puts the estimate of the larger drift off by +0.05 .. +0.16, against
-0.05 .. +0.06 at p_outlier = 0.
The group model's data jitter every subject's parameters by +-10 % around the
group values, and its fit pools the subjects' quantiles (the average model), so
its bar is 0.15.
"""
import numpy as np
import pytest

GROUP_MEANS = {"a": 2.0, "t": 0.3, "v(c0)": 0.5, "v(c1)": 1.5}


# ---------------------------------------------------------------- CPU tests

def _frame(n_subj, n=40):
    import pandas as pd
    rng = np.random.default_rng(0)
    rt = (0.3 + rng.gamma(2.0, 0.2, n_subj * n)) * rng.choice([-1.0, 1.0], n_subj * n)
    return pd.DataFrame({"rt": rt, "subj_idx": np.repeat(np.arange(n_subj), n),
                         "cond": np.tile(["c0", "c1"], n_subj * n // 2)})


class _NoDevice:
    """The model without its resident data: the argument checks come first."""

    @staticmethod
    def build(n_subj):
        from hddm_amd.hierarchical import HDDM

        class Model(HDDM):
            def _make_dataset(self, rt, node_codes, device):
                return None
        return Model(_frame(n_subj), depends_on={"v": "cond"}, seed=1)


def test_ml_on_a_group_model_raises_type_error():
    m = _NoDevice.build(3)
    with pytest.raises(TypeError, match="not defined for group models"):
        m.optimize("ML")


def test_unknown_method_raises_value_error():
    for n_subj in (1, 3):
        with pytest.raises(ValueError):
            _NoDevice.build(n_subj).optimize("least-squares")
    with pytest.raises(NotImplementedError):
        _NoDevice.build(1).optimize("ML", n_bootstraps=4)


def test_chains_and_regressor_have_no_point_fit():
    from hddm_amd.hierarchical import HDDMChains
    from hddm_amd.regression import HDDMRegressor
    for cls in (HDDMChains, HDDMRegressor):
        with pytest.raises(NotImplementedError):
            cls.optimize(object.__new__(cls), "gsquare")


def test_set_values_by_group_node_name():
    m = _NoDevice.build(1)
    m.set_values({"a": 1.7, "v(c1)": 0.9, "t": 0.25})
    assert m.group["a"][0] == 1.7 and m.subj["a"][0] == 1.7
    assert m.group["v"][1] == 0.9 and m.subj["v"][1] == 0.9 and m.group["v"][0] == 2.0
    g = _NoDevice.build(3)
    before = g.subj["v"].copy()
    g.set_values({"v(c0)": 0.4})
    assert g.group["v"][0] == 0.4 and np.array_equal(g.subj["v"], before)
    with pytest.raises(KeyError):
        m.set_values({"sv": 1.0})  # not included


CENTRES = np.array([[1.0, -2.0, 0.5], [0.1, 0.2, 0.3], [-3.0, 1.5, 2.5], [4.0, 4.0, -4.0],
                    [0.7, -0.7, 7.0], [-1.0, -1.0, -1.0], [2.5, 0.0, -0.25]])
SCALES = np.array([[1.0, 2.0, 3.0], [0.5, 0.5, 0.5], [3.0, 1.0, 2.0], [1.0, 1.0, 1.0],
                   [2.0, 4.0, 0.5], [1.5, 2.5, 3.5], [0.25, 1.0, 4.0]])


def _bowls(X, idx):
    return np.sum(SCALES[idx] * (X - CENTRES[idx]) ** 2, axis=1) + 0.5 * idx


def test_lockstep_minimize_bowls():
    """7 shifted quadratic bowls in 3 dimensions: each minimum to 1e-6, and each
    problem's run bit-identical to the same problem minimised alone."""
    from hddm_amd.optimize import _lockstep_minimize
    x0 = np.tile([0.3, -0.2, 0.1], (7, 1)) + 0.1 * np.arange(7)[:, None]
    calls = []

    def counted(X, idx):
        calls.append(len(idx))
        return _bowls(X, idx)

    x, f, it, ev = _lockstep_minimize(counted, x0, xtol=1e-9, ftol=1e-16, maxiter=2000)
    assert np.abs(x - CENTRES).max() < 1e-6, np.abs(x - CENTRES).max()
    assert np.allclose(f, 0.5 * np.arange(7), atol=1e-11)
    assert np.all(it < 2000) and len(set(it)) > 1  # they stop at different iterations
    assert sum(calls) == ev.sum()
    for b in range(7):
        xb, fb, itb, evb = _lockstep_minimize(
            lambda X, idx, b=b: _bowls(X, np.full(len(idx), b)), x0[b:b + 1], xtol=1e-9,
            ftol=1e-16, maxiter=2000)
        assert np.array_equal(xb[0], x[b]) and fb[0] == f[b] and itb[0] == it[b] \
            and evb[0] == ev[b], b


# ---------------------------------------------------------------- GPU tests

@pytest.fixture(scope="module")
def single():
    from hddm_amd.hierarchical import gen_data
    data, tr = gen_data(n_subj=1, n_trials=2000, conds={"c0": 0.5, "c1": 1.5}, a=2.0, t=0.3,
                        seed=20261020)
    # the subject's own generating values (gen_data jitters them around a, t and the drifts)
    truth = {"a": tr["a"][0], "t": tr["t"][0], "v(c0)": tr["v"]["c0"][0],
             "v(c1)": tr["v"]["c1"][0]}
    return data, truth


def _model(data, start):
    """The model started at `start`, as the reference's tests start at the truth."""
    from hddm_amd.hierarchical import HDDM
    m = HDDM(data, depends_on={"v": "cond"}, seed=3, p_outlier=0.0)
    m.set_values(start)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["chisquare", "gsquare", "ML"])
def test_single_subject_recovery(single, method):
    data, truth = single
    m = _model(data, truth)
    res = m.optimize(method)
    print(method, res, truth)
    assert sorted(res) == sorted(truth)
    for k, v in truth.items():
        assert abs(res[k] - v) < 0.1, (method, k, res[k])
    # the fit became the model's values
    assert m.group["a"][0] == res["a"] and m.subj["v"][1] == res["v(c1)"]
    if method == "gsquare":
        b = m.bic_info
        assert b["penalty"] == 4 * np.log(2000)
        assert b["bic"] == -b["likelihood"] + b["penalty"]
        assert b["likelihood"] == -m.quantile_objective("gsquare")
    else:
        assert not hasattr(m, "bic_info")


@pytest.mark.gpu
def test_chisquare_objective_is_the_sum_of_node_statistics(single):
    """At the fitted values the objective equals, bit for bit, the sum over the
    nodes of the host reduction of dmat_cdf_array at the node's edges."""
    from test_cdf_rows import _reduce
    from hddm_amd import cdfdif_wrapper as cw
    from hddm_amd.quantiles import quantile_stats
    data, truth = single
    m = _model(data, truth)
    res = m.optimize("chisquare", n_runs=1)
    rt = data["rt"].to_numpy()
    total = 0.0
    for c in ("c0", "c1"):
        s = quantile_stats(rt[(data["cond"] == c).to_numpy()])
        cdf = cw.dmat_cdf_array(s["emp_rt"], res[f"v({c})"], 0.0, res["a"], 0.5, 0.0, res["t"],
                                0.0, m.p_outlier, m.wp["w_outlier"])
        total += _reduce(cdf, s["freq_obs"], s["n_samples"])[0]
    assert m.quantile_objective("chisquare") == total
    assert np.isfinite(total) and total > 0


@pytest.mark.gpu
def test_group_model_gsquare():
    from hddm_amd.hierarchical import gen_data
    data, _ = gen_data(n_subj=8, n_trials=300, conds={"c0": 0.5, "c1": 1.5}, a=2.0, t=0.3,
                       seed=20261021)
    m = _model(data, GROUP_MEANS)
    state = {k: {n: np.array(v, copy=True) for n, v in getattr(m, k).items()}
             for k in ("group", "subj", "std", "inter")}
    res = m.optimize("gsquare")
    print(res)
    for k, v in GROUP_MEANS.items():
        assert np.isfinite(res[k]) and abs(res[k] - v) < 0.15, (k, res[k])
    for k, d in state.items():
        for n, v in d.items():
            assert np.array_equal(np.asarray(getattr(m, k)[n]), v), (k, n)
    assert set(m.bic_info) == {"likelihood", "penalty", "bic"}
    assert m.bic_info["penalty"] == 4 * np.log(2400)


@pytest.mark.gpu
def test_bootstrap(single):
    from hddm_amd.optimize import bootstrap_fits
    data, truth = single
    frames = []
    for _ in range(2):
        m = _model(data, truth)
        res = m.optimize("gsquare", n_runs=1, n_bootstraps=16, seed=11)
        frames.append(m.bootstrap_stats)
    st = frames[0]
    assert {"mean", "std", "2.5%", "97.5%"} <= set(st.index)
    assert sorted(st.columns) == sorted(truth)
    for k in truth:
        assert st.loc["min", k] <= res[k] <= st.loc["max", k], (k, res[k], st[k])
        assert st.loc["2.5%", k] <= st.loc["97.5%", k]
    assert st.loc["count"].eq(16).all()
    assert frames[0].equals(frames[1])
    assert np.array_equal(frames[0].to_numpy(), frames[1].to_numpy())
    # replicate 0 alone (B = 1) is its row of the batch
    x0 = np.array([res[k] for k in m.bootstrap_values.columns])
    alone = bootstrap_fits(m, "gsquare", (.1, .3, .5, .7, .9), x0, m.bootstrap_seed, [0])
    assert np.array_equal(alone[0], m.bootstrap_values.to_numpy()[0])
