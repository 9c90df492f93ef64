"""HDDMRegressor (hddm_amd/regression.py): the design-matrix subset, the
model's bookkeeping and priors on the CPU (RegDataset replaced by an
oracle-backed stand-in, as tests/test_hierarchical.py does for Dataset), and
parameter recovery on the GPU."""
import math

import numpy as np
import pytest
from scipy import stats


# ---------------------------------------------------------------- design_matrix

def _frame():
    import pandas as pd
    return pd.DataFrame({"x": [0.5, -1.0, 2.0, 0.25, 1.5],
                         "c": ["b", "a", "c", "a", "b"],
                         "y": [1.0, 2.0, 3.0, 4.0, 5.0]})


def test_design_matrix_numeric():
    from hddm_amd.regression import design_matrix
    d = _frame()
    for rhs in ("1 + x", "x"):
        X = design_matrix(rhs, d)
        assert list(X.columns) == ["Intercept", "x"]
        assert np.array_equal(X.to_numpy(), np.column_stack([np.ones(5), d["x"]]))
    X = design_matrix("0 + x + y", d)
    assert list(X.columns) == ["x", "y"]
    assert np.array_equal(X.to_numpy(), d[["x", "y"]].to_numpy())
    assert X.to_numpy().dtype == np.float64


def test_design_matrix_categorical():
    from hddm_amd.regression import design_matrix
    d = _frame()
    is_a, is_b, is_c = [(d["c"] == k).to_numpy(dtype=float) for k in "abc"]
    X = design_matrix("C(c)", d)  # treatment coding over the sorted levels
    assert list(X.columns) == ["Intercept", "C(c)[T.b]", "C(c)[T.c]"]
    assert np.array_equal(X.to_numpy(), np.column_stack([np.ones(5), is_b, is_c]))
    X = design_matrix("0 + C(c)", d)  # full coding
    assert list(X.columns) == ["C(c)[a]", "C(c)[b]", "C(c)[c]"]
    assert np.array_equal(X.to_numpy(), np.column_stack([is_a, is_b, is_c]))
    X = design_matrix("x + C(c)", d)  # patsy's order: categorical terms before numeric ones
    assert list(X.columns) == ["Intercept", "C(c)[T.b]", "C(c)[T.c]", "x"]
    assert np.array_equal(X.to_numpy(), np.column_stack([np.ones(5), is_b, is_c, d["x"]]))


def test_design_matrix_interaction_needs_patsy():
    from hddm_amd.regression import design_matrix
    try:
        import patsy  # noqa: F401
    except ImportError:
        with pytest.raises(NotImplementedError, match="x:C\\(c\\)"):
            design_matrix("x:C(c)", _frame())
        with pytest.raises(NotImplementedError, match="np.log"):
            design_matrix("1 + np.log(y)", _frame())
    else:
        X = design_matrix("x:C(c)", _frame())
        assert X.shape[0] == 5


# ---------------------------------------------------------------- the model on the CPU

class _OracleRegDataset:
    """Test stand-in for hddm_amd.wfpt.RegDataset backed by the oracle (CPU)."""

    def __init__(self, rt, design, group_id=None, n_groups=None, device=None):
        import oracle
        self.o = oracle
        self.rt = np.asarray(rt, dtype=np.float64)
        self.X = np.asarray(design, dtype=np.float64)
        self.group = np.asarray(group_id)
        self.n_groups = n_groups

    def wiener_like_reg_groups(self, model, coef_table, params, err, n_st, n_sz, use_adaptive,
                               simps_err, w_outlier):
        link = {"identity": lambda e: e, "exp": np.exp, "invlogit": lambda e: 1 / (1 + np.exp(-e))}
        out = np.zeros(self.n_groups)
        for g in range(self.n_groups):
            sel = self.group == g
            if not sel.any():
                continue
            vals = dict(zip(("v", "sv", "a", "z", "sz", "t", "st"), params[g][:7]))
            for name, c0, nc, lk in model:
                eta = np.zeros(int(sel.sum()))
                for c in range(c0, c0 + nc):
                    eta = eta + self.X[sel, c] * coef_table[g][c]
                vals[name] = link[lk](eta)
            out[g] = self.o.wiener_like_multi(
                self.rt[sel], *[vals[k] for k in ("v", "sv", "a", "z", "sz", "t", "st")], err,
                multi=[m[0] for m in model], n_st=n_st, n_sz=n_sz, use_adaptive=use_adaptive,
                simps_err=simps_err, p_outlier=params[g][7], w_outlier=w_outlier)
        return out


def _cpu_data(seed=3, n_subj=4, n=40):
    import pandas as pd
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(n_subj):
        x = rng.choice([-1.0, 1.0], n, p=[0.3, 0.7]) * (0.3 + rng.gamma(2.0, 0.3, n))
        rows.append(pd.DataFrame({"rt": x, "subj_idx": s, "cov": rng.normal(size=n),
                                  "cond": rng.choice(["lo", "mid", "hi"], n)}))
    return pd.concat(rows, ignore_index=True)


MODELS = ["v ~ 1 + cov + C(cond)", {"model": "a ~ 1 + cov", "link_func": "exp"}]


@pytest.fixture
def reg(oracle_lib, monkeypatch):
    from hddm_amd import regression as r
    monkeypatch.setattr(r._wfpt, "RegDataset", _OracleRegDataset)
    return r


def test_regressor_bookkeeping_on_cpu(reg):
    m = reg.HDDMRegressor(_cpu_data(), MODELS, seed=0)
    assert m.coef_names == ["v_Intercept", "v_C(cond)[T.lo]", "v_C(cond)[T.mid]", "v_cov",
                            "a_Intercept", "a_cov"]
    assert m.coef_intercept == [True, False, False, False, True, False]
    assert m.reg_model == [("v", 0, 4, "identity"), ("a", 4, 2, "exp")]
    assert m.FAMILIES == ("t",) and m.n_nodes == 4 and m.design.shape == (160, 6)
    assert m.coef_table().shape == (4, 6) and m.node_table().shape == (4, 8)
    assert np.all(m.node_table()[:, 7] == 0.05) and np.all(m.node_table()[:, 3] == 0.5)
    # without an intercept every plain C(...) column is one (hddm_regression.py:257-260)
    m = reg.HDDMRegressor(_cpu_data(), "v ~ 0 + C(cond) + cov", seed=0)
    assert m.coef_names == ["v_C(cond)[hi]", "v_C(cond)[lo]", "v_C(cond)[mid]", "v_cov"]
    assert m.coef_intercept == [True, True, True, False]
    assert m.FAMILIES == ("a", "t")
    # depends_on of a non-regressed family: (subject x condition) nodes are the groups, a
    # subject-level coefficient reaches a node through its subject
    m = reg.HDDMRegressor(_cpu_data(), "v ~ cov", depends_on={"a": "cond"},
                          group_only_regressors=False, seed=0)
    assert m.n_nodes == 12 and m.levels["a"] == [("hi",), ("lo",), ("mid",)]
    m.coef_subj["v_cov"] = np.arange(4.0)
    assert np.array_equal(m.coef_table()[:, 1], m.node_subj.astype(float))
    assert np.array_equal(m.coef_table({"v_cov": 7.0})[:, 1], np.full(12, 7.0))
    assert np.isfinite(m.logp())


def _gamma(x, mean, sd):
    return stats.gamma.logpdf(x, mean ** 2 / sd ** 2, scale=sd ** 2 / mean)


def test_regressor_logp_matches_a_restatement(reg, oracle_lib):
    data = _cpu_data()
    m = reg.HDDMRegressor(data, MODELS, group_only_regressors=False, include=("st",), seed=0)
    rng = np.random.default_rng(1)
    S = m.n_subj
    g = {"v_Intercept": 1.1, "v_C(cond)[T.lo]": -0.2, "v_C(cond)[T.mid]": 0.1, "v_cov": 0.3,
         "a_Intercept": 0.6, "a_cov": 0.05}
    for nm in m.coef_names:
        m.coef[nm] = g[nm]
        m.coef_std[nm] = 0.2 + 0.1 * rng.uniform()
        m.coef_subj[nm] = g[nm] + 0.05 * rng.normal(size=S)
    m.group["t"][:] = 0.25
    m.std["t"] = 0.07
    m.subj["t"] = 0.2 + 0.02 * rng.uniform(size=S)
    m.inter["st"] = 0.04
    # the restatement: per subject the oracle's wiener_like_multi, priors from scipy
    import pandas as pd
    cond = data["cond"].to_numpy()
    Xv = np.column_stack([np.ones(len(data)), cond == "lo", cond == "mid", data["cov"]])
    Xa = np.column_stack([np.ones(len(data)), data["cov"]])
    want = 0.0
    for s in range(S):
        sel = (data["subj_idx"] == s).to_numpy()
        bv = np.array([m.coef_subj[nm][s] for nm in m.coef_names[:4]])
        ba = np.array([m.coef_subj[nm][s] for nm in m.coef_names[4:]])
        want += oracle_lib.wiener_like_multi(
            data["rt"].to_numpy()[sel], Xv[sel].astype(float) @ bv, 0.0,
            np.exp(Xa[sel] @ ba), 0.5, 0.0, m.subj["t"][s], 0.04, 1e-4, multi=["v", "a"],
            n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, p_outlier=0.05, w_outlier=0.1)
    want += stats.norm.logpdf(g["v_Intercept"], 2.0, 3.0)
    want += np.sum(stats.norm.logpdf(m.coef_subj["v_Intercept"], g["v_Intercept"],
                                     m.coef_std["v_Intercept"]))
    want += stats.halfnorm.logpdf(m.coef_std["v_Intercept"], scale=2.0)
    want += _gamma(g["a_Intercept"], 1.5, 0.75)
    want += np.sum(_gamma(m.coef_subj["a_Intercept"], g["a_Intercept"],
                          m.coef_std["a_Intercept"]))
    want += stats.halfnorm.logpdf(m.coef_std["a_Intercept"], scale=2.0)
    for nm in ("v_C(cond)[T.lo]", "v_C(cond)[T.mid]", "v_cov", "a_cov"):
        want += stats.norm.logpdf(g[nm], 0.0, 15.0)
        want += np.sum(stats.norm.logpdf(m.coef_subj[nm], g[nm], m.coef_std[nm]))
        want += stats.uniform.logpdf(m.coef_std[nm], 1e-10, 100.0 - 1e-10)
    want += _gamma(0.25, 0.4, 0.2) + np.sum(_gamma(m.subj["t"], 0.25, 0.07))
    want += stats.halfnorm.logpdf(0.07, scale=1.0)
    want += stats.halfnorm.logpdf(0.04, scale=0.3)
    got = m.logp()
    assert np.isfinite(want)
    assert abs(got - want) < 1e-9 * abs(want), (got, want)


@pytest.mark.parametrize("group_only", [True, False])
def test_regressor_short_sample_on_cpu(reg, group_only):
    m = reg.HDDMRegressor(_cpu_data(), MODELS, group_only_regressors=group_only, seed=0)
    tr = m.sample(6, burn=2)
    want = set(m.coef_names) | {"t", "t_std"}
    if not group_only:
        want |= {nm + "_std" for nm in m.coef_names}
    assert set(tr) == want
    for k, v in tr.items():
        assert v.shape == (4,) and np.all(np.isfinite(v)), k
    assert m.trace_subj["t"].shape == (4, 4)
    if not group_only:
        assert m.trace_subj["v_cov"].shape == (4, 4)
    assert np.isfinite(m.logp())
    assert m.likelihood_calls > 6 and sum(c for c, _ in m.call_stats.values()) == \
        m.likelihood_calls
    assert set(m.gen_stats()["v_cov"]) == {"mean", "std", "2.5q", "97.5q"}


def test_regressor_refusals(reg):
    data = _cpu_data()
    with pytest.raises(TypeError, match="device.*identity.*exp.*invlogit"):
        reg.HDDMRegressor(data, {"model": "v ~ cov", "link_func": lambda x: x})
    with pytest.raises(ValueError, match="depends_on"):
        reg.HDDMRegressor(data, "v ~ cov", depends_on={"v": "cond"})
    with pytest.raises(NotImplementedError, match="'z'"):
        reg.HDDMRegressor(data, "z ~ cov")
    with pytest.raises(ValueError):
        reg.HDDMRegressor(data, {"model": "v ~ cov", "link_func": "log"})


# ---------------------------------------------------------------- recovery on the GPU

def _simulate(n_subj=12, n_trials=200, seed=7, dt=1e-3):
    """Euler walks of the DDM with the trial's drift v = 1.0 + 0.8 cov; a and t
    jittered by +-10% per subject as hierarchical.gen_data does."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    rows, a_true, t_true = [], [], []
    for s in range(n_subj):
        a = 2.0 * (1 + 0.1 * rng.uniform(-1, 1))
        t = 0.3 * (1 + 0.1 * rng.uniform(-1, 1))
        cov = rng.normal(size=n_trials)
        v = 1.0 + 0.8 * cov
        pos = np.full(n_trials, 0.5 * a)
        rt = np.zeros(n_trials)
        live = np.ones(n_trials, dtype=bool)
        k = 0
        while live.any():
            k += 1
            pos[live] += v[live] * dt + math.sqrt(dt) * rng.normal(size=int(live.sum()))
            hit = live & ((pos >= a) | (pos <= 0))
            rt[hit] = np.where(pos[hit] >= a, 1.0, -1.0) * (t + k * dt)
            live &= ~hit
        rows.append(pd.DataFrame({"rt": rt, "subj_idx": s, "cov": cov}))
        a_true.append(a)
        t_true.append(t)
    return pd.concat(rows, ignore_index=True), float(np.mean(a_true)), float(np.mean(t_true))


@pytest.mark.gpu
def test_regressor_recovers_the_slope(gpu):
    """12 subjects x 200 trials, v = 1.0 + 0.8 cov: the bars of
    tests/test_hierarchical.py::test_parameter_recovery_small_model for a drift
    level (0.35), a (0.25) and t (0.05) at this size."""
    from hddm_amd.regression import HDDMRegressor
    data, a_true, t_true = _simulate()
    m = HDDMRegressor(data, "v ~ cov", seed=1)
    assert m.coef_names == ["v_Intercept", "v_cov"]
    m.sample(150, burn=50)
    st = m.gen_stats()
    print({k: (round(v["mean"], 4), round(v["2.5q"], 4), round(v["97.5q"], 4))
           for k, v in st.items()}, m.likelihood_calls, round(m.sample_seconds, 2))
    assert abs(st["v_cov"]["mean"] - 0.8) < 0.35
    assert st["v_cov"]["2.5q"] > 0 or st["v_cov"]["97.5q"] < 0
    assert abs(st["a"]["mean"] - a_true) < 0.25
    assert abs(st["t"]["mean"] - t_true) < 0.05
