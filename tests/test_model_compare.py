"""Model comparison at the model layer (hddm_amd/compare.py): dic_info, waic
and compare.

CPU: the arithmetic on hand-made pointwise dicts through a stand-in model that
states the three things compare.Pointwise asks of a sampler. GPU: HDDM, HDDMrl
and HDDMRegressor after a short fit, dic_info against the formula evaluated
from one node_logp call per kept sweep, waic's lppd against numpy on the
per-trial terms of the existing calls.
"""
import math

import numpy as np
import pytest
from scipy.special import logsumexp

from hddm_amd import compare
from hddm_amd.hierarchical import HDDM, HDDMChains


class _Model(compare.Pointwise):
    """A sampler reduced to what Pointwise needs: S kept sweeps of `terms`
    (S, n) in `nodes` equal parts."""
    _picked_sweeps = staticmethod(HDDM._picked_sweeps)

    def __init__(self, terms, mean_terms, nodes=2, trial=None):
        self.terms = np.asarray(terms, dtype=np.float64)
        self.mean_terms = np.asarray(mean_terms, dtype=np.float64)
        self.nodes = nodes
        self.trial = np.arange(self.terms.shape[1]) if trial is None else np.asarray(trial)
        self.trace = {"a": np.zeros(self.terms.shape[0])}
        self.trace_subj = {}
        self.calls = 0

    def _node_sums(self, t):
        return np.stack([p.sum(axis=-1) for p in np.array_split(t, self.nodes, axis=-1)], axis=-1)

    def _pw_score(self, picked):
        self.calls += 1
        t = self.terms[picked]
        lppd, p = np.empty(t.shape[1]), np.empty(t.shape[1])
        for i, col in enumerate(t.T):
            fin = col[np.isfinite(col)]
            lppd[i] = logsumexp(fin) - math.log(col.size) if fin.size else -np.inf
            p[i] = np.var(fin, ddof=1) if fin.size >= 2 else (0.0 if fin.size else np.nan)
        return {"sums": self._node_sums(t), "lppd": lppd, "p_waic": p, "mean": lppd.copy(),
                "n_inf": np.sum(t == -np.inf, axis=0), "trial": self.trial,
                "n_inf_total": int(np.sum(t == -np.inf))}

    def _pw_mean_logp(self, picked):
        return self._node_sums(self.mean_terms)


TERMS = np.array([[-1.0, -2.0, -0.5, -3.0],
                  [-1.5, -1.0, -0.5, -2.0],
                  [-0.5, -3.0, -0.5, -4.0]])


def test_dic_info_arithmetic():
    m = _Model(TERMS, [-0.9, -1.8, -0.5, -2.9])
    info = m.dic_info()
    D = [-2 * -6.5, -2 * -5.0, -2 * -8.0]
    deviance = sum(D) / 3
    d_hat = -2 * -(0.9 + 1.8 + 0.5 + 2.9)
    assert info["deviance"] == pytest.approx(deviance, rel=1e-15)
    assert info["pD"] == pytest.approx(deviance - d_hat, rel=1e-14)
    assert info["DIC"] == pytest.approx(2 * deviance - d_hat, rel=1e-14)
    assert m.dic == info["DIC"]
    assert set(info) == {"DIC", "deviance", "pD"}


def test_waic_arithmetic():
    m = _Model(TERMS, TERMS[0])
    w = m.waic()
    lppd_i = logsumexp(TERMS, axis=0) - math.log(3)
    p_i = np.var(TERMS, axis=0, ddof=1)
    elpd_i = lppd_i - p_i
    assert np.allclose(w["elpd"], elpd_i, rtol=1e-15, atol=0)
    assert w["elpd_waic"] == math.fsum(elpd_i) and w["waic"] == -2 * w["elpd_waic"]
    assert w["p_waic"] == math.fsum(p_i) and w["lppd"] == math.fsum(lppd_i)
    assert w["se"] == pytest.approx(2 * math.sqrt(4 * np.var(elpd_i)), rel=1e-14)
    assert w["n_trials"] == 4 and w["n_inf"] == 0
    assert w["n_high_var"] == int(np.sum(p_i > 0.4)) == 2
    assert np.array_equal(w["trial"], np.arange(4))


def test_constant_terms_have_no_penalty():
    """Terms that do not vary over the sweeps: pD == 0 and p_waic == 0 exactly."""
    row = np.array([-0.3, -7.25, -123.5, -1.0])
    m = _Model(np.tile(row, (8, 1)), row)
    info, w = m.dic_info(), m.waic()
    assert info["pD"] == 0.0 and info["DIC"] == info["deviance"] == -2 * row.sum()
    assert w["p_waic"] == 0.0 and w["n_high_var"] == 0 and w["se"] > 0


def test_waic_with_zero_densities():
    t = TERMS.copy()
    t[1, 0] = -np.inf
    w = _Model(t, TERMS[0]).waic()
    assert w["n_inf"] == 1 and np.isfinite(w["waic"])
    t[:, 3] = -np.inf  # a trial no sweep gives a density: waic is inf, not an exception
    w = _Model(t, TERMS[0]).waic()
    assert w["waic"] == np.inf and w["elpd_waic"] == -np.inf and w["n_inf"] == 4
    assert w["elpd"][3] == -np.inf and np.isfinite(w["elpd"][:3]).all()
    assert np.isfinite(w["p_waic"]) and np.isnan(w["se"])


def test_pointwise_is_cached_per_trace_and_samples():
    m = _Model(TERMS, TERMS[0])
    a = m.pointwise_loglik()
    assert m.pointwise_loglik() is a and m.calls == 1
    m.waic(), m.dic_info()
    assert m.calls == 1 and np.array_equal(a["picked"], [0, 1, 2])
    b = m.pointwise_loglik(samples=2)
    assert m.calls == 2 and np.array_equal(b["picked"], [0, 2]) and b["sums"].shape == (2, 2)
    m.trace = dict(m.trace)  # a new sample() makes new traces
    assert m.pointwise_loglik(samples=2) is not b and m.calls == 3
    empty = _Model(TERMS, TERMS[0])
    del empty.trace
    with pytest.raises(RuntimeError, match="sample"):
        empty.waic()


def test_compare_ranks_by_waic():
    good = _Model(TERMS, TERMS[0])
    bad = _Model(TERMS - np.array([0.5, 0.1, 1.0, 0.2]), TERMS[0] - 0.4)
    other = _Model(TERMS[:, :3] - 2.0, TERMS[0, :3] - 2.0, nodes=1, trial=[0, 1, 5])
    table = compare.compare({"bad": bad, "other": other, "good": good})
    assert list(table.columns) == ["waic", "p_waic", "d_waic", "dse", "dic", "pD"]
    assert list(table.index) == sorted(table.index, key=lambda k: table.loc[k, "waic"])
    assert table.index[0] == "good" and table.loc["good", "d_waic"] == 0
    assert table.loc["good", "dse"] == 0
    wg, wb = good.waic(), bad.waic()
    assert table.loc["bad", "d_waic"] == wb["waic"] - wg["waic"] > 0
    diff = wg["elpd"] - wb["elpd"]
    assert table.loc["bad", "dse"] == pytest.approx(2 * math.sqrt(4 * np.var(diff)), rel=1e-14)
    assert np.isnan(table.loc["other", "dse"])  # scored on other trials
    assert table.loc["bad", "dic"] == bad.dic and table.loc["bad", "pD"] == bad.dic_info()["pD"]
    with pytest.raises(ValueError):
        compare.compare({})


def test_chains_refuse_model_comparison():
    for name in ("pointwise_loglik", "dic_info", "waic"):
        with pytest.raises(NotImplementedError, match="one chain"):
            getattr(HDDMChains, name)(None)


# ---------------------------------------------------------------- GPU: fitted models

def _ddm_frame(n_subj, n_trials, seed, conds=("c0", "c1")):
    import pandas as pd
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(n_subj):
        x = rng.choice([-1.0, 1.0], n_trials, p=[0.3, 0.7]) * (0.3 + rng.gamma(2.0, 0.3, n_trials))
        rows.append(pd.DataFrame({"rt": x, "subj_idx": s, "cov": rng.normal(size=n_trials),
                                  "cond": rng.choice(list(conds), n_trials)}))
    return pd.concat(rows, ignore_index=True).sample(frac=1.0, random_state=1).reset_index(
        drop=True)


def _check_model(m, sweep_over, mean_over, sweep_terms):
    """dic_info against one node_logp call per kept sweep (the same addends in
    another order: 1e-9 relative), waic's lppd against numpy on the terms."""
    S = len(next(iter(m.trace.values())))
    assert S == 20
    calls = m.likelihood_calls
    info, w = m.dic_info(), m.waic()
    assert m.likelihood_calls == calls  # neither goes through the sampler's per-step calls
    D = np.array([-2.0 * np.sum(m.node_logp(sweep_over(s))) for s in range(S)])
    deviance = D.mean()
    d_hat = -2.0 * np.sum(m.node_logp(mean_over()))
    assert info["deviance"] == pytest.approx(deviance, rel=1e-9)
    assert info["pD"] == pytest.approx(deviance - d_hat, rel=1e-9)
    assert info["DIC"] == pytest.approx(2 * deviance - d_hat, rel=1e-9)
    assert m.dic == info["DIC"]
    terms = np.stack([sweep_terms(s) for s in range(S)])
    pw = m.pointwise_loglik()
    terms = terms[:, pw["trial"]]
    lppd_i = logsumexp(terms, axis=0) - math.log(S)
    assert w["lppd"] == pytest.approx(math.fsum(lppd_i), rel=1e-12)
    assert np.allclose(pw["lppd"], lppd_i, rtol=1e-12, atol=1e-12)
    # a variance's rounding error grows with (mean / sd)^2: up to ~1e5 for a trial whose
    # term hardly moves over the sweeps, times S = 20 roundings of 1.1e-16
    assert np.allclose(pw["p_waic"], np.var(terms, axis=0, ddof=1), rtol=1e-9, atol=1e-12)
    assert w["n_trials"] == terms.shape[1] and w["n_inf"] == 0
    assert w["waic"] == pytest.approx(-2 * math.fsum(lppd_i - np.var(terms, axis=0, ddof=1)),
                                      rel=1e-9)
    few = m.pointwise_loglik(samples=5)
    assert few["sums"].shape[0] == 5 and np.array_equal(few["picked"], [0, 5, 10, 14, 19])
    return w


@pytest.mark.gpu
def test_hddm_dic_and_waic(gpu):
    m = HDDM(_ddm_frame(3, 40, 5), depends_on={"v": "cond"}, include=("sv", "st"), seed=2)
    m.sample(30, burn=10)
    fams, inter = m.FAMILIES, m.inter_names
    over = lambda s: {**{f: m.trace_subj[f][s] for f in fams},
                      **{n: float(m.trace[n][s]) for n in inter}}
    mean = lambda: {**{f: m.trace_subj[f].mean(axis=0) for f in fams},
                    **{n: float(np.mean(m.trace[n])) for n in inter}}
    terms = lambda s: m.dataset.wiener_like_nodes(m.node_table(over(s)), trials=True, **m.wp)[1]
    w = _check_model(m, over, mean, terms)
    assert w["n_trials"] == 120 and np.array_equal(w["trial"], np.arange(120))
    flat = HDDM(m.data, seed=2)
    flat.sample(30, burn=10)
    table = compare.compare({"by cond": m, "flat": flat})
    assert set(table.index) == {"by cond", "flat"} and np.isfinite(table.to_numpy()).all()
    assert table["dse"].iloc[1] > 0 and table["d_waic"].iloc[1] >= 0


@pytest.mark.gpu
def test_hddmrl_dic_and_waic(gpu):
    from hddm_amd import rl
    from test_hddmrl import CONDS, _stub_draw
    data, _ = rl.gen_rl_data(3, 20, CONDS, seed=5, draw=_stub_draw(5), a=1.8, t=0.3, v=2.5,
                             alpha=-0.5)
    m = rl.HDDMrl(data, seed=3)
    m.sample(30, burn=10)
    over = lambda s: {f: m.trace_subj[f][s] for f in m.FAMILIES}
    mean = lambda: {f: m.trace_subj[f].mean(axis=0) for f in m.FAMILIES}
    terms = lambda s: m.dataset.wiener_like_rlddm_nodes(*m._tables(over(s)), terms=True,
                                                        **m.wp)[1]
    w = _check_model(m, over, mean, terms)
    # 3 subjects x 2 conditions: every segment's first trial is not scored
    assert w["n_trials"] == 3 * 2 * 20 - 6


@pytest.mark.gpu
@pytest.mark.parametrize("group_only", [True, False])
def test_regressor_dic_and_waic(gpu, group_only):
    from hddm_amd.regression import HDDMRegressor
    m = HDDMRegressor(_ddm_frame(3, 40, 9), ["v ~ 1 + cov", {"model": "a ~ 1", "link_func": "exp"}],
                      group_only_regressors=group_only, seed=0)
    m.sample(30, burn=10)
    coef = (lambda s: {nm: float(m.trace[nm][s]) for nm in m.coef_names}) if group_only else \
        (lambda s: {nm: m.trace_subj[nm][s] for nm in m.coef_names})
    over = lambda s: {**{f: m.trace_subj[f][s] for f in m.FAMILIES}, **coef(s)}
    mean = lambda: {**{f: m.trace_subj[f].mean(axis=0) for f in m.FAMILIES},
                    **{nm: (float(np.mean(m.trace[nm])) if group_only
                            else m.trace_subj[nm].mean(axis=0)) for nm in m.coef_names}}
    terms = lambda s: m.dataset.wiener_like_reg_groups(
        m.reg_model, m.coef_table(over(s)), m.node_table(over(s)), terms=True, **m.wp)[1]
    w = _check_model(m, over, mean, terms)
    assert w["n_trials"] == 120
