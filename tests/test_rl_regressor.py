"""HDDMrlRegressor (hddm_amd/rl_regression.py; the reference's
hddm/models/hddm_rl_regression.py): bookkeeping, the joint density against a
restatement, short chains, refusals and the unsorted-data warning on the CPU
with an oracle-backed stand-in for wfpt.RLRegDataset; recovery of a block
effect on the learning rate on the GPU.
"""
import math
import warnings

import numpy as np
import pytest
from scipy import stats

from test_hddmrl import CONDS, _cpu_data as _rl_cpu_data
from test_regressor import _gamma
from test_rl_reg import recurrence

RL_BASE = 2.718281828459
LINK = {"identity": lambda e: e, "exp": np.exp, "invlogit": lambda e: 1 / (1 + np.exp(-e))}
WP = dict(err=1e-4, n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, w_outlier=0.1)


def _rate(alpha):
    e = RL_BASE ** np.asarray(alpha, dtype=np.float64)
    return e / (1 + e)


def _node(o, rt, response, feedback, split, q, rate, vmul, sv, a, z, sz, t, st, p_outlier):
    """One node as the reference scores it: the recurrence's drifts into the
    oracle's wiener_like_multi."""
    n = rt.size
    drift = recurrence(response, feedback, split, q, np.broadcast_to(rate, n),
                       np.broadcast_to(vmul, n))
    multi = ["v"] + [k for k, val in (("a", a), ("t", t)) if np.ndim(val)]
    return o.wiener_like_multi(rt, drift, sv, a, z, sz, t, st, WP["err"], multi=multi,
                               n_st=WP["n_st"], n_sz=WP["n_sz"], use_adaptive=1,
                               simps_err=WP["simps_err"], p_outlier=p_outlier,
                               w_outlier=WP["w_outlier"])


class _OracleRLRegDataset:
    """Test stand-in for hddm_amd.wfpt.RLRegDataset backed by the oracle (CPU)."""

    def __init__(self, rt, response, feedback, split_by, design, group_id=None, n_groups=None,
                 device=None):
        import oracle
        self.o = oracle
        self.rt = np.asarray(rt, dtype=np.float64)
        self.response, self.feedback, self.split = response, feedback, split_by
        self.X = np.asarray(design, dtype=np.float64)
        self.group = np.asarray(group_id)
        self.n_groups = n_groups

    def wiener_like_rl_reg_groups(self, model, coef_table, q, alpha, params, err, n_st, n_sz,
                                  use_adaptive, simps_err, w_outlier):
        assert (err, n_st, n_sz, use_adaptive, simps_err, w_outlier) == tuple(WP.values())
        out = np.zeros(self.n_groups)
        for g in range(self.n_groups):
            sel = self.group == g
            if not sel.any():
                continue
            vals = dict(zip(("v", "sv", "a", "z", "sz", "t", "st"), params[g][:7]), alpha=alpha[g])
            for name, c0, nc, lk in model:
                eta = np.zeros(int(sel.sum()))
                for c in range(c0, c0 + nc):
                    eta = eta + self.X[sel, c] * coef_table[g][c]
                vals[name] = LINK[lk](eta)
            out[g] = _node(self.o, self.rt[sel], self.response[sel], self.feedback[sel],
                           self.split[sel], q[g], _rate(vals["alpha"]), vals["v"], vals["sv"],
                           vals["a"], vals["z"], vals["sz"], vals["t"], vals["st"], params[g][7])
        return out


def _cpu_data(seed=5, **kw):
    data, _ = _rl_cpu_data(seed=seed, **kw)
    data["cov"] = np.random.default_rng(seed).normal(size=len(data))
    return data


@pytest.fixture
def rlreg(oracle_lib, monkeypatch):
    from hddm_amd import rl_regression as mod
    monkeypatch.setattr(mod._wfpt, "RLRegDataset", _OracleRLRegDataset)
    return mod


# ---------------------------------------------------------------- CPU

def test_rl_regressor_bookkeeping_on_cpu(rlreg):
    import hddm_amd
    assert hddm_amd.HDDMrlRegressor is rlreg.HDDMrlRegressor
    data = _cpu_data()
    m = rlreg.HDDMrlRegressor(data, ["alpha ~ 1 + cov", {"model": "a ~ 1 + cov",
                                                         "link_func": "exp"}], seed=0)
    assert m.coef_names == ["alpha_Intercept", "alpha_cov", "a_Intercept", "a_cov"]
    assert m.coef_intercept == [True, False, True, False]
    assert m.reg_model == [("alpha", 0, 2, "identity"), ("a", 2, 2, "exp")]
    assert m.FAMILIES == ("v", "t") and m.n_nodes == 4 and m.design.shape == (160, 4)
    assert np.array_equal(m.node_q, np.full(4, 0.5)) and np.all(m.alpha_rows() == 0)
    assert m.coef_table().shape == (4, 4) and m.node_table().shape == (4, 8)
    # the intercept of a regressed alpha starts at 0 and takes the family's prior
    assert m.coef["alpha_Intercept"] == 0.0
    assert m._coef_group_prior("alpha_Intercept", 3.0) == stats.norm.logpdf(3.0, 0, 50)
    assert m._coef_group_prior("alpha_cov", 3.0) == pytest.approx(stats.norm.logpdf(3.0, 0, 15))
    # alpha not regressed: a subject-level family after a, v, t with HDDMrl's slice widths
    data["q_init"] = np.where(data["subj_idx"] == 2, 0.3, 0.6)
    m = rlreg.HDDMrlRegressor(data, "v ~ 1 + cov", seed=0)
    assert m.FAMILIES == ("a", "t", "alpha") and m.coef_names == ["v_Intercept", "v_cov"]
    assert np.array_equal(m.node_q, [0.6, 0.6, 0.3, 0.6])
    assert m.group["alpha"][0] == 0.0 and np.all(m.subj["alpha"] == 0.0) and m.std["alpha"] == 0.1
    assert m.SLICE_WIDTHS["alpha"] == 1.5 and m.SLICE_WIDTHS["alpha_std"] == 1
    assert m.MODEL["alpha"].group_prior == ("normal", 0.0, 50.0) and m.MODEL["alpha"].std_sd == 10.0
    m.subj["alpha"] = np.arange(4.0)
    assert np.array_equal(m.alpha_rows(), np.arange(4.0))
    assert np.array_equal(m.alpha_rows({"alpha": np.full(4, 7.0)}), np.full(4, 7.0))
    assert list(m.sample(2)) == ["a", "t", "alpha", "a_std", "t_std", "alpha_std", "v_Intercept",
                                 "v_cov"]
    assert list(m.trace_subj) == ["a", "t", "alpha"]


@pytest.mark.parametrize("regress_alpha", [True, False])
def test_rl_regressor_logp_matches_a_restatement(rlreg, oracle_lib, regress_alpha):
    data = _cpu_data()
    models = ["v ~ 1 + cov"] + (["alpha ~ 1 + cov"] if regress_alpha else [])
    m = rlreg.HDDMrlRegressor(data, models, group_only_regressors=False, seed=0)
    rng = np.random.default_rng(1)
    S = m.n_subj
    g = {"v_Intercept": 2.2, "v_cov": 0.3, "alpha_Intercept": -0.6, "alpha_cov": 0.4}
    for nm in m.coef_names:
        m.coef[nm] = g[nm]
        m.coef_std[nm] = 0.2 + 0.1 * rng.uniform()
        m.coef_subj[nm] = g[nm] + 0.05 * rng.normal(size=S)
    fam = {"a": (1.7, 0.3, 1.8, 2.0), "t": (0.25, 0.07, 0.2, 1.0)}  # group, std, subj, std_sd
    if not regress_alpha:
        fam["alpha"] = (-0.4, 0.5, -0.5, 10.0)
    for f, (gm, sd, sub, _) in fam.items():
        m.group[f][:] = gm
        m.std[f] = sd
        m.subj[f] = sub + 0.02 * rng.uniform(size=S)
    X = np.column_stack([np.ones(len(data)), data["cov"]])
    col = lambda c: data[c].to_numpy()
    want = 0.0
    for s in range(S):
        sel = (data["subj_idx"] == s).to_numpy()
        b = lambda out: np.array([m.coef_subj[f"{out}_Intercept"][s], m.coef_subj[f"{out}_cov"][s]])
        alpha = X[sel] @ b("alpha") if regress_alpha else m.subj["alpha"][s]
        want += _node(oracle_lib, col("rt")[sel], col("response")[sel], col("feedback")[sel],
                      col("split_by")[sel], 0.5, _rate(alpha), X[sel] @ b("v"), 0.0,
                      m.subj["a"][s], 0.5, 0.0, m.subj["t"][s], 0.0, 0.05)
    for f, (gm, sd, _, std_sd) in fam.items():
        if f == "alpha":
            want += np.sum(stats.norm.logpdf(m.subj[f], gm, sd)) + stats.norm.logpdf(gm, 0, 50)
        else:
            want += np.sum(_gamma(m.subj[f], gm, sd))
            want += _gamma(gm, *{"a": (1.5, 0.75), "t": (0.4, 0.2)}[f])
        want += stats.halfnorm.logpdf(sd, scale=std_sd)
    for nm in m.coef_names:
        want += np.sum(stats.norm.logpdf(m.coef_subj[nm], m.coef[nm], m.coef_std[nm]))
        if nm.endswith("Intercept"):
            mu, sd, std_sd = {"v": (2.0, 3.0, 2.0), "alpha": (0.0, 50.0, 10.0)}[nm.split("_")[0]]
            want += stats.norm.logpdf(m.coef[nm], mu, sd)
            want += stats.halfnorm.logpdf(m.coef_std[nm], scale=std_sd)
        else:
            want += stats.norm.logpdf(m.coef[nm], 0, 15) - math.log(100.0 - 1e-10)
    got = m.logp()
    assert np.isfinite(want)
    assert abs(got - want) < 1e-9 * abs(want), (got, want)


@pytest.mark.parametrize("group_only", [True, False])
def test_rl_regressor_short_chain_on_cpu(rlreg, group_only):
    m = rlreg.HDDMrlRegressor(_cpu_data(), ["alpha ~ 1 + cov", "v ~ 1"],
                              group_only_regressors=group_only, seed=0)
    tr = m.sample(3)
    want = set(m.coef_names) | {"a", "t", "a_std", "t_std"}
    if not group_only:
        want |= {nm + "_std" for nm in m.coef_names}
    assert set(tr) == want
    for k, v in tr.items():
        assert v.shape == (3,) and np.all(np.isfinite(v)), k
    if not group_only:
        assert m.trace_subj["alpha_cov"].shape == (3, 4)
    assert np.isfinite(m.logp())
    assert m.likelihood_calls > 3 and sum(c for c, _ in m.call_stats.values()) == \
        m.likelihood_calls


def test_rl_regressor_refusals(rlreg):
    data = _cpu_data()
    with pytest.raises(TypeError, match="HDDMrlRegressor: .*identity.*exp.*invlogit"):
        rlreg.HDDMrlRegressor(data, {"model": "alpha ~ cov", "link_func": lambda x: x})
    with pytest.raises(ValueError, match="HDDMrlRegressor: 'alpha' is a regression outcome"):
        rlreg.HDDMrlRegressor(data, "alpha ~ cov", depends_on={"alpha": "split_by"})
    with pytest.raises(NotImplementedError, match=r"'z' is not supported.*\(v, a, t, alpha\)"):
        rlreg.HDDMrlRegressor(data, "z ~ cov")
    with pytest.raises(KeyError, match="feedback"):
        rlreg.HDDMrlRegressor(data.drop(columns="feedback"), "v ~ cov")
    # HDDMRegressor keeps its own outcomes and words
    from hddm_amd import regression
    with pytest.raises(NotImplementedError,
                       match=r"HDDMRegressor: outcome 'alpha' is not supported at model level "
                             r"\(v, a, t\)"):
        regression.HDDMRegressor(data, "alpha ~ cov")
    m = rlreg.HDDMrlRegressor(data, "alpha ~ cov", seed=0)
    for name, word in (("dic_info", "pointwise"), ("dic", "pointwise"), ("waic", "pointwise"),
                       ("pointwise_loglik", "pointwise"), ("post_pred_rows", "posterior pred"),
                       ("post_pred_gen", "posterior pred"), ("post_pred_stats", "posterior pred"),
                       ("optimize", "point fits"), ("quantile_objective", "point fits"),
                       ("node_logp_multi", "one table")):
        for obj in (m, object.__new__(rlreg.HDDMrlRegressor)):
            with pytest.raises(NotImplementedError, match=word):
                getattr(obj, name)()


def test_rl_regressor_warns_about_unsorted_data(rlreg):
    data = _cpu_data()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # contiguous runs: no warning
        rlreg.HDDMrlRegressor(data, "v ~ cov", seed=0)
    # subject 1's trials interleaved: condition 0 comes back after condition 1
    sub = data[data["subj_idx"] == 1]
    mixed = sub.iloc[np.argsort(np.arange(len(sub)) % 10, kind="stable")]
    shuffled = data.copy()
    shuffled.loc[sub.index] = mixed.to_numpy()
    with pytest.warns(UserWarning, match="Q restarts at every adjacent change") as rec:
        rlreg.HDDMrlRegressor(shuffled, "v ~ cov", seed=0)
    assert len([w for w in rec if issubclass(w.category, UserWarning)]) == 1


# ---------------------------------------------------------------- recovery on the GPU

def _block_data():
    """Two gen_rl_data sets that differ in the learning rate (alpha -2.5 in
    block 0, 0.5 in block 1), joined per subject with disjoint split_by values
    and sorted so that every (subject, condition) run is contiguous."""
    import pandas as pd
    from hddm_amd import rl
    parts, truth = [], None
    for block, alpha in enumerate((-2.5, 0.5)):
        d, truth = rl.gen_rl_data(12, 60, CONDS, a=1.8, t=0.3, v=3.0, alpha=alpha, seed=77)
        d["block"] = block
        d["split_by"] = d["split_by"] + 2 * block
        parts.append(d)
    data = pd.concat(parts, ignore_index=True)
    return data.sort_values(["subj_idx", "split_by"], kind="stable").reset_index(drop=True), truth


@pytest.mark.gpu
def test_rl_regressor_recovers_a_block_effect_on_alpha(gpu):
    """12 subjects x 2 blocks x 2 conditions x 60 trials, alpha -2.5 in block 0
    and 0.5 in block 1, 150 sweeps with burn 50: the block coefficient and v
    credibly positive, a and t at test_hddmrl_recovery's bars.

    Measured on an MI355X: alpha_block 3.077 [2.860, 3.294],
    alpha_Intercept -2.498 [-2.645, -2.316], v 3.078 [2.910, 3.263], a 1.736
    [1.669, 1.794] (true 1.765), t 0.308 [0.299, 0.318] (true 0.299)."""
    from hddm_amd import HDDMrlRegressor
    data, truth = _block_data()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = HDDMrlRegressor(data, "alpha ~ 1 + block", seed=1)
    m.sample(150, burn=50)
    st = m.gen_stats()
    print(f"sample {m.sample_seconds:.2f}s, {m.likelihood_calls} likelihood calls; true a "
          f"{np.mean(truth['a']):.3f} t {np.mean(truth['t']):.3f} v {np.mean(truth['v']):.3f}")
    for k in ("a", "v", "t", "alpha_Intercept", "alpha_block"):
        print(f"  {k}: mean {st[k]['mean']:.3f} [{st[k]['2.5q']:.3f}, {st[k]['97.5q']:.3f}]")
    assert st["alpha_block"]["2.5q"] > 0
    assert st["v"]["2.5q"] > 0
    assert abs(st["a"]["mean"] - np.mean(truth["a"])) < 0.25
    assert abs(st["t"]["mean"] - np.mean(truth["t"])) < 0.05
