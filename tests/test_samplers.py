"""What HDDM, HDDMChains, HDDMRegressor and optimize's flat model share: the
model spec (hierarchical.MODEL / INTER), the group-node names, the parameter
table and the refusals of the subclasses. All on the CPU over the oracle-backed
stand-ins of the resident data sets."""
import numpy as np
import pytest
from scipy import stats

from test_hierarchical import _OracleDataset, _cpu_data
from test_regressor import MODELS, _OracleRegDataset, _gamma
from test_regressor import _cpu_data as _reg_data

FULL = ("sv", "sz", "st")


@pytest.fixture
def h(oracle_lib, monkeypatch):
    from hddm_amd import hierarchical
    monkeypatch.setattr(hierarchical._wfpt, "Dataset", _OracleDataset)
    return hierarchical


@pytest.fixture
def reg(oracle_lib, monkeypatch):
    from hddm_amd import regression
    monkeypatch.setattr(regression._wfpt, "RegDataset", _OracleRegDataset)
    return regression


def _chain_states(m, rng):
    """Non-default values, different in each chain, written into an HDDMChains."""
    C = m.C
    m.group["a"][:] = 1.6 + 0.3 * rng.uniform(size=(C, 1))
    m.group["v"][:] = rng.normal(1.0, 0.5, size=(C, 2))
    m.group["t"][:] = 0.2 + 0.05 * rng.uniform(size=(C, 1))
    m.std["a"][:] = 0.2 + 0.2 * rng.uniform(size=C)
    m.std["v"][:] = 0.3 + 0.3 * rng.uniform(size=C)
    m.std["t"][:] = 0.03 + 0.04 * rng.uniform(size=C)
    m.subj["a"] = 1.5 + 0.5 * rng.uniform(size=(C, m.n_units["a"]))
    m.subj["v"] = rng.normal(1.0, 0.6, size=(C, m.n_units["v"]))
    m.subj["t"] = 0.15 + 0.1 * rng.uniform(size=(C, m.n_units["t"]))
    m.inter["sv"][:] = 0.2 + 0.3 * rng.uniform(size=C)
    m.inter["sz"][:] = 0.05 + 0.2 * rng.uniform(size=C)
    m.inter["st"][:] = 0.02 + 0.05 * rng.uniform(size=C)


def _one_chain(h, data, chains, c):
    """An HDDM at the values of chain c of `chains`."""
    m = h.HDDM(data, depends_on={"v": "cond"}, include=FULL, seed=0)
    for fam in m.FAMILIES:
        m.group[fam] = chains.group[fam][c].copy()
        m.std[fam] = float(chains.std[fam][c])
        m.subj[fam] = chains.subj[fam][c].copy()
    for name in FULL:
        m.inter[name] = float(chains.inter[name][c])
    return m


def test_logp_matches_a_restatement(h, oracle_lib):
    """HDDM.logp() and HDDMChains.logp() against the header's model written
    out with scipy.stats and the oracle's per-node likelihood (4 subjects x 2
    conditions x 40 trials, sv, sz, st included, three different states)."""
    data = _cpu_data(n=40)
    chains = h.HDDMChains(data, chains=3, depends_on={"v": "cond"}, include=FULL, seed=0)
    _chain_states(chains, np.random.default_rng(5))
    got_chains = chains.logp()
    assert got_chains.shape == (3,)
    rt, subj, cond = (data[k].to_numpy() for k in ("rt", "subj_idx", "cond"))
    level = {"hi": 0, "lo": 1}  # sorted condition levels
    for c in range(3):
        a, v, t = (chains.subj[f][c] for f in ("a", "v", "t"))
        ga, gv, gt = (chains.group[f][c] for f in ("a", "v", "t"))
        sa, sv_, st_ = (chains.std[f][c] for f in ("a", "v", "t"))
        sv, sz, st = (chains.inter[n][c] for n in FULL)
        want = 0.0
        for s in range(4):
            for cn, lv in level.items():
                want += oracle_lib.wiener_like(rt[(subj == s) & (cond == cn)], v[2 * s + lv], sv,
                                               a[s], 0.5, sz, t[s], st, 1e-4, 2, 2, 1, 1e-3,
                                               0.05, 0.1)
        want += np.sum(_gamma(a, ga[0], sa)) + _gamma(ga[0], 1.5, 0.75)
        want += np.sum(stats.norm.logpdf(v, np.tile(gv, 4), sv_))
        want += np.sum(stats.norm.logpdf(gv, 2.0, 3.0))
        want += np.sum(_gamma(t, gt[0], st_)) + _gamma(gt[0], 0.4, 0.2)
        want += stats.halfnorm.logpdf(sa, scale=2.0) + stats.halfnorm.logpdf(sv_, scale=2.0)
        want += stats.halfnorm.logpdf(st_, scale=1.0)
        want += stats.halfnorm.logpdf(sv, scale=2.0) + stats.beta.logpdf(sz, 1, 3)
        want += stats.halfnorm.logpdf(st, scale=0.3)
        assert np.isfinite(want)
        got = _one_chain(h, data, chains, c).logp()
        print(f"chain {c}: want {want!r} HDDM {got!r} HDDMChains {got_chains[c]!r}")
        assert abs(got - want) < 1e-9 * abs(want), (c, got, want)
        assert abs(got_chains[c] - want) < 1e-9 * abs(want), (c, got_chains[c], want)


def test_table_builders_agree(h):
    """One state, four builders of the (n_nodes, 8) parameter table."""
    from hddm_amd.optimize import _FlatModel
    data = _cpu_data(n=40)
    chains = h.HDDMChains(data, chains=3, depends_on={"v": "cond"}, include=FULL, seed=0,
                          p_outlier=0.03)
    _chain_states(chains, np.random.default_rng(6))
    m = _one_chain(h, data, chains, 1)
    m.p_outlier = 0.03
    P = m.node_table()
    assert P.shape == (8, 8) and np.all(P[:, 3] == 0.5) and np.all(P[:, 7] == 0.03)
    for fam in m.FAMILIES:
        assert np.array_equal(P[:, m._COL[fam]], m.subj[fam][m.node_unit[fam]])
    for name in FULL:
        assert np.all(P[:, m._COL[name]] == m.inter[name])
    assert np.array_equal(chains.node_tables()[1], P)
    m.trace_subj = {fam: m.subj[fam][None] for fam in m.FAMILIES}
    m.trace = {name: np.array([m.inter[name]]) for name in FULL}
    picked, rows = m.post_pred_rows(1)
    assert list(picked) == [0] and np.array_equal(rows[0], P)
    # the flat model: one subject, whose subject values follow its group nodes
    one = h.HDDM(data[data["subj_idx"] == 2], depends_on={"v": "cond"}, include=FULL, seed=0,
                 p_outlier=0.03)
    one.set_values({"a": 1.7, "v(hi)": 1.3, "v(lo)": 0.4, "t": 0.21, "sv": 0.3, "sz": 0.2,
                    "st": 0.04})
    flat = _FlatModel(one)
    T = flat.table(flat.current()[None], flat.node_col)[0]
    assert np.array_equal(T, one.node_table())
    assert np.all(T[:, 3] == 0.5) and np.all(T[:, 7] == 0.03)
    assert [list(r) for r in T] == [[1.3, 0.3, 1.7, 0.5, 0.2, 0.21, 0.04, 0.03],
                                    [0.4, 0.3, 1.7, 0.5, 0.2, 0.21, 0.04, 0.03]]


NODES = ["a", "v(hi)", "v(lo)", "t"]
TRACE = NODES + ["a_std", "v_std", "t_std", "st"]


def test_group_node_names(h):
    from hddm_amd.optimize import _FlatModel
    data = _cpu_data(n=40)
    m = h.HDDM(data, depends_on={"v": "cond"}, include=("st",), seed=0)
    assert [name for name, _, _ in m.group_nodes()] == NODES
    assert list(m.sample(2)) == TRACE and list(m.trace_subj) == ["a", "v", "t"]
    assert _FlatModel(m).names == NODES + ["st"]
    m.set_values({name: 0.5 for name in NODES + ["st"]})
    assert m.group["v"][1] == 0.5 and m.inter["st"] == 0.5
    for bad in ("a_std", "v", "v(mid)", "sv", "a()"):
        with pytest.raises(KeyError):
            m.set_values({bad: 0.5})
    c = h.HDDMChains(data, chains=2, depends_on={"v": "cond"}, include=("st",), seed=0)
    assert list(c.sample(2)) == TRACE and list(c.trace_subj) == ["a", "v", "t"]
    assert c.trace["v(lo)"].shape == (2, 2) and c.trace_subj["v"].shape == (2, 2, 8)


@pytest.mark.parametrize("group_only", [True, False])
def test_regressor_node_names(reg, group_only):
    m = reg.HDDMRegressor(_reg_data(), "a ~ cov", depends_on={"v": "cond"}, include=("st",),
                          group_only_regressors=group_only, seed=0)
    nodes = ["v(hi)", "v(lo)", "v(mid)", "t"]
    coefs = ["a_Intercept", "a_cov"] if group_only else \
        ["a_Intercept", "a_Intercept_std", "a_cov", "a_cov_std"]
    assert list(m.sample(2)) == nodes + ["v_std", "t_std"] + coefs + ["st"]
    assert list(m.trace_subj) == ["v", "t"] + ([] if group_only else ["a_Intercept", "a_cov"])
    m.set_values({name: 0.5 for name in nodes + ["st"]})
    assert np.all(m.group["v"] == 0.5) and m.group["t"][0] == 0.5 and m.inter["st"] == 0.5
    for bad in ("a", "a_Intercept", "v_std", "sz"):
        with pytest.raises(KeyError):
            m.set_values({bad: 0.5})


def test_subclasses_refuse_what_they_do_not_support(h, reg):
    """On a model, on a bare instance and through the class, whatever the
    arguments (optimize: test_optimize.py; the cdf post_pred_gen: test_sim.py)."""
    refused = {h.HDDMChains: ("set_values", "quantile_objective", "node_logp_multi",
                              "post_pred_gen", "post_pred_rows", "optimize", "node_table"),
               reg.HDDMRegressor: ("quantile_objective", "node_logp_multi", "post_pred_gen",
                                   "post_pred_rows", "optimize")}
    models = {h.HDDMChains: h.HDDMChains(_cpu_data(n=40), chains=2, seed=0),
              reg.HDDMRegressor: reg.HDDMRegressor(_reg_data(), MODELS, seed=0)}
    for cls, names in refused.items():
        for name in names:
            for m in (models[cls], object.__new__(cls)):
                with pytest.raises(NotImplementedError, match="."):
                    getattr(m, name)()
                with pytest.raises(NotImplementedError):
                    getattr(cls, name)(m, "gsquare")
        for kw in ({"method": "drift"}, {"method": "cdf", "samples": 3}, {"no_such": 1}):
            with pytest.raises(NotImplementedError):
                models[cls].post_pred_gen(**kw)
    with pytest.raises(NotImplementedError):
        models[h.HDDMChains].set_values({"a": 1.0})
    assert np.all(models[h.HDDMChains].group["a"] == 1.5)
