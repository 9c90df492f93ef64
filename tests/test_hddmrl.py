"""HDDMrl (hddm_amd/rl.py): the hierarchical RLDDM sampler and gen_rl_data.

The CPU tests run over `_OracleRLDataset`, a stand-in for wfpt.RLDataset whose
node likelihood is the restated Q recurrence (tests/test_rl.py) plus the
oracle's wiener_like_multi per node. No reference sampler can run here (PyMC 2
and kabuki are absent), so the model is pinned through its joint density, its
node likelihoods and, on the device, recovery conditions.
"""
import numpy as np
import pytest
from scipy import stats

from test_rl import restate_rlddm

KEYS = ["a", "v", "t", "a_std", "v_std", "t_std", "alpha", "alpha_std"]


class _OracleRLDataset:
    """Test stand-in for hddm_amd.wfpt.RLDataset backed by the oracle (CPU)."""

    def __init__(self, rt, response, feedback, split_by, node_id=None, n_nodes=None, device=None):
        import oracle
        self.o = oracle
        self.rt = np.asarray(rt, dtype=np.float64)
        self.response, self.feedback = np.asarray(response), np.asarray(feedback)
        self.split_by, self.node, self.n_nodes = np.asarray(split_by), np.asarray(node_id), n_nodes
        self.n = self.rt.size

    def node_terms(self, j, rl_row, row, err, n_st, n_sz, use_adaptive, simps_err, w_outlier):
        """(sum, number of scored trials) of node j: wienerRL_like restated."""
        sel = self.node == j
        v, sv, a, z, sz, t, st, po = row
        drift, scored = restate_rlddm(self.response[sel], self.feedback[sel], self.split_by[sel],
                                      *rl_row, v)
        if not (0 <= po <= 1):
            return -np.inf, int(scored.sum())
        if not scored.any():
            return 0.0, 0
        return self.o.wiener_like_multi(
            self.rt[sel][scored], drift[scored], sv, a, z, sz, t, st, err, multi=["v"], n_st=n_st,
            n_sz=n_sz, use_adaptive=use_adaptive, simps_err=simps_err, p_outlier=po,
            w_outlier=w_outlier), int(scored.sum())

    def wiener_like_rlddm_nodes(self, rl_rows, params, **kw):
        return np.array([self.node_terms(j, rl_rows[j], params[j], **kw)[0]
                         for j in range(self.n_nodes)])

    def wiener_like_rlddm_nodes_multi(self, rl_tables, params, **kw):
        self.multi_calls = getattr(self, "multi_calls", 0) + 1
        return np.stack([self.wiener_like_rlddm_nodes(r, p, **kw)
                         for r, p in zip(rl_tables, params)])


def _stub_draw(seed):
    """A deterministic stand-in for the device draw: the upper boundary is the
    likelier the larger the drift."""
    rng = np.random.default_rng(seed)

    def draw(drifts):
        up = rng.uniform(size=drifts.size) < 1 / (1 + np.exp(-1.5 * drifts))
        return np.where(up, 1.0, -1.0) * (0.35 + rng.gamma(2.0, 0.25, drifts.size))
    return draw


CONDS = {0: (0.8, 0.2), 1: (0.7, 0.3)}


def _cpu_data(n_subj=4, n=20, seed=5, **kw):
    from hddm_amd import rl
    args = dict(a=1.8, t=0.3, v=2.5, alpha=-0.5)
    args.update(kw)
    return rl.gen_rl_data(n_subj, n, CONDS, seed=seed, draw=_stub_draw(seed), **args)


@pytest.fixture
def rl(oracle_lib, monkeypatch):
    from hddm_amd import rl as mod
    monkeypatch.setattr(mod._wfpt, "RLDataset", _OracleRLDataset)
    return mod


# ---------------------------------------------------------------- CPU

def test_hddmrl_bookkeeping_on_cpu(rl):
    data, _ = _cpu_data()
    data["cond"] = np.where(data["trial"] % 2 == 0, "even", "odd")
    data.loc[data["subj_idx"] == 2, "q_init"] = 0.4
    m = rl.HDDMrl(data, seed=0)
    assert m.FAMILIES == ("a", "v", "t", "alpha") and not m.dual
    assert m.n_nodes == 4 and m.n_units["alpha"] == 4  # split_by makes segments, not nodes
    assert np.array_equal(m.node_q, [0.5, 0.5, 0.4, 0.5])
    R, P = m.rl_table(), m.node_table()
    assert R.shape == (4, 3) and P.shape == (4, 8)
    assert np.array_equal(R[:, 0], m.node_q) and np.all(R[:, 1] == 0.0) and np.all(R[:, 2] == 100.0)
    assert np.all(P[:, 3] == 0.5) and np.all(P[:, 7] == 0.05) and np.all(P[:, 0] == 2.0)
    assert np.array_equal(m.rl_table({"alpha": np.arange(4.0)})[:, 1], np.arange(4.0))
    assert m.SLICE_WIDTHS["alpha"] == 1.5 and m.SLICE_WIDTHS["alpha_std"] == 1
    assert m.std["alpha"] == 0.1 and m.group["alpha"][0] == 0.0
    m.sample(2)
    assert list(m.trace) == KEYS and list(m.trace_subj) == ["a", "v", "t", "alpha"]
    assert set(m.gen_stats()) == set(KEYS)
    m.set_values({"alpha": -1.0, "a": 1.7})
    assert m.group["alpha"][0] == -1.0 and m.group["a"][0] == 1.7
    # dual: a second, identical family for positive prediction errors
    d = rl.HDDMrl(data, dual=True, include=("sv",), seed=0)
    assert d.FAMILIES == ("a", "v", "t", "alpha", "pos_alpha")
    d.subj["pos_alpha"] = np.arange(4.0) / 10
    assert np.array_equal(d.rl_table()[:, 2], np.arange(4.0) / 10)
    assert d.MODEL["pos_alpha"] == d.MODEL["alpha"]
    d.sample(1)
    assert list(d.trace) == KEYS + ["pos_alpha", "pos_alpha_std", "sv"]
    # depends_on for alpha: (subject, level) units, nodes are subject x cond
    c = rl.HDDMrl(data, depends_on={"alpha": "cond"}, seed=0)
    assert c.n_nodes == 8 and c.n_units["alpha"] == 8 and c.n_units["a"] == 4
    assert c.levels["alpha"] == [("even",), ("odd",)]
    c.subj["alpha"] = np.arange(8.0)
    assert np.array_equal(c.rl_table()[:, 1], c.node_unit["alpha"].astype(float))
    assert [k for k, _, _ in c.group_nodes()][3:] == ["alpha(even)", "alpha(odd)"]
    assert np.isfinite(c.logp())
    # what the RL model does not offer
    for call in (lambda: m.optimize("ML"), lambda: m.quantile_objective("chisquare"),
                 m.post_pred_rows, m.post_pred_gen, m.post_pred_stats,
                 lambda: rl.HDDMrl(data, non_centered=True)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(KeyError):
        rl.HDDMrl(data.drop(columns="feedback"))


def _gamma(x, mean, sd):
    return stats.gamma.logpdf(x, mean ** 2 / sd ** 2, scale=sd ** 2 / mean)


@pytest.mark.parametrize("dual", [False, True])
def test_hddmrl_logp_matches_a_restatement(rl, oracle_lib, dual):
    data, _ = _cpu_data()
    m = rl.HDDMrl(data, dual=dual, include=("st",), seed=0)
    rng = np.random.default_rng(1)
    S = m.n_subj
    g = {"a": 1.7, "v": 2.2, "t": 0.25, "alpha": -0.4, "pos_alpha": 0.3}
    sd = {"a": 0.2, "v": 0.5, "t": 0.07, "alpha": 0.6, "pos_alpha": 1.3}
    for fam in m.FAMILIES:
        m.group[fam][:] = g[fam]
        m.std[fam] = sd[fam]
        m.subj[fam] = g[fam] * (1 + 0.05 * rng.uniform(-1, 1, S))
    m.inter["st"] = 0.04
    want = 0.0
    ds = m.dataset
    for s in range(S):
        pos = m.subj["pos_alpha"][s] if dual else 100.0
        row = (m.subj["v"][s], 0.0, m.subj["a"][s], 0.5, 0.0, m.subj["t"][s], 0.04, 0.05)
        want += ds.node_terms(s, (0.5, m.subj["alpha"][s], pos), row, 1e-4, 2, 2, 1, 1e-3, 0.1)[0]
    want += _gamma(g["a"], 1.5, 0.75) + np.sum(_gamma(m.subj["a"], g["a"], sd["a"]))
    want += stats.norm.logpdf(g["v"], 2.0, 3.0) + np.sum(stats.norm.logpdf(m.subj["v"], g["v"],
                                                                           sd["v"]))
    want += _gamma(g["t"], 0.4, 0.2) + np.sum(_gamma(m.subj["t"], g["t"], sd["t"]))
    want += stats.halfnorm.logpdf(sd["a"], scale=2.0) + stats.halfnorm.logpdf(sd["v"], scale=2.0)
    want += stats.halfnorm.logpdf(sd["t"], scale=1.0) + stats.halfnorm.logpdf(0.04, scale=0.3)
    for fam in m.rl_families:
        want += stats.norm.logpdf(g[fam], 0.2, 3.0)
        want += np.sum(stats.norm.logpdf(m.subj[fam], g[fam], sd[fam]))
        want += stats.uniform.logpdf(sd[fam], 1e-10, 10.0 - 1e-10)
    got = m.logp()
    assert np.isfinite(want)
    assert abs(got - want) < 1e-9 * abs(want), (got, want)
    m.std["alpha"] = 10.5  # outside the Uniform's support
    assert m.logp() == -np.inf


@pytest.mark.parametrize("dual", [False, True])
def test_hddmrl_short_chains_on_cpu(rl, dual):
    """Seeded chains run, stay finite, keep the std nodes inside their Uniform
    support, and are the same chain with and without paired probes."""
    data, _ = _cpu_data()
    traces, calls = [], []
    for paired in (False, True):
        m = rl.HDDMrl(data, dual=dual, include=("sz",) if dual else (), seed=3,
                      paired_probes=paired)
        m.sample(5)
        assert np.isfinite(m.logp())
        for k, v in m.trace.items():
            assert v.shape == (5,) and np.all(np.isfinite(v)), k
        for fam in m.rl_families:
            s = m.trace[fam + "_std"]
            assert np.all((s > 1e-10) & (s < 10))
            assert np.all(np.isfinite(m.trace_subj[fam])) and m.trace_subj[fam].shape == (5, 4)
        assert bool(getattr(m.dataset, "multi_calls", 0)) == paired
        traces.append((m.trace, m.trace_subj))
        calls.append(m.likelihood_calls)
    for part in (0, 1):
        for k in traces[0][part]:
            assert np.array_equal(traces[0][part][k], traces[1][part][k]), k
    assert calls[1] < calls[0]
    assert any(k.startswith("alpha") for k in m.call_stats)


@pytest.mark.parametrize("pos_alpha", [None, 0.8])
def test_gen_rl_data_closes_the_loop(pos_alpha):
    from hddm_amd import rl
    data, truth = _cpu_data(n_subj=3, n=25, seed=9, pos_alpha=pos_alpha)
    assert len(data) == 3 * 2 * 25 and set(truth) >= {"a", "t", "v", "alpha"}
    assert ("pos_alpha" in truth) == (pos_alpha is not None)
    assert np.array_equal((data["rt"] > 0).astype(int), data["response"])
    # the rewards are drawn up front from the generator's own stream, before any step
    rng = np.random.default_rng(9)
    rng.uniform(-1, 1, 3 * (4 if pos_alpha is None else 5))
    for s in range(3):
        sel = (data["subj_idx"] == s).to_numpy()
        d = data[sel]
        pos = 100.0 if pos_alpha is None else truth["pos_alpha"][s]
        drift, _ = restate_rlddm(d["response"].to_numpy(), d["feedback"].to_numpy(),
                                 d["split_by"].to_numpy(), 0.5, truth["alpha"][s], pos,
                                 truth["v"][s])
        assert np.array_equal(d["sim_drift"].to_numpy(), drift)
        assert np.array_equal(d["sim_drift"].to_numpy(),
                              (d["q_up"].to_numpy() - d["q_low"].to_numpy()) * truth["v"][s])
        for c, (p_up, p_low) in CONDS.items():
            seq = d[d["split_by"] == c]
            assert seq["sim_drift"].iloc[0] == 0.0 and list(seq["trial"]) == list(range(1, 26))
            up, low = rng.binomial(1, p_up, 25), rng.binomial(1, p_low, 25)
            assert np.array_equal(seq["feedback"].to_numpy(),
                                  np.where(seq["response"].to_numpy() == 1, up, low))
    assert rl.learning_rate(0.0) == 0.5


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_hddmrl_node_logp_matches_the_restatement(gpu, oracle_lib):
    from hddm_amd import rl
    data, _ = _cpu_data(n_subj=5, n=40)
    data["q_init"] = np.where(data["subj_idx"] == 1, 0.45, 0.5)
    m = rl.HDDMrl(data, dual=True, seed=0)
    m.subj["pos_alpha"] = np.linspace(-1.0, 1.0, 5)
    ref = _OracleRLDataset(m.signed_rt, data["response"], data["feedback"], data["split_by"],
                           node_id=m.node_codes, n_nodes=m.n_nodes)
    got = m.node_logp()
    R, P = m.rl_table(), m.node_table()
    for j in range(m.n_nodes):
        want, n_scored = ref.node_terms(j, R[j], P[j], **m.wp)
        print(f"node {j}: got {got[j]!r} want {want!r} scored {n_scored}")
        assert abs(got[j] - want) < n_scored * 1e-6
    multi = m.node_logp_multi([{}, {"alpha": np.full(5, -1.0)}, {"sv": 0.3}])
    assert np.array_equal(multi[0], got)
    assert np.array_equal(multi[1], m.node_logp({"alpha": np.full(5, -1.0)}))
    assert np.array_equal(multi[2], m.node_logp({"sv": 0.3}))


@pytest.mark.gpu
def test_hddmrl_paired_probes_keep_the_chain_on_the_device(gpu):
    """The end-to-end check that the multi call's rows are bit-identical: the
    same seed gives the same chain with and without the two-table probes."""
    from hddm_amd import rl
    data, _ = _cpu_data(n_subj=6, n=30)
    runs = []
    for paired in (False, True):
        m = rl.HDDMrl(data, dual=True, include=("sv", "sz", "st"), seed=11, paired_probes=paired)
        m.sample(8)
        runs.append(m)
    a, b = runs
    for part in ("trace", "trace_subj"):
        for k, v in getattr(a, part).items():
            assert np.array_equal(v, getattr(b, part)[k]), (part, k)
    assert b.likelihood_calls < a.likelihood_calls
    assert any(" x2" in k for k in b.call_stats) and not any(" x2" in k for k in a.call_stats)


@pytest.mark.gpu
def test_hddmrl_recovery(gpu):
    """Two data sets that differ only in the learning rate (alpha -2.5: rate
    0.076; alpha 0.5: rate 0.62), 12 subjects x 2 conditions x 60 trials, 150
    sweeps with burn 50. Conditions instead of a reference chain: v credibly
    positive, a and t at the bars tests/test_hierarchical.py and
    tests/test_regressor.py use at this size, and the two posteriors of alpha
    ordered and separated."""
    from hddm_amd import rl
    stats_ = {}
    for name, alpha in (("low", -2.5), ("high", 0.5)):
        data, truth = rl.gen_rl_data(12, 60, CONDS, a=1.8, t=0.3, v=3.0, alpha=alpha, seed=77)
        m = rl.HDDMrl(data, seed=1)
        m.sample(150, burn=50)
        st = m.gen_stats()
        stats_[name] = st
        print(f"alpha={alpha}: sample {m.sample_seconds:.2f}s, {m.likelihood_calls} likelihood "
              f"calls; true a {np.mean(truth['a']):.3f} t {np.mean(truth['t']):.3f} "
              f"v {np.mean(truth['v']):.3f} alpha {np.mean(truth['alpha']):.3f}")
        for k in ("a", "v", "t", "alpha", "alpha_std"):
            print(f"  {k}: mean {st[k]['mean']:.3f} [{st[k]['2.5q']:.3f}, {st[k]['97.5q']:.3f}]")
        assert st["v"]["2.5q"] > 0
        assert abs(st["a"]["mean"] - np.mean(truth["a"])) < 0.25
        assert abs(st["t"]["mean"] - np.mean(truth["t"])) < 0.05
    assert stats_["high"]["alpha"]["mean"] > stats_["low"]["alpha"]["mean"]
    assert stats_["high"]["alpha"]["2.5q"] > stats_["low"]["alpha"]["97.5q"]
