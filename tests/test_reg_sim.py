"""The regressor's posterior predictive: RegDataset.gen_rts_drift[_stats]
(wfpt_gen_rts_reg_drift*, reg_sim_kernel) and
HDDMRegressor.post_pred_gen / post_pred_stats.

The oracle of the draws is the project's own drift sampler: trial i of sweep s
is draw s of row i of gen_rts_from_drift_nodes over the trials' parameters, and
those parameters are the ones the regression likelihood predicts. Everything
is compared bit for bit, so the shapes are small: 201 trials in groups of 1, 70
and 130 (a one-trial group, group boundaries inside a wave, n no multiple of
64), shuffled against the stored order, 4 design columns, 3 sweeps, dt = 1e-3.
"""
import ctypes

import numpy as np
import pytest

N, G, C, S = 201, 3, 4, 3
SIZES = (1, 70, 130)
DT, SEED = 1e-3, 20240607
MODEL = [("v", 0, 2, "identity"), ("a", 2, 1, "exp"), ("t", 3, 1, "invlogit")]
MODEL_A_IDENTITY = [("v", 0, 2, "identity"), ("a", 2, 1, "identity"), ("t", 3, 1, "invlogit")]
FIELD = {"v": 0, "sv": 1, "a": 2, "z": 3, "sz": 4, "t": 5, "st": 6}


def _inputs(a_identity=False):
    """(rt, design, group ids, coef (S, G, C), params (S, G, 8))."""
    rng = np.random.default_rng(11)
    gid = rng.permutation(np.repeat(np.arange(G), SIZES)).astype(np.int32)
    X = np.column_stack([np.ones(N), rng.normal(size=N), rng.uniform(0.8, 1.2, N),
                         rng.uniform(0.8, 1.2, N)])
    rt = rng.choice([-1.0, 1.0], N, p=[0.3, 0.7]) * (0.5 + rng.gamma(2.0, 0.3, N))
    coef = np.empty((S, G, C))
    coef[..., 0] = rng.normal(0.8, 0.3, (S, G))
    coef[..., 1] = rng.normal(0.0, 0.4, (S, G))
    a = rng.uniform(1.2, 2.0, (S, G))
    coef[..., 2] = a if a_identity else np.log(a)
    coef[..., 3] = rng.uniform(-1.6, -1.0, (S, G))  # t = invlogit(.) ~ 0.17 .. 0.27
    par = np.zeros((S, G, 8))
    par[..., 0] = par[..., 2] = par[..., 5] = -77.0  # regressed: must not be read
    par[..., 3] = rng.uniform(0.4, 0.6, (S, G))
    for col, hi in ((1, 0.8), (4, 0.3), (6, 0.15)):  # sv, sz, st: zero in group 1, nonzero in 2
        par[..., col] = rng.uniform(0.05, hi, (S, G))
        par[:, 1, col] = 0.0
    par[1, 0, 1] = par[2, 0, 6] = 0.0  # and mixed in the one-trial group
    return rt, X, gid, coef, par


@pytest.fixture(scope="module")
def base(gpu):
    """The data set and ONE debugging call on it, shared and left unchanged."""
    rt, X, gid, coef, par = _inputs()
    ds = gpu.RegDataset(rt, X, group_id=gid, n_groups=G)
    out, dbg = ds.gen_rts_drift(MODEL, coef, par, dt=DT, seed=SEED, return_debug=True)
    for a in (out, *dbg.values()):
        a.setflags(write=False)
    return dict(ds=ds, rt=rt, X=X, gid=gid, coef=coef, par=par, out=out, dbg=dbg)


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.gpu
def test_formed_parameters_are_the_likelihoods(base):
    """Per sweep, the parameters a lane forms are wiener_like_reg_groups'
    predicted arrays and, for the others, the trial's group row: bit for bit."""
    b = base
    assert b["out"].shape == (S, N) and b["dbg"]["params"].shape == (S, N, 7)
    for s in range(S):
        lik_rows = b["par"][s].copy()
        lik_rows[:, [0, 2, 5]] = 0.0
        _, _, pred = b["ds"].wiener_like_reg_groups(MODEL, b["coef"][s], lik_rows, terms=True)
        got = b["dbg"]["params"][s]
        for name, f in FIELD.items():
            want = pred[name] if name in pred else b["par"][s][b["gid"], f]
            assert np.array_equal(got[:, f], want), (s, name)
    assert np.all(b["dbg"]["params"][..., 2] > 0)


@pytest.mark.gpu
def test_draws_are_the_drift_samplers(gpu, base):
    """Row s equals draw s of each row of gen_rts_from_drift_nodes over the
    (n, 7) caller-order table of the formed parameters: the RTs and the start
    point, delay, drift and step count behind them."""
    b = base
    assert np.all(np.isfinite(b["out"]))
    for s in range(S):
        rts, off, dbg = gpu.gen_rts_from_drift_nodes(b["dbg"]["params"][s], s + 1, dt=DT,
                                                     seed=SEED, return_debug=True)
        pick = off[:-1] + s
        assert np.array_equal(b["out"][s], rts[pick]), s
        for k in ("y0", "delay", "drift", "n_steps"):
            assert np.array_equal(b["dbg"][k][s], dbg[k][pick]), (s, k)
    assert len({b["out"][s].tobytes() for s in range(S)}) == S


@pytest.mark.gpu
def test_launch_shape_grouping_and_tiling_change_nothing(gpu, base):
    b = base
    ds, coef, par = b["ds"], b["coef"], b["par"]
    assert np.array_equal(ds.gen_rts_drift(MODEL, coef, par, dt=DT, seed=SEED), b["out"])
    for wd in (64, 128, 1024):
        out, dbg = ds.gen_rts_drift(MODEL, coef, par, dt=DT, seed=SEED, wave_draws=wd,
                                    return_debug=True)
        assert np.array_equal(out, b["out"]), wd
        assert dbg["wave_steps"].shape == (-(-S * N // wd),) and np.all(dbg["wave_steps"] > 0)
        # a wave ran at least its longest walk and at most all of them
        assert 4 * -(-dbg["n_steps"].max() // 4) <= dbg["wave_steps"].max() <= dbg["n_steps"].sum()
    # sweeps in tiles of 1 and of 2 + 1
    for sweeps in (1, 2):
        out, dbg = ds.gen_rts_drift(MODEL, coef, par, dt=DT, seed=SEED,
                                    max_workspace=8 * N * sweeps, return_debug=True)
        assert np.array_equal(out, b["out"]), sweeps
        for k in ("params", "y0", "delay", "drift", "n_steps"):
            assert np.array_equal(dbg[k], b["dbg"][k]), (sweeps, k)
    # one group in the caller's order against three groups stored group-major,
    # the one row repeated for each group
    one = gpu.RegDataset(b["rt"], b["X"])
    flat = one.gen_rts_drift(MODEL, coef[:, 1:2], par[:, 1:2], dt=DT, seed=SEED)
    rep = ds.gen_rts_drift(MODEL, np.repeat(coef[:, 1:2], G, axis=1),
                           np.repeat(par[:, 1:2], G, axis=1), dt=DT, seed=SEED)
    assert np.array_equal(flat, rep)
    assert not np.array_equal(flat, b["out"])
    # a 2-D input is one sweep: sweep 0 of the stack
    assert np.array_equal(ds.gen_rts_drift(MODEL, coef[0], par[0], dt=DT, seed=SEED)[0],
                          b["out"][0])


@pytest.mark.gpu
def test_invalid_trials_are_nan_and_counted(gpu):
    """Value rows, as tests/test_invalid_rows.py: a <= 0 through the identity
    link in one (sweep, group), a NaN design value in one trial, walks cut at
    max_t. NaN exactly there, the unchanged bits everywhere else."""
    rt, X, gid, coef, par = _inputs(a_identity=True)
    good = gpu.RegDataset(rt, X, group_id=gid, n_groups=G)
    want, wdbg = good.gen_rts_drift(MODEL_A_IDENTITY, coef, par, dt=DT, seed=SEED,
                                    return_debug=True)
    assert np.all(np.isfinite(want))
    k = int(np.flatnonzero(gid == 1)[5])
    Xb, cb = X.copy(), coef.copy()
    Xb[k, 1] = np.nan
    cb[1, 2, 2] = -0.5  # X[:, 2] > 0: a <= 0 for every trial of group 2 in sweep 1
    mask = np.zeros((S, N), dtype=bool)
    mask[:, k] = True
    mask[1, gid == 2] = True
    bad = gpu.RegDataset(rt, Xb, group_id=gid, n_groups=G)
    got, dbg = bad.gen_rts_drift(MODEL_A_IDENTITY, cb, par, dt=DT, seed=SEED, invalid="nan",
                                 return_debug=True)
    assert np.array_equal(np.isnan(got), mask)
    assert np.array_equal(got[~mask], want[~mask])
    assert np.all(dbg["n_steps"][mask] == 0) and np.all(np.isnan(dbg["y0"][mask]))
    assert np.array_equal(dbg["n_steps"][~mask], wdbg["n_steps"][~mask])
    assert np.all(dbg["params"][1][gid == 2, 2] <= 0) and np.all(np.isnan(dbg["params"][:, k, 0]))
    with pytest.raises(RuntimeError, match=f"{mask.sum()} of {S * N}"):
        bad.gen_rts_drift(MODEL_A_IDENTITY, cb, par, dt=DT, seed=SEED)
    # the statistics entry counts them on the device alike
    with pytest.raises(RuntimeError, match=f"{mask.sum()} of {S * N}"):
        bad.gen_rts_drift_stats(MODEL_A_IDENTITY, cb, par, dt=DT, seed=SEED)
    # walks cut at max_t: the walks that need more than max_steps steps
    max_t = 0.3
    max_steps = int(np.ceil(max_t / DT))
    cut = wdbg["n_steps"] > max_steps
    assert 0 < cut.sum() < S * N
    got = good.gen_rts_drift(MODEL_A_IDENTITY, coef, par, dt=DT, seed=SEED, max_t=max_t,
                             unfinished="nan")
    assert np.array_equal(np.isnan(got), cut) and np.array_equal(got[~cut], want[~cut])
    with pytest.raises(RuntimeError, match=f"{cut.sum()} of {S * N} draws"):
        good.gen_rts_drift(MODEL_A_IDENTITY, coef, par, dt=DT, seed=SEED, max_t=max_t)
    # both kinds at once are counted apart: the invalid ones are reported first
    got = bad.gen_rts_drift(MODEL_A_IDENTITY, cb, par, dt=DT, seed=SEED, max_t=max_t,
                            unfinished="nan", invalid="nan")
    assert np.array_equal(np.isnan(got), mask | cut)
    with pytest.raises(RuntimeError, match=f"{(cut & ~mask).sum()} of {S * N} draws"):
        bad.gen_rts_drift(MODEL_A_IDENTITY, cb, par, dt=DT, seed=SEED, max_t=max_t, invalid="nan")


def _regrouped_stats(gpu, draws, gid, n_groups, quantiles):
    rows = [draws[s][gid == g] for s in range(draws.shape[0]) for g in range(n_groups)]
    off = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    return gpu.rt_stats_rows(np.concatenate(rows), off, quantiles).reshape(
        draws.shape[0], n_groups, -1)


@pytest.mark.gpu
def test_stats_are_the_statistics_of_the_draws(gpu, base):
    """gen_rts_drift_stats equals rt_stats_rows over gen_rts_drift's draws
    regrouped per (sweep, group); a group of 300 trials takes the block tier
    (kStatsWaveMax = 256), and tiling the sweeps changes nothing."""
    b = base
    q = (10, 30, 50, 70, 90)
    got, draws = b["ds"].gen_rts_drift_stats(MODEL, b["coef"], b["par"], dt=DT, seed=SEED,
                                             return_draws=True)
    assert got.shape == (S, G, 18) and np.array_equal(draws, b["out"])
    assert _eq(got, _regrouped_stats(gpu, b["out"], b["gid"], G, q))
    assert np.array_equal(got[..., 0], np.tile(SIZES, (S, 1)))
    assert _eq(got, b["ds"].gen_rts_drift_stats(MODEL, b["coef"], b["par"], dt=DT, seed=SEED,
                                                max_workspace=8 * N * 2))
    rng = np.random.default_rng(5)
    n2 = 305
    gid2 = rng.permutation(np.repeat([0, 1], [300, 5])).astype(np.int32)
    X2 = np.column_stack([np.ones(n2), rng.normal(size=n2), np.ones(n2), np.ones(n2)])
    ds2 = gpu.RegDataset(np.ones(n2), X2, group_id=gid2, n_groups=2)
    coef2, par2 = b["coef"][:2, :2], b["par"][:2, 1:]
    draws2 = ds2.gen_rts_drift(MODEL, coef2, par2, dt=DT, seed=3)
    got2 = ds2.gen_rts_drift_stats(MODEL, coef2, par2, dt=DT, seed=3, quantiles=(25, 75))
    assert got2.shape == (2, 2, 12)
    assert _eq(got2, _regrouped_stats(gpu, draws2, gid2, 2, (25, 75)))


@pytest.mark.gpu
def test_no_terms_and_an_empty_group(gpu, base):
    """Without a regression term every parameter is the group row's; a group
    without trials draws nothing and its statistics row is the empty one."""
    b = base
    ds = gpu.RegDataset(b["rt"], b["X"], group_id=b["gid"], n_groups=G + 1)
    par = np.zeros((S, G + 1, 8))
    par[..., :7] = b["dbg"]["params"][:, :G + 1]  # any valid rows
    out = ds.gen_rts_drift([], np.zeros((S, G + 1, C)), par, dt=DT, seed=SEED)
    for s in range(S):
        rts, off = gpu.gen_rts_from_drift_nodes(par[s][b["gid"]], s + 1, dt=DT, seed=SEED)
        assert np.array_equal(out[s], rts[off[:-1] + s]), s
    stats = ds.gen_rts_drift_stats([], np.zeros((S, G + 1, C)), par, dt=DT, seed=SEED)
    assert _eq(stats[:, :G], _regrouped_stats(gpu, out, b["gid"], G, (10, 30, 50, 70, 90)))
    assert np.all(stats[:, G, :3] == 0) and np.all(np.isnan(stats[:, G, 3:]))


def _model_data():
    import pandas as pd
    rng = np.random.default_rng(3)
    rows = []
    for s in range(4):
        x = rng.choice([-1.0, 1.0], 60, p=[0.3, 0.7]) * (0.3 + rng.gamma(2.0, 0.3, 60))
        rows.append(pd.DataFrame({"rt": x, "subj_idx": s, "cov": rng.normal(size=60)}))
    return pd.concat(rows, ignore_index=True).sample(frac=1.0, random_state=1).reset_index(
        drop=True)


@pytest.mark.gpu
@pytest.mark.parametrize("group_only", [True, False])
def test_model_posterior_predictive(gpu, group_only):
    """post_pred_gen is one gen_rts_drift call on post_pred_rows' tables, and
    post_pred_stats reduces the same draws."""
    from hddm_amd.regression import HDDMRegressor
    m = HDDMRegressor(_model_data(), ["v ~ 1 + cov", {"model": "a ~ 1", "link_func": "exp"}],
                      group_only_regressors=group_only, seed=0)
    m.sample(30, burn=10)
    frame = m.post_pred_gen(samples=5, seed=7)
    picked, B, P = m.post_pred_rows(5)
    n = len(m.data)
    assert picked.size == 5 and B.shape == (5, 4, 3) and P.shape == (5, 4, 8) and n == 240
    for j, nm in enumerate(m.coef_names):
        src = m.trace[nm][picked][:, None] if group_only else \
            m.trace_subj[nm][picked][:, m.node_subj]
        assert np.array_equal(B[:, :, j], np.broadcast_to(src, (5, 4)))
    assert list(frame.columns) == ["sample", "node", "trial", "rt", "response"]
    assert np.array_equal(frame["sample"], np.repeat(picked, n))
    assert np.array_equal(frame["trial"], np.tile(np.arange(n), 5))
    assert np.array_equal(frame["node"], np.tile(m.data["subj_idx"].to_numpy(), 5))
    assert np.array_equal(frame["response"], (frame["rt"] > 0).astype(np.int64))
    direct = m.dataset.gen_rts_drift(m.reg_model, B, P, seed=7)
    assert np.all(np.isfinite(direct))
    assert np.array_equal(frame["rt"].to_numpy().reshape(5, n), direct)
    table, sampled = m.post_pred_stats(samples=5, seed=7, return_sampled=True)
    assert _eq(sampled, _regrouped_stats(gpu, direct, m.node_codes, 4, (10, 30, 50, 70, 90)))
    assert set(table.index.get_level_values(0)) == {0, 1, 2, 3}
    with pytest.raises(NotImplementedError):
        m.optimize("gsquare")


# ------------------------------------------------------------------------ CPU

def test_entry_points_reject_null_and_empty_calls_without_gpu():
    from hddm_amd import _lib
    z = [None, None, None, 0, None, None, 1, DT, 1.0, 100, 0]
    assert _lib.wfpt_gen_rts_reg_drift(*z, None, None, None) == 2
    assert b"null" in _lib.wfpt_last_error()
    assert _lib.wfpt_gen_rts_reg_drift_ex(*z, 0, 0, *[None] * 9) == 2
    assert _lib.wfpt_gen_rts_reg_drift_stats(*z, 0, None, None, None, None, 0, None) == 2
    # S < 1 is refused before the context or the data set is looked at
    mem = ctypes.create_string_buffer(256)
    addr = ctypes.c_void_p(ctypes.addressof(mem))
    d = (ctypes.c_double * 8)()
    nun, ninv = ctypes.c_int64(), ctypes.c_int64()
    for S_bad in (0, -3):
        rc = _lib.wfpt_gen_rts_reg_drift(
            addr, addr, None, 0, d, ctypes.cast(d, _lib._PP), S_bad, DT, 1.0, 100, 0, d,
            ctypes.byref(nun), ctypes.byref(ninv))
        assert rc == 2 and b"S < 1" in _lib.wfpt_last_error()


def _bare_dataset():
    from hddm_amd import wfpt
    ds = object.__new__(wfpt.RegDataset)  # the checks below need neither device nor handle
    ds.n, ds.n_cols, ds.n_groups, ds.handle = N, C, G, None
    return ds


def test_python_argument_checks_without_gpu():
    ds = _bare_dataset()
    _, _, _, coef, par = _inputs()
    bad = [dict(coef_tables=coef[:, :2]), dict(coef_tables=coef[..., :3]),
           dict(coef_tables=coef[0, 0]), dict(params=par[:2]), dict(params=par[..., :7]),
           dict(params=par[0]),
           dict(model=[("v", 0, 2, "probit")]), dict(model=[("v", 3, 2, "identity")]),
           dict(dt=0.0), dict(dt=-1e-3), dict(dt=float("nan")), dict(intra_sv=0.0),
           dict(max_t=0.0), dict(unfinished="drop"), dict(invalid="drop"), dict(wave_draws=65),
           dict(max_workspace=-1)]
    for kw in bad:
        args = dict(model=MODEL, coef_tables=coef, params=par, dt=DT, seed=1)
        args.update(kw)
        with pytest.raises(ValueError):
            ds.gen_rts_drift(**args)
        with pytest.raises(ValueError):
            ds.gen_rts_drift_stats(**{k: v for k, v in args.items() if k != "wave_draws"},
                                   quantiles=(101,) if "wave_draws" in kw else (10, 90))


def test_model_refuses_the_cdf_method_without_gpu():
    from hddm_amd.regression import HDDMRegressor
    m = object.__new__(HDDMRegressor)
    # without a data set that has the trial-wise sampler the model refuses outright
    for name in ("post_pred_rows", "post_pred_gen", "post_pred_stats"):
        with pytest.raises(NotImplementedError, match="gen_rts_drift"):
            getattr(m, name)()
    m.dataset = _bare_dataset()  # has the sampler; the checks below never reach the device
    for meth in ("cdf", "nope"):
        with pytest.raises(ValueError, match="drift"):
            m.post_pred_gen(method=meth)
        with pytest.raises(ValueError, match="drift"):
            m.post_pred_stats(method=meth)
    with pytest.raises(RuntimeError, match="sample\\(\\) first"):
        m.post_pred_gen()
    with pytest.raises(NotImplementedError):
        m.optimize("gsquare")
