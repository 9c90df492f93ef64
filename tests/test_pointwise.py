"""The model-comparison pass: per-trial statistics over S
sweeps of log terms, reduced on the device next to the terms.

The update rule (hddm_amd/csrc/pointwise_update.hpp) is compiled here with g++
(tests/c/pointwise_host.cpp, contraction off) and
  * checked on the CPU against scipy's logsumexp and numpy's variance,
  * held bit for bit against the device pass on the GPU, for each of the three
    resident data-set kinds, fed with the terms their existing `trials=True` /
    `terms=True` calls return.
Every test here needs entry points the parent commit does not have.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from scipy.special import logsumexp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "pointwise_host.cpp")
_PD = ctypes.POINTER(ctypes.c_double)
_PI64 = ctypes.POINTER(ctypes.c_int64)
KN = dict(err=1e-4, n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, w_outlier=0.1)
FIELDS = ("lppd", "p_waic", "mean")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """terms (S, len) -> dict of lppd, p_waic, mean, n_inf by the host build."""
    so = str(tmp_path_factory.mktemp("pointwise") / "libpointwise_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                    "-shared", "-o", so, SRC, "-lm"], check=True)
    L = ctypes.CDLL(so)
    L.pointwise_host.restype = None
    L.pointwise_host.argtypes = [_PD, ctypes.c_int64, ctypes.c_int64, _PD, _PI64]

    def f(terms):
        lp = np.ascontiguousarray(terms, dtype=np.float64)
        S, n = lp.shape
        out = np.empty((3, n))
        ninf = np.empty(n, dtype=np.int64)
        L.pointwise_host(lp.ctypes.data_as(_PD), S, n, out.ctypes.data_as(_PD),
                         ninf.ctypes.data_as(_PI64))
        return {"lppd": out[0], "p_waic": out[1], "mean": out[2], "n_inf": ninf}
    return f


def _close(got, want, what):
    """1e-12 relative, floored at 1e-12 absolute."""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.abs(got - want) > 1e-12 * np.maximum(1.0, np.abs(want))
    assert not bad.any(), (what, got[bad][:3], want[bad][:3])


def _bits_equal(got, want, what):
    """Equal as int64 views, NaN equal to NaN."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    same = (got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(~same)
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _same_stats(pw, want, what):
    for f in FIELDS:
        _bits_equal(pw[f], want[f], f"{what}: {f}")
    assert np.array_equal(pw["n_inf"], want["n_inf"]), what


# ---------------------------------------------------------------- CPU: the rule

@pytest.mark.parametrize("S", [1, 2, 7, 33, 257])
def test_host_rule_against_logsumexp_and_variance(host, S):
    """Random terms at scales 1e-3 ... 300 around a negative level: lppd against
    scipy's logsumexp - log S, p_waic against numpy's sample variance, the mean
    against numpy's. In plain Python floats the recurrence stays within 1.3e-15
    (lppd) and 4.4e-15 (variance) over 10 000 such cases; 1e-12 is far above
    rounding and far below any ordering or indexing mistake."""
    rng = np.random.default_rng(1000 + S)
    for scale in (1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0, 300.0):
        lp = -2.0 * scale + scale * rng.normal(size=(S, 97))
        got = host(lp)
        _close(got["lppd"], logsumexp(lp, axis=0) - np.log(S), ("lppd", S, scale))
        want_var = np.var(lp, axis=0, ddof=1) if S > 1 else np.zeros(97)
        _close(got["p_waic"], want_var, ("p_waic", S, scale))
        _close(got["mean"], lp.mean(axis=0), ("mean", S, scale))
        assert not got["n_inf"].any()


def test_host_rule_edges(host):
    inf, nan = np.inf, np.nan
    lp = np.array([[-1.0, -inf, -1.0, -3.0, 0.5],
                   [-inf, -inf, nan, -2.0, -0.5],
                   [-2.0, -inf, -1.5, -inf, 0.25]])
    got = host(lp)
    assert got["n_inf"].tolist() == [1, 3, 0, 1, 0]
    # a -inf term only counts: trial 0 is the two finite terms over S = 3 sweeps
    fin = np.array([-1.0, -2.0])
    _close(got["lppd"][0], logsumexp(fin) - np.log(3), "lppd with a zero density")
    _close(got["p_waic"][0], np.var(fin, ddof=1), "p_waic with a zero density")
    _close(got["mean"][0], fin.mean(), "mean with a zero density")
    # no finite term at all
    assert got["lppd"][1] == -inf and got["mean"][1] == -inf and np.isnan(got["p_waic"][1])
    # a NaN term poisons the trial
    assert np.isnan(got["lppd"][2]) and np.isnan(got["p_waic"][2]) and np.isnan(got["mean"][2])
    # one finite pair
    _close(got["lppd"][3], logsumexp([-3.0, -2.0]) - np.log(3), "trial 3")
    # S = 1: no variance
    one = host(lp[:1])
    assert one["p_waic"][0] == 0.0 and one["lppd"][0] == -1.0 and one["mean"][0] == -1.0
    assert one["lppd"][1] == -inf and np.isnan(one["p_waic"][1])
    # rising and falling terms take both branches of the maximum update
    _close(got["lppd"][4], logsumexp(lp[:, 4]) - np.log(3), "trial 4")


def test_host_rule_constant_terms(host):
    """Terms that do not vary over the sweeps: p_waic is exactly 0, the mean
    exactly the term, and lppd the term (m + log 8 - log 8, two roundings)."""
    lp = np.tile(np.array([-0.3, -7.25, -123.5]), (8, 1))
    got = host(lp)
    assert np.all(got["p_waic"] == 0.0)
    assert np.array_equal(got["mean"], lp[0])
    _close(got["lppd"], lp[0], "lppd of constant terms")


def test_new_entries_reject_null_arguments_without_gpu():
    from hddm_amd import _lib
    assert _lib.wfpt_pointwise_nodes(None, None, None, 1, None, 0, None, None, None) == 2
    assert b"null" in _lib.wfpt_last_error()
    assert _lib.wfpt_pointwise_rlddm_nodes(None, None, None, None, 1, None, 0, None, None, None,
                                           None) == 2
    assert _lib.wfpt_pointwise_reg_groups(None, None, None, 0, None, None, 1, None, 0, None, None,
                                          None) == 2
    assert _lib.wfpt_pointwise_profile(None, None, 0) == 2


# ---------------------------------------------------------------- GPU: plain nodes

NODE_SIZES = (1, 63, 65, 257)  # n = 386: crosses a wave and a 256-lane block, a multiple of neither


def _node_data(seed=7):
    rng = np.random.default_rng(seed)
    node = rng.permutation(np.repeat(np.arange(4), NODE_SIZES)).astype(np.int32)
    n = node.size
    rt = rng.uniform(0.45, 2.5, n) * np.where(rng.random(n) < 0.7, 1.0, -1.0)
    return rt, node


def _tables(S, full, p_outlier=0.05, seed=3):
    """(S, 4, 8): the drift changes sign over the sweeps, so a trial's term
    rises and falls and both branches of the maximum update run."""
    rng = np.random.default_rng(seed + 10 * S + full)
    P = np.empty((S, 4, 8))
    s = np.arange(S)[:, None]
    P[:, :, 0] = 1.6 * np.cos(2.1 * s + np.arange(4)) + rng.normal(0, 0.2, (S, 4))
    P[:, :, 2] = rng.uniform(1.4, 2.3, (S, 4))
    P[:, :, 3] = 0.5
    P[:, :, 5] = rng.uniform(0.2, 0.3, (S, 4))
    P[:, :, 1] = rng.uniform(0.1, 1.0, (S, 1)) if full else 0.0
    P[:, :, 4] = rng.uniform(0.05, 0.3, (S, 1)) if full else 0.0
    P[:, :, 6] = rng.uniform(0.05, 0.2, (S, 1)) if full else 0.0
    P[:, :, 7] = p_outlier
    return P


@pytest.fixture(scope="module")
def node_ds(gpu):
    rt, node = _node_data()
    return gpu.Dataset(rt, node_id=node, n_nodes=4), rt, node


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["simple", "full"])
@pytest.mark.parametrize("S", [1, 2, 7, 33])
def test_nodes_bitwise_against_host_and_tiling(node_ds, host, S, full):
    ds, rt, node = node_ds
    tabs = _tables(S, full)
    sums, terms = ds.wiener_like_nodes_multi(tabs, trials=True, **KN)
    if S > 1:  # the terms rise and fall over the sweeps
        assert np.any(np.diff(terms, axis=0) > 0) and np.any(np.diff(terms, axis=0) < 0)
    want = host(terms)
    pw = ds.pointwise_nodes(tabs, **KN)
    assert pw["sums"].shape == (S, 4)
    _bits_equal(pw["sums"], sums, "sums")
    _same_stats(pw, want, f"S={S} full={full}")
    assert np.array_equal(pw["trial"], np.arange(rt.size))
    assert pw["n_inf_total"] == 0 and np.all(np.isfinite(pw["lppd"]))
    if S in (7, 33):  # 1 and 3 sweeps per tile (3: a ragged last tile for S = 7)
        for per_tile in (1, 3):
            tiled = ds.pointwise_nodes(tabs, max_workspace=8 * rt.size * per_tile, **KN)
            _bits_equal(tiled["sums"], pw["sums"], f"sums, {per_tile} per tile")
            _same_stats(tiled, pw, f"{per_tile} sweeps per tile")


@pytest.mark.gpu
def test_nodes_zero_densities(gpu, host):
    """p_outlier = 0: a trial at or below its node's t has a zero density. t
    rises above some |rt| in some sweeps and above one trial's |rt| in all."""
    rt, node = _node_data(seed=11)
    near = np.abs(np.abs(rt) - 0.9) < 0.05  # keep clear of t = 0.9: a density a hair above t
    rt[near] = np.sign(rt[near])            # underflows to zero by itself
    rt[5] = np.sign(rt[5]) * 0.05  # below every t: no sweep gives it a density
    S = 9
    tabs = _tables(S, False, p_outlier=0.0)
    tabs[:, :, 5] = np.where(np.arange(S)[:, None] % 3 == 1, 0.9, 0.2)  # 0.9 > many |rt|
    tabs[4, :, 5] = 3.0  # above every |rt|: a sweep of zero densities only
    ds = gpu.Dataset(rt, node_id=node, n_nodes=4)
    pw = ds.pointwise_nodes(tabs, **KN)
    want_ninf = np.sum(np.abs(rt)[None, :] < tabs[:, node, 5], axis=0)
    assert np.array_equal(pw["n_inf"], want_ninf)
    assert pw["n_inf_total"] == int(want_ninf.sum())
    assert want_ninf[5] == S and want_ninf.min() == 1 and np.sum(want_ninf == 3) > 50
    alive = want_ninf < S
    assert np.all(np.isfinite(pw["lppd"][alive])) and np.all(np.isfinite(pw["mean"][alive]))
    assert pw["lppd"][5] == -np.inf and pw["mean"][5] == -np.inf and np.isnan(pw["p_waic"][5])
    sums, terms = ds.wiener_like_nodes_multi(tabs, trials=True, **KN)
    _bits_equal(pw["sums"], sums, "sums")
    _same_stats(pw, host(terms), "zero densities")
    tiled = ds.pointwise_nodes(tabs, max_workspace=8 * rt.size * 2, **KN)
    _same_stats(tiled, pw, "zero densities, 2 sweeps per tile")
    assert tiled["n_inf_total"] == pw["n_inf_total"]


@pytest.mark.gpu
def test_nodes_shape_errors(gpu, node_ds):
    ds, rt, _ = node_ds
    with pytest.raises(ValueError, match="node ids"):
        gpu.Dataset(rt).pointwise_nodes(_tables(2, False), **KN)
    for bad in (_tables(2, False)[:, :3], _tables(2, False)[0], np.empty((0, 4, 8)),
                np.zeros((2, 4, 7))):
        with pytest.raises(ValueError, match=r"\(S, 4, 8\)"):
            ds.pointwise_nodes(bad, **KN)


# ---------------------------------------------------------------- GPU: the RL node batch

def _rl_data():
    """3 nodes x 2 conditions with segments of 1, 2 and 70 trials, interleaved."""
    rng = np.random.default_rng(23)
    lengths = {(0, 0): 1, (0, 1): 70, (1, 0): 2, (1, 1): 70, (2, 0): 70, (2, 1): 2}
    node = np.concatenate([np.full(k, nd) for (nd, _), k in lengths.items()])
    split = np.concatenate([np.full(k, c) for (_, c), k in lengths.items()])
    order = rng.permutation(node.size)
    node, split = node[order].astype(np.int32), split[order].astype(np.int64)
    n = node.size
    rt = rng.uniform(0.5, 2.0, n) * np.where(rng.random(n) < 0.6, 1.0, -1.0)
    response = (rt > 0).astype(np.int64)
    feedback = rng.integers(0, 2, n).astype(np.float64)
    return rt, response, feedback, split, node


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 5])
def test_rl_nodes_bitwise_against_host(gpu, host, S):
    rt, response, feedback, split, node = _rl_data()
    ds = gpu.RLDataset(rt, response, feedback, split, node_id=node, n_nodes=3)
    rng = np.random.default_rng(40 + S)
    rl = np.empty((S, 3, 3))
    rl[:, :, 0] = 0.5
    rl[:, :, 1] = rng.normal(0.0, 1.0, (S, 3))
    rl[:, :, 2] = 100.0
    P = _tables(S, False)[:, :3].copy()
    P[:, :, 0] = 2.5 * np.cos(1.9 * np.arange(S)[:, None] + np.arange(3))  # the drift scaling
    sums, terms, _ = ds.wiener_like_rlddm_nodes_multi(rl, P, terms=True, **KN)
    pw = ds.pointwise_rlddm_nodes(rl, P, **KN)
    # exactly the non-first trial of each (node, condition) segment
    first = {}
    for i in range(rt.size):
        first.setdefault((node[i], split[i]), i)
    scored = np.array(sorted(set(range(rt.size)) - set(first.values())))
    assert scored.size == rt.size - 6 and ds.n_scored == scored.size
    assert np.array_equal(np.sort(pw["trial"]), scored)
    _bits_equal(pw["sums"], sums, "sums")
    _same_stats(pw, host(terms[:, pw["trial"]]), f"RL S={S}")
    if S == 5:
        tiled = ds.pointwise_rlddm_nodes(rl, P, max_workspace=8 * scored.size * 2, **KN)
        _bits_equal(tiled["sums"], pw["sums"], "sums, 2 sweeps per tile")
        _same_stats(tiled, pw, "RL, 2 sweeps per tile")
        assert np.array_equal(tiled["trial"], pw["trial"])


@pytest.mark.gpu
def test_rl_shape_errors(gpu):
    rt, response, feedback, split, node = _rl_data()
    with pytest.raises(ValueError, match="node ids"):
        gpu.RLDataset(rt, response, feedback, split).pointwise_rlddm_nodes(
            np.zeros((1, 3, 3)), np.zeros((1, 3, 8)), **KN)
    ds = gpu.RLDataset(rt, response, feedback, split, node_id=node, n_nodes=3)
    with pytest.raises(ValueError, match=r"\(S, 3, 3\)"):
        ds.pointwise_rlddm_nodes(np.zeros((3, 3)), np.zeros((1, 3, 8)), **KN)
    with pytest.raises(ValueError, match=r"\(2, 3, 8\)"):
        ds.pointwise_rlddm_nodes(np.zeros((2, 3, 3)), np.zeros((1, 3, 8)), **KN)


# ---------------------------------------------------------------- GPU: regression groups

REG_MODEL = [("v", 0, 2, "identity"), ("a", 2, 1, "exp")]


def _reg_data():
    rng = np.random.default_rng(31)
    group = rng.permutation(np.repeat(np.arange(3), (1, 64, 130))).astype(np.int32)
    n = group.size
    rt = rng.uniform(0.5, 2.2, n) * np.where(rng.random(n) < 0.65, 1.0, -1.0)
    X = np.column_stack([np.ones(n), rng.normal(size=n), np.ones(n)])
    return rt, X, group


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 4])
def test_reg_groups_bitwise_against_host(gpu, host, S):
    rt, X, group = _reg_data()
    ds = gpu.RegDataset(rt, X, group_id=group, n_groups=3)
    rng = np.random.default_rng(50 + S)
    B = np.empty((S, 3, 3))
    B[:, :, 0] = 1.2 * np.cos(2.3 * np.arange(S)[:, None] + np.arange(3))  # the sign changes
    B[:, :, 1] = rng.normal(0, 0.4, (S, 3))
    B[:, :, 2] = rng.uniform(0.4, 0.8, (S, 3))  # a = exp(.)
    P = _tables(S, True)[:, :3].copy()
    each = [ds.wiener_like_reg_groups(REG_MODEL, B[s], P[s], terms=True, **KN) for s in range(S)]
    pw = ds.pointwise_reg_groups(REG_MODEL, B, P, **KN)
    assert pw["sums"].shape == (S, 3)
    _bits_equal(pw["sums"], np.stack([e[0] for e in each]), "sums")
    _same_stats(pw, host(np.stack([e[1] for e in each])), f"regression S={S}")
    assert np.array_equal(pw["trial"], np.arange(rt.size))


@pytest.mark.gpu
def test_reg_shape_errors(gpu):
    rt, X, group = _reg_data()
    ds = gpu.RegDataset(rt, X, group_id=group, n_groups=3)
    with pytest.raises(ValueError, match=r"\(S, 3, 3\)"):
        ds.pointwise_reg_groups(REG_MODEL, np.zeros((3, 3)), np.zeros((1, 3, 8)), **KN)
    with pytest.raises(ValueError, match=r"\(2, 3, 8\)"):
        ds.pointwise_reg_groups(REG_MODEL, np.zeros((2, 3, 3)), np.zeros((2, 3, 7)), **KN)
