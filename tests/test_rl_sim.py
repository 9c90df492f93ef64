"""The closed-loop RLDDM simulator (wfpt_gen_rlddm_rows, rl_sim_kernel;
hddm/generate.py:430-516 and its one-step-ahead form, generate.py:608-661) and
what is built on it: gen_rl_data(closed_loop='device'), HDDMrl.post_pred_sim.

Reference: the loop restated below, trial after trial, from pieces that are
pinned elsewhere -- test_drift's walk and Philox streams (pinned to a recorded
run of the reference), test_sim's uniforms, and the Q update of
test_rl.restate_rlddm in plain Python floats. dt = 1e-3 and a in 0.1 .. 1.5
throughout: a walk is a few to a few hundred steps. Tolerances:
  * rt, start point, delay, steps, feedback, Q values, sim_drift: none
    (assert_array_equal), the walk fed the device's own per-trial drift as
    test_drift.restate allows;
  * the walk's drift minus sim_drift against sv times the host Box-Muller:
    relative 1e-13, test_drift's bound for the same reason (the device's log,
    cos and sqrt are each a few ulp from glibc's);
  * the distribution check (g): a two-sample bound of 4.5 standard errors of
    the difference of the means over 1500 independent sequences each, false
    alarm rate about 7e-6 before the seeds were fixed.
"""
import ctypes

import numpy as np
import pytest

from test_drift import PhiloxSteps, philox_normal, restate, walk
from test_rl import E, restate_rlddm
from test_sim import philox_uniform

DT = 1e-3
STREAM_UP, STREAM_LOW = 5, 6
NEVER = np.iinfo(np.int64).max
# v (drift scaling), sv, a, z, sz, t, st | q, alpha, pos_alpha | p_upper, p_lower
KINDS = np.array([
    (2.0, 0.0, 1.0, 0.5, 0.0, 0.3, 0.0, 0.5, -0.5, 100.0, 0.8, 0.2),      # plain
    (1.5, 0.3, 1.2, 0.5, 0.1, 0.3, 0.1, 0.5, 0.2, 100.0, 0.7, 0.3),       # sv, sz, st
    (2.5, 0.0, 0.8, 0.45, 0.0, 0.25, 0.0, 0.4, -1.2, 0.4, 0.8, 0.2),      # two learning rates
    (2.0, 0.0, 0.1, 0.5, 0.2, 0.3, 0.0, 0.5, 0.3, 100.0, 0.6, 0.4),       # a = 0.1: a few steps
    (1.0, 0.0, 1.0, 0.021, 0.04, 0.2, 0.0, 0.5, 0.0, 100.0, 0.75, 0.25),  # crossings on step 0
    (2.0, 0.0, 0.6, 0.5, 0.0, 0.3, 0.0, 0.5, -0.3, 100.0, 1.0, 0.0),      # p = (1, 0)
    (3.0, 0.0, 1.5, 0.5, 0.0, 0.3, 0.0, 0.5, 0.5, 100.0, 0.5, 0.5),       # p = (0.5, 0.5)
])
COUNTS = (0, 1, 2, 5, 9, 33)
R_A, SEED_A = 70, 0x51ED270B7F4A7C15


def tables(R):
    K = KINDS[np.arange(R) % len(KINDS)]
    cnt = np.array([COUNTS[r % len(COUNTS)] for r in range(R)], dtype=np.int64)
    return K[:, :7].copy(), K[:, 7:10].copy(), K[:, 10:].copy(), cnt


# ---------------------------------------------------------------- restatement

def rate(alpha):
    return (E ** alpha) / (1 + E ** alpha)


def restate_loop(P, RL, counts, seed, rewards=None, arrays=None, observed=None, start=None,
                 dt=DT, intra_sv=1.0, max_steps=20000, row0=0, drift=None, learn=True):
    """What the device call returns, row after row: a dict of per-trial rt,
    feedback, q_up, q_low, sim_drift, drift (the host Box-Muller's), y0, delay,
    n_steps. The rows advance in lockstep, trial k of all rows that have one.
    drift: per-trial rates to walk with instead of the host's. learn=False
    leaves Q alone (the loop is then test_drift.restate with draw = trial)."""
    P, RL = np.asarray(P, dtype=np.float64), np.asarray(RL, dtype=np.float64)
    R = P.shape[0]
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), (R,))
    off = np.r_[0, np.cumsum(counts)]
    start = off[:-1] if start is None else np.asarray(start)
    out = {k: np.full(off[-1], np.nan) for k in ("rt", "feedback", "q_up", "q_low", "sim_drift",
                                                 "drift", "y0", "delay")}
    out["n_steps"] = np.zeros(off[-1], dtype=np.int64)
    q_up, q_low = [float(q) for q in RL[:, 0]], [float(q) for q in RL[:, 0]]
    neg = [rate(float(al)) for al in RL[:, 1]]
    pos = [neg[r] if RL[r, 2] == 100.0 else rate(float(RL[r, 2])) for r in range(R)]
    alive = np.ones(R, dtype=bool)
    for k in range(int(counts.max()) if R else 0):
        idx = np.nonzero(alive & (counts > k))[0]
        if idx.size == 0:
            break
        e, row = off[idx] + k, idx + row0
        draw = np.full(idx.shape, k)
        v, sv, a, z, sz, t, st = (np.ascontiguousarray(P[idx, i]) for i in range(7))
        qu, ql = np.array([q_up[r] for r in idx]), np.array([q_low[r] for r in idx])
        sim_drift = (qu - ql) * v
        u_t = np.where(st != 0, philox_uniform(seed, row, draw, 1), 0.0)
        u_z = np.where(sz != 0, philox_uniform(seed, row, draw, 2), 0.0)
        delay = (t + st * u_t) - st / 2.
        y0 = ((z + sz * u_z) - sz / 2.) * a
        host = np.where(sv != 0, sim_drift + sv * philox_normal(seed, row, draw, 3), sim_drift)
        d = host if drift is None else drift[e]
        rt, steps = walk(a, y0, delay, d, d, np.full(idx.shape, NEVER), dt, intra_sv, max_steps,
                         PhiloxSteps(seed, row, draw))
        for name, val in (("rt", rt), ("q_up", qu), ("q_low", ql), ("sim_drift", sim_drift),
                          ("drift", host), ("y0", y0), ("delay", delay), ("n_steps", steps)):
            out[name][e] = val
        for i, r in enumerate(idx):
            if np.isnan(rt[i]):  # a cut walk ends its sequence
                alive[r] = False
                continue
            up = bool(rt[i] > 0)
            s = int(start[r]) + k
            if observed is not None:
                up, f = bool(observed[0][s]), float(observed[1][s])
            elif arrays is not None:
                f = float(arrays[0 if up else 1][s])
            else:
                u = philox_uniform(seed, row[i], k, STREAM_UP if up else STREAM_LOW)
                f = 1.0 if float(u) < rewards[r][0 if up else 1] else 0.0
            out["feedback"][e[i]] = f
            if learn:  # test_rl.restate_rlddm's lines (wfpt.pyx:145-153)
                q = q_up[r] if up else q_low[r]
                alfa = pos[r] if f > q else neg[r]
                q = q + alfa * (f - q)
                if up:
                    q_up[r] = q
                else:
                    q_low[r] = q
    return out


# --------------------------------------------------------------------------- CPU

def test_restatement_without_learning_is_the_open_loop_restatement():
    """With the Q update switched off the drift stays (q - q) * v = 0 and the
    loop is test_drift.restate (pinned to the reference fixture) at v = 0 with
    the draw index in the trial's place."""
    P, RL, p, cnt = tables(14)
    cnt = np.minimum(cnt, 9)
    got = restate_loop(P, RL, cnt, 99, rewards=p, row0=3, learn=False)
    P0 = P.copy()
    P0[:, 0] = 0.0
    want = restate(P0, None, cnt, 99, dt=DT, row0=3)
    for k in ("rt", "y0", "delay", "drift", "n_steps"):
        np.testing.assert_array_equal(got[k], want[k])
    assert np.all(got["sim_drift"] == 0) and cnt.sum() > 20


def test_python_argument_checks_without_gpu(monkeypatch):
    from hddm_amd import _lib, wfpt

    def no_context(*a, **k):
        raise AssertionError("a context was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "context", no_context)
    assert "gen_rlddm_rows" in wfpt.__all__ and "gen_rlddm_stats_rows" in wfpt.__all__
    P, RL, p, _ = tables(2)
    f = wfpt.gen_rlddm_rows
    rew = (np.zeros(10), np.ones(10))
    obs = (np.zeros(10, dtype=np.int64), np.ones(10))
    bad = [
        dict(params=np.zeros((2, 6))), dict(rl_rows=RL[:1]), dict(rl_rows=np.zeros((2, 2))),
        dict(rl_rows=np.array([[0.5, np.nan, 100.0]] * 2)),
        dict(n_trials=[5, 4, 3]), dict(n_trials=[5, -1]),
        dict(rewards=None), dict(reward_arrays=rew), dict(observed=obs),  # none / two sources
        dict(rewards=[0.5, 1.5]), dict(rewards=[-0.1, 0.5]), dict(rewards=[np.nan, 0.5]),
        dict(rewards=np.zeros((3, 2))),
        dict(rewards=None, reward_arrays=(np.zeros(10), np.ones(9))),
        dict(rewards=None, reward_arrays=(np.zeros(9), np.ones(9))),   # 2 x 5 trials do not fit
        dict(rewards=None, reward_arrays=rew + ([0, 6],)),             # row 1 reads past the end
        dict(rewards=None, reward_arrays=rew + ([0, -1],)),
        dict(rewards=None, reward_arrays=rew + ([0],)),
        dict(rewards=None, observed=(obs[0],)),
        dict(row0=-1), dict(row0=2 ** 31 - 1), dict(dt=0.0), dict(intra_sv=0.0),
        dict(unfinished="ignore"), dict(wave_rows=100), dict(dt=1e-9, max_t=20.)]
    for kw in bad:
        args = dict(params=P, rl_rows=RL, n_trials=5, rewards=p)
        args.update(kw)
        with pytest.raises(ValueError):
            f(**args)
    with pytest.raises(ValueError):
        wfpt.gen_rlddm_stats_rows(P, RL, 5, [0, 1], rewards=p)  # groups must end at R
    with pytest.raises(ValueError):
        wfpt.gen_rlddm_stats_rows(P, RL, 5, [0, 2], rewards=p, quantiles=[101])
    for good in (dict(rewards=p), dict(reward_arrays=rew), dict(observed=obs + ([0, 5],)),
                 dict(reward_arrays=rew + ([5, 5],))):
        with pytest.raises(AssertionError):  # valid arguments do reach the context
            f(P, RL, 5, dt=DT, **good)
    with pytest.raises(AssertionError):
        wfpt.gen_rlddm_stats_rows(P, RL, 5, [0, 0, 2], rewards=p)


def test_entry_points_reject_bad_arguments_without_gpu():
    from hddm_amd import _lib
    two = 2
    assert _lib.wfpt_gen_rlddm_rows(None, None, None, 0, None, None, 1e-3, 1.0, 10, 0, None,
                                    None) == two
    assert b"null" in _lib.wfpt_last_error()
    assert _lib.wfpt_gen_rlddm_rows_ex(None, None, None, 0, None, None, 1e-3, 1.0, 10, 0, 0, 0,
                                       *[None] * 11) == two
    assert b"null" in _lib.wfpt_last_error()
    assert _lib.wfpt_gen_rlddm_rows_stats(None, None, None, 0, None, None, 1e-3, 1.0, 10, 0, None,
                                          None, None, 0, None, 0, None) == two
    assert b"null" in _lib.wfpt_last_error()
    P = np.zeros((2, 8))
    P[:, :7] = KINDS[:2, :7]
    RL = KINDS[:2, 7:10].copy()
    p = KINDS[:2, 10:].copy()
    cnt = np.array([3, 2], dtype=np.int64)
    out, nun = np.empty(5), np.zeros(1, dtype=np.int64)
    rew, resp = np.zeros(5), np.zeros(5, dtype=np.int64)
    stats, q = np.empty((1, 10)), np.array([50.0])
    addr = lambda a: a.ctypes.data

    def call(kind="", src=None, R=2, counts=cnt, rows=P, rl=RL, dt=1e-3, intra_sv=1.0,
             max_steps=10, row0=0, wave_rows=0, goff=(0, 2)):
        s = _lib.RlSource()
        for k, v in (dict(p=addr(p)) if src is None else src).items():
            setattr(s, k, v)
        head = (None, rows.ctypes.data_as(_lib._PP), _lib.dptr(rl), R,
                counts.ctypes.data_as(_lib._PI64), ctypes.byref(s), dt, intra_sv, max_steps, 0)
        tail = (_lib.dptr(out), nun.ctypes.data_as(_lib._PI64))
        if kind == "ex":
            return _lib.wfpt_gen_rlddm_rows_ex(*head, row0, wave_rows, *tail, *[None] * 9)
        if kind == "stats":
            g = np.array(goff, dtype=np.int64)
            return _lib.wfpt_gen_rlddm_rows_stats(*head, *tail, g.ctypes.data_as(_lib._PI64),
                                                  g.size - 1, _lib.dptr(q), 1, _lib.dptr(stats))
        return _lib.wfpt_gen_rlddm_rows(*head, *tail)

    nan_rl, far_p, bad_row = RL.copy(), p.copy(), P.copy()
    nan_rl[1, 0] = np.nan
    far_p[1, 1] = 1.5
    bad_row[1, 2] = 0.0
    arrays = dict(rew_up=addr(rew), rew_low=addr(rew), n=5)
    past_end, before_start = np.array([0, 4], dtype=np.int64), np.array([-1, 0], dtype=np.int64)
    cases = [
        ({}, b"context"), ({"R": 0}, b"R < 1"), ({"dt": 0.0}, b"dt <= 0"),
        ({"dt": float("nan")}, b"dt <= 0"), ({"intra_sv": 0.0}, b"intra_sv"),
        ({"max_steps": 0}, b"max_steps"), ({"max_steps": 2 ** 31 + 1}, b"max_steps"),
        ({"counts": np.array([3, -1], dtype=np.int64)}, b"negative count"),
        ({"rl": nan_rl}, b"NaN in RL row 1"),
        ({"src": {}}, b"exactly one reward source"),
        ({"src": dict(p=addr(p), **arrays)}, b"exactly one reward source"),
        ({"src": dict(arrays, obs_response=addr(resp), obs_feedback=addr(rew))},
         b"exactly one reward source"),
        ({"src": dict(rew_up=addr(rew), n=5)}, b"null pointer"),
        ({"src": dict(obs_feedback=addr(rew), n=5)}, b"null pointer"),
        ({"src": dict(arrays, n=4)}, b"row 1 reads"),
        ({"src": dict(arrays, n=-1)}, b"negative length"),
        ({"src": dict(arrays, start=addr(past_end))}, b"row 1 reads"),
        ({"src": dict(arrays, start=addr(before_start))}, b"row 0 reads"),
        ({"src": arrays}, b"context"),
        ({"src": dict(obs_response=addr(resp), obs_feedback=addr(rew), n=5)}, b"context"),
    ]
    for kind in ("", "ex", "stats"):
        for kw, msg in cases:
            assert call(kind, **kw) == two, (kind, kw)
            assert msg in _lib.wfpt_last_error(), (kind, kw, _lib.wfpt_last_error())
        assert call(kind, src={"p": addr(far_p)}) == two
        assert b"outside [0, 1] in row 1" in _lib.wfpt_last_error()
        assert call(kind, rows=bad_row) == 4  # the drift sampler's row check, naming the row
        assert b"row 1 cannot be simulated" in _lib.wfpt_last_error()
    for kw, msg in (({"row0": -1}, b"row0"), ({"row0": 2 ** 31 - 1}, b"row0"),
                    ({"row0": 2 ** 31 - 2}, b"context"), ({"wave_rows": 100}, b"wave_rows"),
                    ({"wave_rows": -64}, b"wave_rows")):
        assert call("ex", **kw) == two, kw
        assert msg in _lib.wfpt_last_error(), (kw, _lib.wfpt_last_error())
    for goff, msg in (((0, 1), b"from 0 to R"), ((1, 2), b"from 0 to R"),
                      ((0, 2, 1, 2), b"falls"), ((0, 2), b"context"), ((0, 0, 2, 2), b"context")):
        assert call("stats", goff=goff) == two, goff
        assert msg in _lib.wfpt_last_error(), (goff, _lib.wfpt_last_error())


def test_the_data_only_predictive_still_refuses_and_names_the_simulator(monkeypatch):
    from hddm_amd import rl
    from test_hddmrl import _OracleRLDataset, _cpu_data
    monkeypatch.setattr(rl._wfpt, "RLDataset", _OracleRLDataset)
    data, _ = _cpu_data(n_subj=2, n=6)
    m = rl.HDDMrl(data, seed=0)
    for call in (m.post_pred_rows, m.post_pred_gen, m.post_pred_stats):
        with pytest.raises(NotImplementedError, match="post_pred_sim"):
            call()
    with pytest.raises(RuntimeError):  # no traces yet
        m.post_pred_sim({0: (0.8, 0.2), 1: (0.7, 0.3)})
    with pytest.raises(ValueError):
        rl.gen_rl_data(1, 2, {0: (0.8, 0.2)}, a=1.0, t=0.3, v=2.0, alpha=0.0, closed_loop="gpu")


# --------------------------------------------------------------------------- GPU

_LOOP = {}


def loop_a(gpu):
    """Test (a)'s device call and its restatement, computed once."""
    if not _LOOP:
        P, RL, p, cnt = tables(R_A)
        rts, off, d = gpu.gen_rlddm_rows(P, RL, cnt, rewards=p, dt=DT, seed=SEED_A,
                                         return_debug=True)
        host = restate_loop(P, RL, cnt, SEED_A, rewards=p, drift=d["drift"])
        _LOOP.update(P=P, RL=RL, p=p, cnt=cnt, rts=rts, off=off, d=d, host=host)
    return _LOOP


EXACT = ("y0", "delay", "n_steps", "feedback", "q_up", "q_low", "sim_drift")


def assert_loop_equal(rts, d, host, sv):
    np.testing.assert_array_equal(rts, host["rt"])
    for k in EXACT:
        np.testing.assert_array_equal(d[k], host[k], err_msg=k)
    # the normal draw alone: sv * n, n a few ulp from the host's Box-Muller
    np.testing.assert_allclose(d["drift"] - d["sim_drift"], host["drift"] - host["sim_drift"],
                               rtol=1e-13, atol=0)
    assert np.all((d["drift"] == d["sim_drift"])[sv == 0])


@pytest.mark.gpu
def test_device_loop_equals_restatement(gpu):
    """(a) 70 rows (a full wave, a partial one, rows handed on as lanes end)
    of every kind and length, bit for bit; a slice of the table under row0;
    another wave range."""
    L = loop_a(gpu)
    P, RL, p, cnt, rts, off, d, host = (L[k] for k in ("P", "RL", "p", "cnt", "rts", "off", "d",
                                                       "host"))
    np.testing.assert_array_equal(off, np.r_[0, np.cumsum(cnt)])
    assert not np.isnan(rts).any() and rts.size == cnt.sum()
    kind = np.repeat(np.arange(R_A) % len(KINDS), cnt)
    assert_loop_equal(rts, d, host, np.repeat(P[:, 1], cnt))
    # the cases the rows were chosen for did occur
    assert d["n_steps"][kind == 4].min() == 1 and d["n_steps"][kind == 3].max() <= 40
    assert np.all(d["feedback"][(kind == 5) & (rts > 0)] == 1.0)
    assert np.all(d["feedback"][(kind == 5) & (rts < 0)] == 0.0)
    assert set(np.unique(d["feedback"][kind == 6])) == {0.0, 1.0}
    first = np.zeros(rts.size, dtype=bool)
    first[off[:-1][cnt > 0]] = True
    assert np.all(d["sim_drift"][first] == 0) and np.mean(d["sim_drift"][~first] != 0) > 0.9
    assert np.any(d["q_up"] != d["q_up"][0]) and np.any(d["q_low"] != d["q_low"][0])
    assert np.any((rts > 0) & (d["feedback"] == 0)) and np.any((rts < 0) & (d["feedback"] == 1))
    # rows 7 .. of the table, called alone with row0 = 7
    own, off7, d7 = gpu.gen_rlddm_rows(P[7:], RL[7:], cnt[7:], rewards=p[7:], dt=DT, seed=SEED_A,
                                       return_debug=True, row0=7)
    np.testing.assert_array_equal(own, rts[off[7]:])
    for k in EXACT + ("drift",):
        np.testing.assert_array_equal(d7[k], d[k][off[7]:], err_msg=k)
    # the wave range changes no value (128: every row in one wave, lanes take a second row)
    for wr in (64, 128):
        w, _, dw = gpu.gen_rlddm_rows(P, RL, cnt, rewards=p, dt=DT, seed=SEED_A,
                                      return_debug=True, wave_rows=wr)
        np.testing.assert_array_equal(w, rts)
        for k in EXACT + ("drift",):
            np.testing.assert_array_equal(dw[k], d[k], err_msg=k)
        assert dw["wave_steps"].shape == (-(-R_A // wr),)
        assert dw["wave_steps"].max() >= d["n_steps"].max()
    other, _ = gpu.gen_rlddm_rows(P, RL, cnt, rewards=p, dt=DT, seed=SEED_A + 1)
    assert np.mean(other != rts) > 0.9


@pytest.mark.gpu
def test_simulator_and_likelihood_agree(gpu):
    """(b) the likelihood's recurrence over the simulated responses and
    feedback holds the drifts the simulator walked with, bit for bit: the two
    share the Q update. One likelihood call per kind, a row per condition."""
    L = loop_a(gpu)
    P, RL, cnt, rts, off, d = (L[k] for k in ("P", "RL", "cnt", "rts", "off", "d"))
    checked = 0
    for kind in range(len(KINDS)):
        rows = [r for r in range(R_A) if r % len(KINDS) == kind and cnt[r] > 0]
        sel = np.concatenate([np.arange(off[r], off[r + 1]) for r in rows])
        split = np.concatenate([np.full(cnt[r], r, dtype=np.int64) for r in rows])
        v, sv, a, z, sz, t, st = KINDS[kind, :7]
        x = np.ascontiguousarray(rts[sel])
        _, _, drift = gpu.wiener_like_rlddm_terms(
            x, (x > 0).astype(np.int64), np.ascontiguousarray(d["feedback"][sel]), split,
            *KINDS[kind, 7:10], v, sv, a, z, sz, t, st, 1e-4, n_st=2, n_sz=2, use_adaptive=1,
            simps_err=1e-3, p_outlier=0.05, w_outlier=0.1)
        assert np.array_equal(drift, d["sim_drift"][sel]), kind
        checked += len(rows)
    assert checked == np.sum(cnt > 0)


@pytest.mark.gpu
def test_rows_whose_drift_never_moves_draw_what_the_open_loop_kernel_draws(gpu):
    """(c) v = 0 with real learning, and alpha = -800 (the rate is exactly 0.0):
    the drift stays 0 and every trial is draw k of row r of
    gen_rts_from_drift_nodes at v = 0 under the same seed and row0."""
    assert rate(-800.0) == 0.0
    P, RL, p, _ = tables(14)
    cnt = np.array([COUNTS[1 + r % 5] for r in range(14)], dtype=np.int64)
    still_v, still_rate = P.copy(), RL.copy()
    still_v[:, 0] = 0.0
    still_rate[:, 1] = -800.0
    still_rate[:, 2] = 100.0
    want, woff, wd = gpu.gen_rts_from_drift_nodes(still_v, cnt, dt=DT, seed=41, row0=5,
                                                  return_debug=True)
    for params, rl in ((still_v, RL), (P, still_rate)):
        rts, off, d = gpu.gen_rlddm_rows(params, rl, cnt, rewards=p, dt=DT, seed=41, row0=5,
                                         return_debug=True)
        np.testing.assert_array_equal(off, woff)
        np.testing.assert_array_equal(rts, want)
        for k in ("y0", "delay", "drift", "n_steps"):
            np.testing.assert_array_equal(d[k], wd[k], err_msg=k)
        assert np.all(d["sim_drift"] == 0)
    # the last call's rate is 0: Q never moves
    np.testing.assert_array_equal(d["q_up"], np.repeat(RL[:, 0], cnt))
    np.testing.assert_array_equal(d["q_low"], np.repeat(RL[:, 0], cnt))


@pytest.mark.gpu
def test_supplied_rewards_and_observed_mode(gpu):
    """(d) Gaussian outcomes as supplied arrays, shared by replicate rows
    through the start offsets; the one-step-ahead mode: Q follows the observed
    pair in every replicate, only the RTs differ."""
    rng = np.random.default_rng(17)
    P, RL, _, _ = tables(6)
    n = 30
    rew_up, rew_low = rng.normal(0.7, 0.3, 2 * n), rng.normal(0.3, 0.3, 2 * n)
    start = np.array([0, n, 0, n, 0, 5])
    cnt = np.array([n, n, n, n, 7, 25], dtype=np.int64)
    rts, off, d = gpu.gen_rlddm_rows(P, RL, cnt, reward_arrays=(rew_up, rew_low, start), dt=DT,
                                     seed=23, return_debug=True)
    src = np.concatenate([start[r] + np.arange(cnt[r]) for r in range(6)])
    np.testing.assert_array_equal(d["feedback"], np.where(rts > 0, rew_up[src], rew_low[src]))
    host = restate_loop(P, RL, cnt, 23, arrays=(rew_up, rew_low), start=start, drift=d["drift"])
    assert_loop_equal(rts, d, host, np.repeat(P[:, 1], cnt))
    # without start offsets a row reads at its own offset
    own, _, d_own = gpu.gen_rlddm_rows(P[:2], RL[:2], n, reward_arrays=(rew_up, rew_low), dt=DT,
                                       seed=23, return_debug=True)
    np.testing.assert_array_equal(own, rts[:2 * n])
    # observed mode: 3 replicates of one observed sequence, for two kinds of row
    response = rng.integers(0, 2, n)
    feedback = rng.integers(0, 2, n).astype(np.float64)
    feedback[3], feedback[11] = 0.5, 0.5  # ties with q = 0.5 where Q has not moved yet
    for kind in (0, 2):
        Pk, RLk = np.tile(KINDS[kind, :7], (3, 1)), np.tile(KINDS[kind, 7:10], (3, 1))
        rts, off, d = gpu.gen_rlddm_rows(Pk, RLk, n, observed=(response, feedback, np.zeros(3)),
                                         dt=DT, seed=29, return_debug=True)
        want, _ = restate_rlddm(response, feedback, np.zeros(n, dtype=np.int64), *KINDS[kind, 7:10],
                                KINDS[kind, 0])
        for r in range(3):
            assert np.array_equal(d["sim_drift"][off[r]:off[r + 1]], want), (kind, r)
            np.testing.assert_array_equal(d["feedback"][off[r]:off[r + 1]], feedback)
        assert np.mean(rts[:n] != rts[n:2 * n]) > 0.9 and np.mean(rts[:n] != rts[2 * n:]) > 0.9
        host = restate_loop(Pk, RLk, n, 29, observed=(response, feedback), start=np.zeros(3),
                            drift=d["drift"])
        assert_loop_equal(rts, d, host, np.repeat(Pk[:, 1], n))


@pytest.mark.gpu
def test_an_unfinished_walk_ends_its_sequence(gpu):
    """(e) max_t = 3 dt: no walk of the a = 2 row can finish, about half of
    the a = 0.1 rows' do (two steps the same way cross); from a row's first cut
    trial on everything is NaN. The seed is one under which the restatement
    finishes leading trials in four rows."""
    P, RL, p, _ = tables(8)
    P[0, 2] = 2.0
    P[[2, 5, 6], 2] = 0.1
    cnt = np.array([6, 9, 5, 33, 9, 2, 5, 33], dtype=np.int64)
    max_t = 3 * DT
    max_steps = int(np.ceil(max_t / DT))
    rts, off, d = gpu.gen_rlddm_rows(P, RL, cnt, rewards=p, dt=DT, seed=36, max_t=max_t,
                                     unfinished="nan", return_debug=True)
    host = restate_loop(P, RL, cnt, 36, rewards=p, drift=np.nan_to_num(d["drift"]),
                        max_steps=max_steps)
    np.testing.assert_array_equal(rts, host["rt"])
    np.testing.assert_array_equal(d["feedback"], host["feedback"])
    np.testing.assert_array_equal(d["n_steps"], host["n_steps"])
    assert np.isnan(rts[off[0]:off[1]]).all() and d["n_steps"][0] == max_steps
    finished_some = 0
    for r in range(8):
        row = rts[off[r]:off[r + 1]]
        nan = np.isnan(row)
        if nan.any():
            first = int(np.argmax(nan))
            assert nan[first:].all() and not nan[:first].any()
            assert np.all(d["n_steps"][off[r] + first + 1:off[r + 1]] == 0)
            finished_some += first > 0
    assert finished_some >= 2 and 0 < np.isnan(rts).sum() < rts.size
    with pytest.raises(RuntimeError, match=rf"\b{int(np.isnan(rts).sum())} of {rts.size}\b"):
        gpu.gen_rlddm_rows(P, RL, cnt, rewards=p, dt=DT, seed=36, max_t=max_t)
    with pytest.raises(RuntimeError):
        gpu.gen_rlddm_stats_rows(P, RL, cnt, [0, 8], rewards=p, dt=DT, seed=36, max_t=max_t)
    again, _ = gpu.gen_rlddm_rows(P, RL, cnt, rewards=p, dt=DT, seed=36)  # the default max_t
    assert np.isfinite(again).all()
    np.testing.assert_array_equal(again[~np.isnan(rts)], rts[~np.isnan(rts)])


@pytest.mark.gpu
def test_fused_statistics_equal_unfused(gpu):
    """(f) six nodes of 2-3 condition sequences, one past the wave tier's 256
    draws, one of empty rows: the fused call's rows are rt_stats_rows of the
    plain call's draws."""
    groups = np.array([0, 2, 5, 7, 10, 12, 14])
    cnt = np.array([5, 9, 130, 100, 60, 0, 0, 33, 1, 2, 64, 64, 7, 0], dtype=np.int64)
    P, RL, p, _ = tables(14)
    rts, off = gpu.gen_rlddm_rows(P, RL, cnt, rewards=p, dt=DT, seed=37)
    goff = off[groups]
    assert np.diff(goff).max() > 256 and np.diff(goff).min() == 0
    for q in ((10, 30, 50, 70, 90), ()):
        want = gpu.rt_stats_rows(rts, goff, q)
        got, got_off, draws = gpu.gen_rlddm_stats_rows(P, RL, cnt, groups, rewards=p, quantiles=q,
                                                       dt=DT, seed=37, return_draws=True)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_off, goff)
        np.testing.assert_array_equal(draws, rts)
        only, _ = gpu.gen_rlddm_stats_rows(P, RL, cnt, groups, rewards=p, quantiles=q, dt=DT,
                                           seed=37)
        np.testing.assert_array_equal(only, want)
    assert np.isnan(want[2, 3]) and want[2, 0] == 0 and want[1, 0] == 290
    # unfinished walks are counted on the device when no draw comes back
    stats, _ = gpu.gen_rlddm_stats_rows(P, RL, cnt, groups, rewards=p, dt=DT, seed=37,
                                        max_t=3 * DT, unfinished="nan")
    cut, _ = gpu.gen_rlddm_rows(P, RL, cnt, rewards=p, dt=DT, seed=37, max_t=3 * DT,
                                unfinished="nan")
    np.testing.assert_array_equal(stats, gpu.rt_stats_rows(cut, goff))
    assert np.isnan(cut).any()


@pytest.mark.gpu
def test_choices_follow_the_host_loops_distribution(gpu):
    """(g) 1500 sequences of 40 trials on the device and by the host-driven
    loop over the same walk: the share of upper choices in trials 31-40."""
    from hddm_amd import rl
    n_seq, n = 1500, 40
    P = np.tile([3.0, 0.0, 1.0, 0.5, 0.0, 0.3, 0.0], (n_seq, 1))
    RL = np.tile([0.5, 0.0, 100.0], (n_seq, 1))
    assert rl.learning_rate(0.0) == 0.5
    rts, _ = gpu.gen_rlddm_rows(P, RL, n, rewards=(0.8, 0.2), dt=DT, seed=20261021)
    dev = np.mean(rts.reshape(n_seq, n)[:, 30:] > 0, axis=1)
    step = [0]

    def draw(drifts):
        T = np.zeros((drifts.size, 7))
        T[:, 0], T[:, 2], T[:, 3], T[:, 5] = drifts, 1.0, 0.5, 0.3
        step[0] += 1
        return gpu.gen_rts_from_drift_nodes(T, 1, dt=DT, seed=977 + step[0])[0]

    data, _ = rl.gen_rl_data(n_seq, n, {0: (0.8, 0.2)}, a=1.0, t=0.3, v=3.0, alpha=0.0,
                             jitter=0, seed=5, closed_loop="host", draw=draw)
    host = np.mean(data["response"].to_numpy().reshape(n_seq, n)[:, 30:], axis=1)
    m1, m2, s1, s2 = dev.mean(), host.mean(), dev.std(ddof=1), host.std(ddof=1)
    bound = 4.5 * np.sqrt(s1 ** 2 / n_seq + s2 ** 2 / n_seq)
    print(f"upper share, trials 31-40: device {m1:.4f} (sd {s1:.4f}), host {m2:.4f} "
          f"(sd {s2:.4f}), |diff| {abs(m1 - m2):.4f}, bound {bound:.4f}")
    assert abs(m1 - m2) <= bound
    assert m1 > 0.6 and m2 > 0.6


@pytest.mark.gpu
def test_model_post_pred_sim(gpu):
    """(h) HDDMrl.post_pred_sim / post_pred_sim_stats and gen_rl_data's device
    loop on a small model."""
    from hddm_amd import rl
    from hddm_amd.hierarchical import HDDM
    conds = {0: (0.8, 0.2), 1: (0.7, 0.3)}
    kw = dict(a=1.2, t=0.3, v=2.5, alpha=-0.5, seed=9, dt=DT)
    data, truth = rl.gen_rl_data(3, 12, conds, closed_loop="host", **kw)
    m = rl.HDDMrl(data, seed=2)
    m.sample(6)
    sim = m.post_pred_sim(conds, samples=3, seed=1, dt=DT, return_debug=True)
    assert list(sim.columns) == ["sample", "node", "split_by", "trial", "rt", "response",
                                 "feedback", "q_up", "q_low", "sim_drift"]
    assert len(sim) == 3 * 3 * 24 and sim["sample"].nunique() == 3
    sizes = sim.groupby(["sample", "node", "split_by"]).size()
    assert len(sizes) == 3 * 3 * 2 and np.all(sizes == 12)
    assert np.array_equal(sim["response"], (sim["rt"] > 0).astype(int))
    assert list(sim["trial"][:12]) == list(range(1, 13))
    again = m.post_pred_sim(conds, samples=3, seed=1, dt=DT, return_debug=True)
    assert sim.equals(again)
    assert not sim["rt"].equals(m.post_pred_sim(conds, samples=3, seed=2, dt=DT)["rt"])
    # a direct call on the documented tables
    T = m.post_pred_sim_rows(3)
    assert T["params"].shape == (18, 8) and T["rl_rows"].shape == (18, 3)
    assert np.array_equal(T["node"], [0, 0, 1, 1, 2, 2]) and np.all(T["counts"] == 12)
    assert np.array_equal(T["split_by"], [0, 1] * 3)
    assert np.all(T["rl_rows"][:, 0] == 0.5) and np.all(T["rl_rows"][:, 2] == 100.0)
    for s, sweep in enumerate(T["picked"]):
        assert np.array_equal(T["rl_rows"][6 * s:6 * s + 6, 1],
                              np.repeat(m.trace_subj["alpha"][sweep], 2))
        assert np.array_equal(T["params"][6 * s:6 * s + 6, 2],
                              np.repeat(m.trace_subj["a"][sweep], 2))
    p = np.tile([conds[0], conds[1]], (9, 1))
    rts, _, d = gpu.gen_rlddm_rows(T["params"], T["rl_rows"], np.tile(T["counts"], 3), rewards=p,
                                   dt=DT, seed=1, return_debug=True)
    np.testing.assert_array_equal(sim["rt"].to_numpy(), rts)
    for k in ("feedback", "q_up", "q_low", "sim_drift"):
        np.testing.assert_array_equal(sim[k].to_numpy(), d[k])
    # one step ahead of the observed choices
    one = m.post_pred_sim(samples=3, seed=1, dt=DT, mode="onestep", return_debug=True)
    assert len(one) == len(sim)
    for (s, j), part in one.groupby(["sample", "node"]):
        obs = data[data["subj_idx"] == j]
        sweep = list(T["picked"]).index(s)
        want, _ = restate_rlddm(obs["response"].to_numpy(), obs["feedback"].to_numpy(),
                                obs["split_by"].to_numpy(), 0.5,
                                m.trace_subj["alpha"][s][j], 100.0, m.trace_subj["v"][s][j])
        order = np.argsort(obs["split_by"].to_numpy(), kind="stable")
        assert np.array_equal(part["sim_drift"].to_numpy(), want[order]), (s, j, sweep)
        assert np.array_equal(part["feedback"].to_numpy(), obs["feedback"].to_numpy()[order])
    with pytest.raises(ValueError):
        m.post_pred_sim(samples=3)  # closed loop without a reward schedule
    with pytest.raises(KeyError):
        m.post_pred_sim({0: (0.8, 0.2)}, samples=3)
    # the check's table, shaped like HDDM.post_pred_stats'
    table, sampled = m.post_pred_sim_stats(conds, samples=3, seed=1, dt=DT, return_sampled=True)
    names = gpu.rt_stats_names()
    assert sampled.shape == (3, 3, len(names))
    assert list(table.index.names) == ["node", "stat"] and len(table) == 3 * len(names)
    assert list(table.columns) == ["observed", "mean", "std", "SEM", "MSE", "credible", "quantile",
                                   "mahalanobis"]
    plain = HDDM(data, seed=2)
    plain.sample(2)
    like = plain.post_pred_stats(samples=2, seed=1)
    assert table.index.equals(like.index) and list(table.columns) == list(like.columns)
    goff = np.arange(0, len(sim) + 1, 24)
    np.testing.assert_array_equal(sampled.reshape(9, -1),
                                  gpu.rt_stats_rows(sim["rt"].to_numpy(), goff))
    # gen_rl_data with the loop on the device: the same columns, the same checks
    dev, truth_d = rl.gen_rl_data(3, 12, conds, closed_loop="device", **kw)
    assert list(dev.columns) == list(data.columns) and truth_d == truth
    assert [str(t) for t in dev.dtypes] == [str(t) for t in data.dtypes]
    assert np.array_equal((dev["rt"] > 0).astype(int), dev["response"])
    rng = np.random.default_rng(9)
    rng.uniform(-1, 1, 3 * 4)
    for s in range(3):
        part = dev[dev["subj_idx"] == s]
        drift, _ = restate_rlddm(part["response"].to_numpy(), part["feedback"].to_numpy(),
                                 part["split_by"].to_numpy(), 0.5, truth["alpha"][s], 100.0,
                                 truth["v"][s])
        assert np.array_equal(part["sim_drift"].to_numpy(), drift)
        assert np.array_equal(part["sim_drift"].to_numpy(),
                              (part["q_up"].to_numpy() - part["q_low"].to_numpy()) * truth["v"][s])
        for c, (p_up, p_low) in conds.items():
            seq = part[part["split_by"] == c]
            assert seq["sim_drift"].iloc[0] == 0.0 and list(seq["trial"]) == list(range(1, 13))
            up, low = rng.binomial(1, p_up, 12), rng.binomial(1, p_low, 12)
            assert np.array_equal(seq["feedback"].to_numpy(),
                                  np.where(seq["response"].to_numpy() == 1, up, low))
