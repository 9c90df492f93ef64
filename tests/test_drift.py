"""The on-device diffusion-path simulator (wfpt_gen_rts_drift_nodes,
sim_drift_kernel): the 'drift' sampling method, hddm/generate.py:208-319.

References: the reference's own function, run once on recorded random numbers
(tests/golden/make_golden_drift.py -> tests/golden/drift.npz); its NumPy
restatement below, pinned to that fixture bit for bit, fed the device's Philox
streams; the oracle's / the GPU's DMAT CDF for the distribution. Tolerances:
  * start point, delay, steps taken, RT given the drift rate: none
    (assert_array_equal);
  * drift rate: relative 1e-13 against the host Box-Muller (the device's log,
    cos and sqrt are each a few ulp from glibc's; ten times that);
  * KS distance to the DMAT CDF: 1.63 / sqrt(n), the 1 % critical value, at
    n = 4000 and dt = 1e-3 (the walk's own discretisation bias, ~0.012 on these
    rows, leaves room below 0.0258; it would not at n = 20000).
"""
import os

import numpy as np
import pytest

from test_sim import ks_distance, philox4x32_10, philox_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1e-3
NEVER = 1e6  # a t_switch no walk reaches: the row keeps its drift
# v, sv, a, z, sz, t, st | v_switch, V_switch, t_switch
ROWS = np.array([
    (0.5, 0.0, 2.0, 0.5, 0.0, 0.3, 0.0, 0.5, 0.0, NEVER),       # plain
    (0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 0.5, 0.0, NEVER),       # full: sv, sz, st
    (1.0, 0.0, 2.0, 0.5, 0.0, 0.3, 0.0, -3.0, 0.0, 0.2),        # switch at step 200
    (0.5, 0.0, 0.1, 0.5, 0.2, 0.3, 0.0, 0.5, 0.0, NEVER),       # a = 0.1: a few steps
    (-1.2, 0.8, 1.4, 0.45, 0.25, 0.25, 0.1, 2.0, 0.5, 0.001),   # switch at step 1, V_switch
    (0.3, 0.0, 1.0, 0.021, 0.04, 0.2, 0.0, 0.3, 0.0, NEVER),    # z - sz/2 = 0.001: crossings on step 0
    (0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, -1.0, 0.5, 0.004),      # switch at step 4
    (0.0, 0.0, 1.0, 0.5, 0.0, 0.1, 0.2, 1.5, 0.0, 0.005),       # switch at step 5, v = 0
])
KS_ROWS = np.array([(0.5, 0.0, 2.0, 0.5, 0.0, 0.3, 0.0), (0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1)])
KS_N, KS_SEED = 4000, 20261019
KS_BOUND = 1.63 / np.sqrt(KS_N)
SWITCH_PARENTS = {"v": 0.5, "a": 2.0, "z": 0.5, "t": 0.3}
SWITCH = {"v_switch": -3.0, "t_switch": 0.2}


def rows_of(R):
    T = ROWS[np.arange(R) % len(ROWS)]
    return T[:, :7].copy(), T[:, 7:].copy()


# ---------------------------------------------------------------- restatement

def switch_step(t_switch, dt):
    """generate.py:237-239: int(round(t_switch / dt))."""
    return np.round(np.asarray(t_switch, dtype=np.float64) / dt).astype(np.int64)


def walk(a, y0, delay, drift, drift_sw, nn, dt, intra_sv, max_steps, ups_at):
    """generate.py:258-313 for n trials in lockstep (each trial's sums stay in
    its own order). drift_sw / nn: the drift rate from step nn on.
    ups_at(k, idx, prob_up): the outcomes of step k for the trials idx.
    Returns (signed RTs, NaN where max_steps steps did not cross; steps taken)."""
    step = np.sqrt(dt) * intra_sv
    p1 = 0.5 * (1 + np.sqrt(dt) / intra_sv * drift)
    p2 = 0.5 * (1 + np.sqrt(dt) / intra_sv * drift_sw)
    n = a.shape[0]
    y = np.array(y0, dtype=np.float64)
    out = np.full(n, np.nan)
    steps = np.full(n, max_steps, dtype=np.int64)
    idx = np.arange(n)
    for k in range(max_steps):
        if idx.size == 0:
            break
        up = ups_at(k, idx, np.where(k >= nn[idx], p2[idx], p1[idx]))
        y1 = y[idx]
        y2 = y1 + np.where(up, step, -step)
        cross = (y2 < 0) | (y2 > a[idx])
        if cross.any():
            c, y1c, y2c = idx[cross], y1[cross], y2[cross]
            m = (y2c - y1c) / dt
            b = y2c - m * k * dt
            rt = np.where(y2c < 0, (0 - b) / m, (a[c] - b) / m)
            out[c] = (rt + delay[c]) * np.sign(y2c)
            steps[c] = k + 1
        y[idx] = y2
        idx = idx[~cross]
    return out, steps


def philox_words(seed, row, draw, stream):
    row, draw, stream = np.broadcast_arrays(np.asarray(row, dtype=np.uint64),
                                            np.asarray(draw, dtype=np.uint64),
                                            np.asarray(stream, dtype=np.uint64))
    m32 = np.uint64(0xFFFFFFFF)
    ctr = np.stack([draw & m32, draw >> np.uint64(32), row, stream], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF],
                                   dtype=np.uint64), row.shape + (2,))
    return philox4x32_10(ctr, key).astype(np.uint64)


def philox_normal(seed, row, draw, stream):
    w = philox_words(seed, row, draw, stream)
    u = [((w[..., i] >> np.uint64(5)).astype(np.float64) * 67108864.0 +
          (w[..., i + 1] >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53 for i in (0, 2)]
    return np.sqrt(-2.0 * np.log(1.0 - u[0])) * np.cos(2.0 * np.pi * u[1])


class PhiloxSteps:
    """Word k % 4 of stream 16 + k // 4 decides step k: up iff w 2^-32 < prob_up."""

    def __init__(self, seed, row, draw):
        self.seed, self.row, self.draw = seed, row, draw
        self.w = np.zeros(row.shape + (4,), dtype=np.uint64)

    def __call__(self, k, idx, prob_up):
        if k % 4 == 0:
            self.w[idx] = philox_words(self.seed, self.row[idx], self.draw[idx], 16 + k // 4)
        return self.w[idx, k % 4].astype(np.float64) * 2.0 ** -32 < prob_up


def restate(P, sw, counts, seed, dt=DT, intra_sv=1.0, max_steps=20000, row0=0, drift=None,
            drift_sw=None):
    """What the device call returns, row after row: dict of rt, y0, delay,
    drift, drift_switch, n_steps. drift / drift_sw: rates to use instead of
    the host Box-Muller's."""
    P = np.asarray(P, dtype=np.float64)
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), (P.shape[0],))
    r = np.repeat(np.arange(P.shape[0]), counts)
    off = np.r_[0, np.cumsum(counts)]
    j = np.arange(off[-1]) - off[r]
    row = r + row0
    v, sv, a, z, sz, t, st = (np.ascontiguousarray(P[r, i]) for i in range(7))
    u_t = np.where(st != 0, philox_uniform(seed, row, j, 1), 0.0)
    u_z = np.where(sz != 0, philox_uniform(seed, row, j, 2), 0.0)
    delay = (t + st * u_t) - st / 2.
    y0 = ((z + sz * u_z) - sz / 2.) * a
    host_drift = np.where(sv != 0, v + sv * philox_normal(seed, row, j, 3), v)
    if sw is None:
        host_sw, nn = np.zeros(r.shape), np.full(r.shape, np.iinfo(np.int64).max)
    else:
        sw = np.asarray(sw, dtype=np.float64)
        host_sw = np.where(sw[r, 1] != 0, sw[r, 0] + sw[r, 1] * philox_normal(seed, row, j, 4),
                           sw[r, 0])
        nn = switch_step(sw[r, 2], dt)
    d1 = host_drift if drift is None else drift
    d2 = host_sw if drift_sw is None else drift_sw
    rt, steps = walk(a, y0, delay, d1, d2, nn, dt, intra_sv, max_steps,
                     PhiloxSteps(seed, row, j))
    return {"rt": rt, "y0": y0, "delay": delay, "drift": host_drift, "drift_switch": host_sw,
            "n_steps": steps}


def lower_share(rts):
    return float(np.mean(rts < 0))


def share_gap_in_standard_errors(plain, switched):
    p, q, n = lower_share(plain), lower_share(switched), plain.size
    return (q - p) / np.sqrt(p * (1 - p) / n + q * (1 - q) / n)


# --------------------------------------------------------------------------- CPU

def test_restatement_reproduces_the_reference_fixture():
    """The fixture's recorded uniforms, normals and step outcomes through the
    restatement: every start point, delay, drift rate and RT of the reference's
    own run, bit for bit."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "drift.npz")))
    dt, intra_sv = float(g["dt"]), float(g["intra_sv"])
    P, sw = g["params"], g["switch"]
    n = P.shape[0]
    assert n >= 40
    v, sv, a, z, sz, t, st = P.T
    has_sw = ~np.isnan(sw[:, 2])
    assert has_sw.sum() >= 10 and (sv != 0).sum() >= 10 and (a == 0.1).sum() >= 8
    delay = (t + st * g["u_t"]) - st / 2.
    y0 = ((z + sz * g["u_z"]) - sz / 2.) * a
    np.testing.assert_array_equal(delay, g["delay"])
    np.testing.assert_array_equal(y0, g["y0"])
    drift = np.where(sv != 0, v + sv * np.nan_to_num(g["n"]), v)
    np.testing.assert_array_equal(drift, g["drift"])
    drift_sw = np.where(has_sw & (np.nan_to_num(sw[:, 1]) != 0),
                        sw[:, 0] + sw[:, 1] * np.nan_to_num(g["n_switch"]), sw[:, 0])
    np.testing.assert_array_equal(drift_sw[has_sw], g["drift_switch"][has_sw])
    nn = np.where(has_sw, switch_step(np.nan_to_num(sw[:, 2], nan=1.0), dt),
                  np.iinfo(np.int64).max)
    assert set(nn[has_sw]) == {5, 200}
    bits = np.unpackbits(g["ups"]).astype(bool)
    off = np.r_[0, np.cumsum(g["n_bits"])]
    ups = np.zeros((n, int(g["n_bits"].max())), dtype=bool)
    for i in range(n):
        ups[i, :g["n_bits"][i]] = bits[off[i]:off[i + 1]]
    rt, steps = walk(a, y0, delay, drift, np.nan_to_num(drift_sw), nn, dt, intra_sv,
                     ups.shape[1], lambda k, idx, p: ups[idx, k])
    assert np.all(steps <= g["n_bits"])  # every crossing inside the recorded outcomes
    np.testing.assert_array_equal(rt, g["rt"])
    small = a == 0.1
    assert steps[small].min() == 1 and steps[small].max() < 20  # crossings from step 0 on
    assert np.unique(steps[small]).size >= 3
    assert np.any(rt < 0) and np.any(rt > 0)


def test_python_argument_checks_without_gpu(monkeypatch):
    from hddm_amd import _lib, wfpt

    def no_context(*a, **k):
        raise AssertionError("a context was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "context", no_context)
    assert "gen_rts_from_drift_nodes" in wfpt.__all__ and "gen_rts_from_drift" in wfpt.__all__
    P, sw = rows_of(2)
    f = wfpt.gen_rts_from_drift_nodes
    with pytest.raises(ValueError):
        f([[0.5, 0, 2, 0.5, 0, 0.3, 0], [0.5, 0, 2]], 5)
    with pytest.raises(ValueError):
        f(np.zeros((2, 6)), 5)
    with pytest.raises(ValueError):
        f(P, [5, 4, 3])
    with pytest.raises(ValueError):
        f(P, [5, -1])
    with pytest.raises(ValueError):
        f(P, 5, dt=0.0)
    with pytest.raises(ValueError):
        f(P, 5, dt=-1e-3)
    with pytest.raises(ValueError):
        f(P, 5, intra_sv=0.0)
    with pytest.raises(ValueError):
        f(P, 5, dt=1e-3, switch=sw[:1])
    with pytest.raises(ValueError):  # 0.0004 / 1e-3 rounds to 0 steps
        f(P, 5, dt=1e-3, switch=[[1.0, 0.0, 0.2], [1.0, 0.0, 0.0004]])
    with pytest.raises(ValueError):
        f(P, 5, unfinished="ignore")
    with pytest.raises(ValueError):  # more than 2^31 steps
        f(P, 5, dt=1e-9, max_t=20.)
    with pytest.raises(ValueError):
        f(P, 5, wave_draws=100)
    with pytest.raises(ValueError):
        wfpt.gen_rts_from_drift(0.5, 0, 2, 0.5, 0, 0.3, 0, 5, v_switch=1.0)
    with pytest.raises(TypeError):
        wfpt.gen_rts_from_drift(0.5, 0, 2, 0.5, 0, 0.3, 0, 5, w_switch=1.0)
    with pytest.raises(AssertionError):  # valid arguments do reach the context
        f(P, 5, dt=1e-3, switch=sw)


def test_entry_points_reject_bad_arguments_without_gpu():
    from hddm_amd import _lib
    two = 2
    assert _lib.wfpt_gen_rts_drift_nodes(None, None, 0, None, None, 1e-3, 1.0, 10, 0, None,
                                         None) == two
    assert b"null" in _lib.wfpt_last_error()
    assert _lib.wfpt_gen_rts_drift_nodes_ex(None, None, 0, None, None, 1e-3, 1.0, 10, 0, 0, 0,
                                            None, None, None, None, None, None, None,
                                            None) == two
    assert b"null" in _lib.wfpt_last_error()
    P = np.zeros((1, 8))
    P[0, :7] = ROWS[0, :7]
    cnt = np.array([3], dtype=np.int64)
    neg = np.array([-1], dtype=np.int64)
    out = np.empty(3)
    nun = np.zeros(1, dtype=np.int64)
    sw0 = np.array([1.0, 0.0, 0.0004])

    def call(counts=cnt, dt=1e-3, intra_sv=1.0, max_steps=10, sw=None, ex=False):
        head = (None, P.ctypes.data_as(_lib._PP), 1, _lib.dptr(sw) if sw is not None else None,
                counts.ctypes.data_as(_lib._PI64), dt, intra_sv, max_steps, 0)
        tail = (_lib.dptr(out), nun.ctypes.data_as(_lib._PI64))
        if ex:
            return _lib.wfpt_gen_rts_drift_nodes_ex(*head, 0, 0, *tail, None, None, None, None,
                                                    None, None)
        return _lib.wfpt_gen_rts_drift_nodes(*head, *tail)

    for ex in (False, True):
        for kw, msg in (({"dt": 0.0}, b"dt <= 0"), ({"dt": -1.0}, b"dt <= 0"),
                        ({"dt": float("nan")}, b"dt <= 0"), ({"intra_sv": 0.0}, b"intra_sv"),
                        ({"max_steps": 0}, b"max_steps"), ({"max_steps": 2 ** 31 + 1}, b"max_steps"),
                        ({"counts": neg}, b"negative count"), ({}, b"context"),
                        ({"sw": sw0}, b"t_switch")):
            assert call(ex=ex, **kw) == two, kw
            assert msg in _lib.wfpt_last_error(), (kw, _lib.wfpt_last_error())


_KS_DRAWS = {}


def ks_restated(i):
    """The restatement's draws of KS row i under the device's Philox streams,
    computed once."""
    if i not in _KS_DRAWS:
        d = restate(KS_ROWS[i:i + 1], None, KS_N, KS_SEED)
        assert not np.isnan(d["rt"]).any()
        _KS_DRAWS[i] = d
    return _KS_DRAWS[i]


@pytest.mark.parametrize("i", [0, 1])
def test_ks_seed_passes_with_the_restatement_alone(oracle_lib, i):
    """The distribution check of test_device_draws_follow_the_dmat_cdf with the
    restatement in the device's place and the oracle's DMAT CDF."""
    draws = np.sort(ks_restated(i)["rt"])
    F = oracle_lib.dmat_cdf_array(draws, *KS_ROWS[i], 0.0, 0.1)
    d = ks_distance(draws, F)
    print(f"restatement KS distance {d:.5f}, bound {KS_BOUND:.5f}")
    assert d < KS_BOUND


def test_switch_moves_the_lower_share_in_the_restatement():
    """v_switch = -3 from 0.2 s on sends most walks to the lower boundary: the
    gap test_gen_random_on_device asks of the device, on the restatement."""
    p = [[SWITCH_PARENTS["v"], 0, SWITCH_PARENTS["a"], SWITCH_PARENTS["z"], 0,
          SWITCH_PARENTS["t"], 0]]
    plain = restate(p, None, 2000, 11)["rt"]
    switched = restate(p, [[SWITCH["v_switch"], 0.0, SWITCH["t_switch"]]], 2000, 12)["rt"]
    gap = share_gap_in_standard_errors(plain, switched)
    print(f"lower shares {lower_share(plain):.3f} -> {lower_share(switched):.3f}, {gap:.1f} SE")
    assert gap > 4


def test_install_rebinds_the_simulator_only_on_request(monkeypatch):
    """install() leaves the reference's generate module alone; drift=True
    rebinds _gen_rts_from_simulated_drift to a wrapper that hands the
    parameter dict to gen_rts_from_drift, and uninstall() puts it back."""
    import types
    from hddm_amd import integration, wfpt as amd
    ref, cdf = types.ModuleType("wfpt"), types.ModuleType("cdfdif_wrapper")
    gen = types.ModuleType("hddm.generate")
    gen._gen_rts_from_simulated_drift = lambda *a, **k: "ref"
    inst = integration.install(ref, cdf, generate_module=gen)
    assert gen._gen_rts_from_simulated_drift() == "ref"
    inst.uninstall()
    calls = []
    monkeypatch.setattr(amd, "gen_rts_from_drift", lambda *a, **k: calls.append((a, k)) or "rts")
    inst = integration.install(ref, cdf, drift=True, generate_module=gen)
    params = {"v": 1.0, "a": 2.0, "t": 0.3, "sv": 0.1, "v_switch": -3.0, "t_switch": 0.2}
    assert gen._gen_rts_from_simulated_drift(params, 7, 1e-3, 1.5) == ("rts", [])
    assert calls == [((1.0, 0.1, 2.0, .5, 0, 0.3, 0, 7, 1e-3, 1.5),
                      {"v_switch": -3.0, "t_switch": 0.2})]
    inst.uninstall()
    assert gen._gen_rts_from_simulated_drift() == "ref"


# --------------------------------------------------------------------------- GPU

_GIVEN = {}


def assert_matches_restatement(P, sw, cnt, seed, rts, off, d, **kw):
    np.testing.assert_array_equal(off, np.r_[0, np.cumsum(cnt)])
    host = restate(P, sw, cnt, seed, **kw)
    np.testing.assert_array_equal(d["y0"], host["y0"])
    np.testing.assert_array_equal(d["delay"], host["delay"])
    np.testing.assert_allclose(d["drift"], host["drift"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(d["drift_switch"], host["drift_switch"], rtol=1e-13, atol=0)
    # the walk under the device's own drift rates, shared by the calls that
    # differ in schedule only (their rates are the same bits)
    key = (P.tobytes(), None if sw is None else sw.tobytes(), cnt.tobytes(), seed,
           d["drift"].tobytes(), d["drift_switch"].tobytes(), tuple(sorted(kw.items())))
    if key not in _GIVEN:
        _GIVEN[key] = restate(P, sw, cnt, seed, drift=d["drift"], drift_sw=d["drift_switch"], **kw)
    given = _GIVEN[key]
    np.testing.assert_array_equal(d["n_steps"], given["n_steps"])
    np.testing.assert_array_equal(rts, given["rt"])
    return given


@pytest.mark.gpu
@pytest.mark.parametrize("R,counts,wave_draws", [
    (1, [1], None), (3, [63, 0, 65], None), (3, [63, 0, 65], 64),
    (130, None, None), (130, None, 128), (130, None, 1024)])
def test_device_equals_restatement(gpu, R, counts, wave_draws):
    """Every draw against the restatement under the same Philox streams, with
    one draw per lane (the default at these sizes) and with lanes taking
    further draws as they finish (wave_draws > 64)."""
    P, sw = rows_of(R)
    cnt = np.array(counts if counts is not None else 1 + np.arange(R) % 130, dtype=np.int64)
    seed = 0x9E3779B97F4A7C15 + R
    rts, off, d = gpu.gen_rts_from_drift_nodes(P, cnt, dt=DT, seed=seed, switch=sw,
                                               return_debug=True, wave_draws=wave_draws)
    given = assert_matches_restatement(P, sw, cnt, seed, rts, off, d)
    assert not np.isnan(rts).any()
    if R == 130:
        r = np.repeat(np.arange(R), cnt) % len(ROWS)
        assert given["n_steps"][r == 5].min() == 1          # crossings on step 0
        assert given["n_steps"][r == 3].max() <= 40         # a = 0.1
        for row, nn in ((4, 1), (6, 4), (7, 5)):            # walks that outlast their switch
            assert np.sum(given["n_steps"][r == row] > nn) > 10
        if wave_draws:
            assert d["wave_steps"].shape == (-(-cnt.sum() // wave_draws),)
            assert d["wave_steps"].max() >= given["n_steps"].max()
    if R == 3 and wave_draws is None:  # without a switch table the rows keep their drift
        rts0, off0, d0 = gpu.gen_rts_from_drift_nodes(P, cnt, dt=DT, seed=seed,
                                                      return_debug=True)
        assert_matches_restatement(P, None, cnt, seed, rts0, off0, d0)
        assert np.all(d0["drift_switch"] == 0)
        plain = np.repeat(sw[:, 2] == NEVER, cnt)
        np.testing.assert_array_equal(rts0[plain], rts[plain])


@pytest.mark.gpu
def test_a_draw_depends_on_seed_row_and_index_only(gpu):
    R, seed = 130, 77
    P, sw = rows_of(R)
    cnt = (1 + np.arange(R) % 130).astype(np.int64)
    full, off = gpu.gen_rts_from_drift_nodes(P, cnt, dt=DT, seed=seed, switch=sw)
    again, _ = gpu.gen_rts_from_drift_nodes(P, cnt, dt=DT, seed=seed, switch=sw)
    np.testing.assert_array_equal(full, again)
    other, _ = gpu.gen_rts_from_drift_nodes(P, cnt, dt=DT, seed=seed + 1, switch=sw)
    assert np.mean(full != other) > 0.9
    for wd in (64, 128, 1024):  # the schedule changes no value
        w, _ = gpu.gen_rts_from_drift_nodes(P, cnt, dt=DT, seed=seed, switch=sw, wave_draws=wd)
        np.testing.assert_array_equal(full, w)
    cnt2 = (7 + 3 * np.arange(R) % 50).astype(np.int64)
    for r in (0, 2, 65, 129):
        want = full[off[r]:off[r + 1]]
        own, _ = gpu.gen_rts_from_drift_nodes(P[r:r + 1], cnt[r:r + 1], dt=DT, seed=seed,
                                              switch=sw[r:r + 1], row0=r)
        np.testing.assert_array_equal(own, want)
        c = cnt2.copy()
        c[r] = cnt[r]
        moved, off2 = gpu.gen_rts_from_drift_nodes(P, c, dt=DT, seed=seed, switch=sw)
        assert r == 0 or off2[r] != off[r]
        np.testing.assert_array_equal(moved[off2[r]:off2[r + 1]], want)
    # NumPy's global RNG supplies the seed when none is given
    np.random.seed(5)
    a, _ = gpu.gen_rts_from_drift_nodes(P[:3], 10, dt=DT)
    np.random.seed(5)
    b, _ = gpu.gen_rts_from_drift_nodes(P[:3], 10, dt=DT)
    c, _ = gpu.gen_rts_from_drift_nodes(P[:3], 10, dt=DT)
    np.testing.assert_array_equal(a, b)
    assert np.any(a != c)


@pytest.mark.gpu
def test_step_bound(gpu):
    P = np.array([[0.0, 0, 2.0, 0.5, 0, 0.3, 0]])
    rts, off, d = gpu.gen_rts_from_drift_nodes(P, 200, dt=DT, seed=3, max_t=0.05,
                                               unfinished="nan", return_debug=True)
    assert rts.shape == (200,) and np.isnan(rts).all()
    np.testing.assert_array_equal(d["n_steps"], 50)
    with pytest.raises(RuntimeError, match=r"\b200 of 200\b"):
        gpu.gen_rts_from_drift_nodes(P, 200, dt=DT, seed=3, max_t=0.05)
    rts, _ = gpu.gen_rts_from_drift_nodes(P, 200, dt=DT, seed=3)  # the same context, default max_t
    assert np.isfinite(rts).all()
    some, _, d = gpu.gen_rts_from_drift_nodes(P, 200, dt=DT, seed=3, max_t=0.6,
                                              unfinished="nan", return_debug=True)
    cut = np.isnan(some)
    assert 0 < cut.sum() < 200
    np.testing.assert_array_equal(some[~cut], rts[~cut])
    assert np.all(d["n_steps"][cut] == 600) and np.all(d["n_steps"][~cut] <= 600)


@pytest.mark.gpu
def test_rows_that_cannot_be_simulated_fail_the_call(gpu):
    P, _ = rows_of(4)
    bad = P.copy()
    bad[1, 2] = 0.0
    with pytest.raises(RuntimeError, match=r"row 1\b"):
        gpu.gen_rts_from_drift_nodes(bad, 10, dt=DT, seed=1)
    bad = P.copy()
    bad[2, 3], bad[2, 4] = 0.95, 0.2  # z + sz / 2 > 1
    bad[3, 2] = float("nan")
    with pytest.raises(RuntimeError, match=r"row 2\b"):
        gpu.gen_rts_from_drift_nodes(bad, 10, dt=DT, seed=1)
    rts, off = gpu.gen_rts_from_drift_nodes(P, 10, dt=DT, seed=1)  # still usable
    assert rts.shape == (40,) and np.all(np.isfinite(rts))


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 1])
def test_device_draws_follow_the_dmat_cdf(gpu, i):
    from hddm_amd import cdfdif_wrapper
    rts, _ = gpu.gen_rts_from_drift_nodes(KS_ROWS[i:i + 1], KS_N, dt=DT, seed=KS_SEED)
    assert not np.isnan(rts).any()  # no draw ran out of steps under the default max_t
    draws = np.sort(rts)
    F = cdfdif_wrapper.dmat_cdf_array(draws, *KS_ROWS[i], 0.0, 0.1)
    d = ks_distance(draws, F)
    print(f"KS distance {d:.5f}, bound {KS_BOUND:.5f}")
    assert d < KS_BOUND


@pytest.mark.gpu
def test_gen_random_on_device(gpu):
    from hddm_amd import likelihoods
    parents = {"v": 0.5, "sv": 0.1, "a": 2.0, "z": 0.5, "sz": 0.1, "t": 0.3, "st": 0.1}
    np.random.seed(1)
    frame = likelihoods.gen_random(parents, 500, sampling_method="drift", sampling_dt=DT)
    assert list(frame.columns) == ["rt", "response"] and len(frame) == 500
    rt, resp = frame["rt"].to_numpy(), frame["response"].to_numpy()
    np.testing.assert_array_equal(resp, (rt > 0).astype(float))
    assert np.all(np.abs(rt) >= parents["t"] - parents["st"] / 2)
    assert 0 < resp.mean() < 1
    assert len(likelihoods.gen_random(parents, (7,), "drift", sampling_dt=DT)) == 7
    np.random.seed(11)
    plain = likelihoods.gen_random(SWITCH_PARENTS, 2000, "drift", sampling_dt=DT)["rt"].to_numpy()
    np.random.seed(12)
    switched = likelihoods.gen_random({**SWITCH_PARENTS, **SWITCH}, 2000, "drift",
                                      sampling_dt=DT)["rt"].to_numpy()
    gap = share_gap_in_standard_errors(plain, switched)
    print(f"lower shares {lower_share(plain):.3f} -> {lower_share(switched):.3f}, {gap:.1f} SE")
    assert gap > 4


@pytest.mark.gpu
def test_post_pred_gen_drift_on_device(gpu):
    from hddm_amd.hierarchical import HDDM, gen_data
    data, _ = gen_data(n_subj=8, n_trials=30, seed=3)
    m = HDDM(data, include=("st",), seed=4)
    m.sample(30, burn=10)
    assert m.n_nodes == 8
    cdf = m.post_pred_gen(samples=2, seed=11, dt=DT)
    frame = m.post_pred_gen(samples=2, seed=11, dt=DT, method="drift")
    assert list(frame.columns) == list(cdf.columns) == ["sample", "node", "rt", "response"]
    assert len(frame) == len(cdf) == 2 * len(data)
    for col in ("sample", "node"):
        np.testing.assert_array_equal(frame[col].to_numpy(), cdf[col].to_numpy())
    assert frame.dtypes.equals(cdf.dtypes)
    picked, P = m.post_pred_rows(2)
    k = np.searchsorted(picked, frame["sample"].to_numpy())
    node, rt = frame["node"].to_numpy(), frame["rt"].to_numpy()
    assert np.all(np.abs(rt) >= P[k, node, 5] - P[k, node, 6] / 2)
    np.testing.assert_array_equal(frame["response"].to_numpy(), (rt > 0).astype(int))
    assert np.any(rt != cdf["rt"].to_numpy())
    again = m.post_pred_gen(samples=2, seed=11, dt=DT, method="drift")
    np.testing.assert_array_equal(again["rt"].to_numpy(), rt)
    with pytest.raises(ValueError):
        m.post_pred_gen(samples=2, method="euler")
