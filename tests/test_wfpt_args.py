"""The samplers' argument rules hold once for the plain and the fused path
(hddm_amd.wfpt: gen_rts_from_cdf_nodes / gen_rts_from_drift_nodes against
gen_rts_stats_nodes), and the binding's list of entry points is its table of
signatures.

The refusals fire before any context is opened, so they run without a device;
their messages are the ones both paths gave before they shared the checks.
"""
import numpy as np
import pytest

from test_sim import PARAM_ROWS

P3 = PARAM_ROWS[:3]  # st = 0, 0.1, 0
P3_NO_ST = PARAM_ROWS[[0, 2, 6]]
BAD_TABLE = "params must have shape (R, 7) or (R, 8), R >= 1"

# (method, params, samples, keywords, message); a seed wherever the call would
# otherwise get as far as drawing from NumPy's global RNG
REFUSALS = [
    ("cdf", np.ones((3, 6)), 2, {}, BAD_TABLE),
    ("cdf", P3[0], 2, {}, BAD_TABLE),
    ("cdf", np.empty((0, 7)), 2, {}, BAD_TABLE),
    ("cdf", P3, [1, 2], {}, "samples must be an int or 3 ints"),
    ("cdf", P3, -1, {}, "samples must be non-negative"),
    ("cdf", P3, [1, -2, 3], {}, "samples must be non-negative"),
    ("cdf", P3, [1., 2., 3.], {}, "samples must be an int or 3 ints"),
    ("cdf", P3, 2, {"u_delay": np.zeros(6)}, "u_delay needs u"),
    ("cdf", P3_NO_ST, 2, {"u": np.zeros(5)}, "u must hold sum(samples) = 6 uniforms"),
    ("cdf", P3_NO_ST, [0, 5, 70], {"u": np.zeros(76)}, "u must hold sum(samples) = 75 uniforms"),
    ("cdf", P3_NO_ST, 2, {"u": np.array([0, .5, 1., 0, 0, 0])}, "u must lie in [0, 1)"),
    ("cdf", P3_NO_ST, 2, {"u": np.array([0, .5, -1e-9, 0, 0, 0])}, "u must lie in [0, 1)"),
    ("cdf", P3, 2, {"u": np.zeros(6)}, "u_delay is needed: a row has st != 0"),
    ("cdf", P3, 2, {"u": np.zeros(6), "u_delay": np.zeros(7)},
     "u_delay must hold sum(samples) = 6 uniforms"),
    ("cdf", P3, 2, {"u": np.zeros(6), "u_delay": np.array([0, 0, 0, 1., 0, 0])},
     "u_delay must lie in [0, 1)"),
    ("cdf", P3, 2, {"seed": 1, "cdf_lb": 0, "cdf_ub": 0.01, "dt": 0.01},
     "the grid np.arange(cdf_lb, cdf_ub, dt) needs at least two points"),
    ("cdf", P3, 2, {"seed": 1, "max_workspace": -1}, "max_workspace must be positive"),
    # two at once: the earlier check speaks
    ("cdf", np.ones((3, 6)), [1, 2], {"u_delay": np.zeros(6)}, BAD_TABLE),
    ("cdf", P3, [1, 2], {"u_delay": np.zeros(6)}, "samples must be an int or 3 ints"),
    ("cdf", P3, 2, {"u": np.zeros(5), "max_workspace": -1},
     "u must hold sum(samples) = 6 uniforms"),
    ("cdf", P3, 2, {"seed": 1, "cdf_lb": 0, "cdf_ub": 0.01, "dt": 0.01, "max_workspace": -1},
     "the grid np.arange(cdf_lb, cdf_ub, dt) needs at least two points"),
    ("drift", np.ones((3, 6)), 2, {}, BAD_TABLE),
    ("drift", P3, [1, 2], {}, "samples must be an int or 3 ints"),
    ("drift", P3, -1, {}, "samples must be non-negative"),
    ("drift", P3, [1., 2., 3.], {}, "samples must be an int or 3 ints"),
    ("drift", P3, 2, {"dt": 0}, "dt must be positive"),
    ("drift", P3, 2, {"dt": -1e-3}, "dt must be positive"),
    ("drift", P3, 2, {"dt": float("inf")}, "dt must be positive"),
    ("drift", P3, 2, {"dt": float("nan")}, "dt must be positive"),
    ("drift", P3, 2, {"intra_sv": 0}, "intra_sv must be positive"),
    ("drift", P3, 2, {"intra_sv": float("inf")}, "intra_sv must be positive"),
    ("drift", P3, 2, {"max_t": 0}, "max_t must be positive"),
    ("drift", P3, 2, {"max_t": float("nan")}, "max_t must be positive"),
    ("drift", P3, 2, {"max_t": 20., "dt": 1e-9}, "ceil(max_t / dt) must lie in [1, 2^31]"),
    ("drift", P3, 2, {"unfinished": "skip"}, "unfinished must be 'raise' or 'nan'"),
    ("drift", P3, 2, {"switch": np.ones((3, 2))},
     "switch must have shape (3, 3): v_switch, V_switch, t_switch"),
    ("drift", P3, 2, {"switch": [[1., 0., 1e-5]] * 3, "dt": 1e-4},
     "t_switch / dt must round to at least one step"),
    # two at once: the earlier check speaks
    ("drift", np.ones((3, 6)), 2, {"dt": 0}, BAD_TABLE),
    ("drift", P3, 2, {"dt": 0, "intra_sv": 0}, "dt must be positive"),
    ("drift", P3, 2, {"intra_sv": 0, "max_t": 0}, "intra_sv must be positive"),
    ("drift", P3, 2, {"max_t": 0, "unfinished": "skip"}, "max_t must be positive"),
    ("drift", P3, 2, {"unfinished": "skip", "switch": np.ones((3, 2))},
     "unfinished must be 'raise' or 'nan'"),
]


def _refusal(call):
    with pytest.raises(Exception) as info:
        call()
    return type(info.value), str(info.value)


@pytest.mark.parametrize("method,params,samples,kw,message", REFUSALS,
                         ids=[f"{r[0]}-{i}" for i, r in enumerate(REFUSALS)])
def test_plain_and_fused_sampler_refuse_alike(method, params, samples, kw, message):
    from hddm_amd import wfpt
    plain = wfpt.gen_rts_from_cdf_nodes if method == "cdf" else wfpt.gen_rts_from_drift_nodes
    state = np.random.get_state()[1].copy()
    want = (ValueError, message)
    assert _refusal(lambda: plain(params, samples, **kw)) == want
    for draws in (False, True):
        assert _refusal(lambda: wfpt.gen_rts_stats_nodes(params, samples, method,
                                                         return_draws=draws, **kw)) == want
    np.testing.assert_array_equal(np.random.get_state()[1], state)  # refused before any draw


def test_plain_drift_sampler_checks_its_own_arguments_last():
    """row0 and wave_draws are the plain sampler's alone: they are looked at
    after the shared checks and before a seed is taken from the global RNG."""
    from hddm_amd import wfpt
    for kw, message in (({"row0": -1}, "row0 must lie in [0, 2^31)"),
                        ({"row0": 2 ** 31}, "row0 must lie in [0, 2^31)"),
                        ({"wave_draws": 65}, "wave_draws must be a positive multiple of 64"),
                        ({"row0": -1, "unfinished": "skip"}, "unfinished must be 'raise' or 'nan'"),
                        ({"row0": -1, "wave_draws": 65}, "row0 must lie in [0, 2^31)")):
        state = np.random.get_state()[1].copy()
        assert _refusal(lambda: wfpt.gen_rts_from_drift_nodes(P3, 2, **kw)) == (ValueError, message)
        np.testing.assert_array_equal(np.random.get_state()[1], state)
    with pytest.raises(TypeError):
        wfpt.gen_rts_stats_nodes(P3, 2, "drift", row0=1)


def test_exported_is_the_table_of_signatures():
    """Every name in EXPORTED is a bound module attribute; only the two
    optional diagnostics may be absent from an older library."""
    from hddm_amd import _lib
    optional = {"wfpt_profile_lists", "wfpt_debug_waves"}
    assert optional <= set(_lib.EXPORTED) and len(set(_lib.EXPORTED)) == len(_lib.EXPORTED)
    for name in _lib.EXPORTED:
        f = getattr(_lib, name)
        if f is None:
            assert name in optional and not hasattr(_lib._lib, name)
            continue
        assert f.argtypes is not None and f.__name__ == name, name


def _rng_state():
    s = np.random.get_state()
    return s[0], s[1].tobytes(), s[2:]


@pytest.mark.gpu
def test_plain_and_fused_samplers_consume_the_global_rng_alike(gpu):
    """Without a seed both paths draw the same uniforms from NumPy's global
    RNG: rand(n_r) and, for a row with st != 0, rand(n_r), row after row (the
    CDF sampler), and two 32-bit words (the drift sampler's seed)."""
    cnt = (0, 5, 70)
    assert list(P3[:, 6] != 0) == [False, True, False]
    kw = dict(cdf_lb=-5, cdf_ub=5, dt=0.5)
    np.random.seed(7)
    a, off = gpu.gen_rts_from_cdf_nodes(P3, cnt, **kw)
    after_plain = _rng_state()
    np.random.seed(7)
    _, off_f, b = gpu.gen_rts_stats_nodes(P3, cnt, "cdf", return_draws=True, **kw)
    assert _rng_state() == after_plain
    np.testing.assert_array_equal(off_f, off)
    np.testing.assert_array_equal(b, a)
    np.random.seed(7)
    gpu.gen_rts_stats_nodes(P3, cnt, "cdf", **kw)  # the draws stay on the device
    assert _rng_state() == after_plain
    np.random.seed(7)
    u5, d5, u70 = np.random.rand(5), np.random.rand(5), np.random.rand(70)
    assert _rng_state() == after_plain
    u, ud = np.r_[u5, u70], np.r_[d5, np.zeros(70)]
    np.testing.assert_array_equal(gpu.gen_rts_from_cdf_nodes(P3, cnt, u=u, u_delay=ud, **kw)[0], a)
    assert _rng_state() == after_plain  # supplied uniforms: the global RNG is left alone

    np.random.seed(7)
    a, off = gpu.gen_rts_from_drift_nodes(P3, cnt, dt=1e-3)
    after_plain = _rng_state()
    np.random.seed(7)
    _, off_f, b = gpu.gen_rts_stats_nodes(P3, cnt, "drift", return_draws=True, dt=1e-3)
    assert _rng_state() == after_plain
    np.testing.assert_array_equal(off_f, off)
    np.testing.assert_array_equal(b, a)
    np.random.seed(7)
    lo, hi = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint64)
    assert _rng_state() == after_plain
    seeded = gpu.gen_rts_from_drift_nodes(P3, cnt, dt=1e-3, seed=int(lo) | (int(hi) << 32))[0]
    np.testing.assert_array_equal(seeded, a)
    assert _rng_state() == after_plain
