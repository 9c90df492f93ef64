"""The batched on-device RT sampler (wfpt_gen_rts_nodes, sim_kernels.hip) and
HDDM.post_pred_gen.

References: the reference's gen_rts_from_cdf loop (wfpt.pyx:323-354, restated
in tests/golden/make_golden_genrts.py:35-52) over the oracle's densities
(oracle/wfpt_oracle.c, bit-exact to the reference's kernels), NumPy for the
exact logic, and the oracle's / the GPU's DMAT CDF (another algorithm) for the
distribution check. Tolerances:
  * running sum, normalisation, search, shift, device RNG, tiling: none
    (assert_array_equal);
  * densities: |log p_gpu - log p_ref| < 1e-6, the project's standing bar;
  * draws against the reference loop: at most max(1, n // 10_000) draws of a
    row on the adjacent grid point (tests/test_parity_strict.py:69-85: a draw
    can differ only where its uniform falls between the two versions of one
    normalised CDF value, |dF| ~ 1e-15);
  * KS distance to the DMAT CDF: 1.63 / sqrt(n) (1 % critical value) + dt *
    max grid density (the grid's own discretisation).
"""
import numpy as np
import pytest

# v, sv, a, z, sz, t, st
PARAM_ROWS = np.array([
    (0.5, 0.0, 2.0, 0.5, 0.0, 0.3, 0.0),       # simple DDM
    (0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1),       # the bench model: sv, sz, st
    (-1.2, 0.8, 1.4, 0.45, 0.25, 0.25, 0.0),   # negative v, sz = 0.25, no st
    (0.9, 0.0, 1.1, 0.35, 0.0, 0.4, 0.2),      # z off centre, st = 0.2 only
    (1.7, 2.0, 0.61, 0.54, 0.21, 0.36, 0.2),   # stress row (make_golden_genrts.py case 3)
    (-0.3, 0.5, 2.5, 0.6, 0.25, 0.2, 0.2),     # negative v, sz = 0.25 and st = 0.2
    (0.0, 0.0, 1.0, 0.5, 0.0, 0.1, 0.0),       # v = 0
    (2.5, 0.3, 1.8, 0.7, 0.0, 0.5, 0.05),      # sv only besides a small st
])
# (cdf_lb, cdf_ub, dt) -> grid length G. Grids 20, 65 and 257 contain exactly
# 0.0; grid 32 starts there, the one place a draw can land on it (f = 0).
GRIDS = {2: (0.5, 1.5, 0.5), 20: (-5, 5, 0.5), 32: (0.0, 4.0, 0.125), 65: (-4.0, 4.125, 0.125),
         257: (-4.0, 4.03125, 0.03125), 1200: (-6, 6, 1e-2), 12000: (-6, 6, 1e-3)}
COUNT_MIX = (0, 1, 63, 64, 65, 1000)


def grid_of(G):
    lb, ub, dt = GRIDS[G]
    x = np.arange(lb, ub, dt)
    assert x.shape[0] == G
    return x


def table(R):
    return PARAM_ROWS[np.arange(R) % len(PARAM_ROWS)]


def counts_of(R, shift=0):
    return np.array([COUNT_MIX[(r + shift) % len(COUNT_MIX)] for r in range(R)], dtype=np.int64)


# ---------------------------------------------------------------- restatements

def philox4x32_10(ctr, key):
    """Philox4x32-10: ctr (..., 4), key (..., 2) uint32 -> (..., 4) uint32."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1],
             p0 & mask]
        k = [(k[0] + np.uint64(0x9E3779B9)) & mask, (k[1] + np.uint64(0xBB67AE85)) & mask]
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_uniform(seed, row, draw, stream):
    """The device's uniform of (seed, global row, draw index in the row, stream)."""
    row, draw = np.broadcast_arrays(np.asarray(row, dtype=np.uint64),
                                    np.asarray(draw, dtype=np.uint64))
    ctr = np.stack([draw & np.uint64(0xFFFFFFFF), draw >> np.uint64(32), row,
                    np.full(row.shape, stream, dtype=np.uint64)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF],
                                   dtype=np.uint64), row.shape + (2,))
    w = philox4x32_10(ctr, key).astype(np.uint64)
    hi, lo = w[..., 0] >> np.uint64(5), w[..., 1] >> np.uint64(6)
    return (hi.astype(np.float64) * 67108864.0 + lo.astype(np.float64)) * 2.0 ** -53


def philox_streams(seed, counts):
    """(u_choice, u_delay) of a seeded call, row after row (the delay stream
    of every draw; the device leaves 0 where the row's st == 0)."""
    row = np.repeat(np.arange(len(counts)), counts)
    off = np.r_[0, np.cumsum(counts)]
    draw = np.arange(off[-1]) - off[row]
    return philox_uniform(seed, row, draw, 0), philox_uniform(seed, row, draw, 1)


def draws_from(x, l_cdf, f, u, t, st):
    """wfpt.pyx:345-352 on a normalised l_cdf (with its leading 0)."""
    rt = x[np.searchsorted(l_cdf, f)]
    if st == 0:
        return rt + np.sign(rt) * t
    return rt + np.sign(rt) * (u * st + (t - st / 2.))


_PDF_CACHE = {}


def oracle_pdf(oracle_lib, row, G):
    """The reference's grid densities of a parameter row (wfpt.pyx:335),
    computed once per (row, grid)."""
    key = (tuple(row[:5]), G)
    if key not in _PDF_CACHE:
        x = grid_of(G)
        v, sv, a, z, sz = row[:5]
        _PDF_CACHE[key] = oracle_lib.pdf_array(x[1:].copy(), v, sv, a, z, sz, 0.0, 0.0, 1e-4)
    return _PDF_CACHE[key]


def reference_row(oracle_lib, row, G, f, u):
    """make_golden_genrts.py:35-52 for one row with given uniforms."""
    x = grid_of(G)
    pdf = oracle_pdf(oracle_lib, row, G)
    l_cdf = np.empty(G)
    l_cdf[0] = 0
    l_cdf[1:] = np.cumsum(pdf)
    l_cdf /= l_cdf[G - 1]
    return draws_from(x, l_cdf, f, u, row[5], row[6])


def reference_loop(oracle_lib, P, counts, G):
    """A loop of reference gen_rts_from_cdf calls drawing from NumPy's global
    RNG: rand(n) and, when st != 0, rand(n) per row."""
    out = []
    for row, n in zip(P, counts):
        f = np.random.rand(int(n))
        u = np.random.rand(int(n)) if row[6] != 0 else None
        out.append(reference_row(oracle_lib, row, G, f, u))
    return out


def assert_rows_match(got, off, want, dt):
    for r, w in enumerate(want):
        g = got[off[r]:off[r + 1]]
        assert g.shape == w.shape
        diff = np.flatnonzero(g != w)
        assert diff.size <= max(1, w.size // 10_000), (r, diff[:10], g[diff[:5]], w[diff[:5]])
        if diff.size:  # the adjacent grid point only
            assert np.all(np.abs(np.abs(g[diff]) - np.abs(w[diff])) <= dt * (1 + 1e-6) + 1e-12)


def ks_distance(draws, cdf_values):
    """sup |F_n - F| from the CDF values at the sorted draws."""
    n = draws.size
    F = np.asarray(cdf_values)
    return max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n))


KS_ROW = PARAM_ROWS[1]
KS_N, KS_SEED, KS_GRID = 20_000, 20261019, 12000


# --------------------------------------------------------------------------- CPU

def test_entry_points_reject_bad_arguments_without_gpu():
    from hddm_amd import _lib
    assert _lib.wfpt_gen_rts_nodes(None, None, 0, None, 0, None, None, None, 0, 0, None) == 2
    assert b"null" in _lib.wfpt_last_error()
    assert _lib.wfpt_gen_rts_nodes_ex(None, None, 0, None, 0, None, None, None, 0, 0, None, None,
                                      None, None, None, None) == 2
    assert b"null" in _lib.wfpt_last_error()
    x = np.array([0.5])
    P = np.zeros((1, 8))
    cnt = np.array([3], dtype=np.int64)
    out = np.empty(3)
    args = (None, _lib.dptr(x), 1, P.ctypes.data_as(_lib._PP), 1,
            cnt.ctypes.data_as(_lib._PI64), None, None, 0, 0, _lib.dptr(out))
    assert _lib.wfpt_gen_rts_nodes(*args) == 2
    assert b"G < 2" in _lib.wfpt_last_error()
    assert _lib.wfpt_gen_rts_nodes_ex(*args, None, None, None, None, None) == 2
    assert b"G < 2" in _lib.wfpt_last_error()
    # a negative count and a lone uniform array, still without a device
    x2 = np.array([0.5, 1.0])
    neg = np.array([-1], dtype=np.int64)
    assert _lib.wfpt_gen_rts_nodes(None, _lib.dptr(x2), 2, P.ctypes.data_as(_lib._PP), 1,
                                   neg.ctypes.data_as(_lib._PI64), None, None, 0, 0,
                                   _lib.dptr(out)) == 2
    assert b"negative count" in _lib.wfpt_last_error()
    P[0, 6] = 0.1
    assert _lib.wfpt_gen_rts_nodes(None, _lib.dptr(x2), 2, P.ctypes.data_as(_lib._PP), 1,
                                   cnt.ctypes.data_as(_lib._PI64), _lib.dptr(out), None, 0, 0,
                                   _lib.dptr(out)) == 2
    assert b"u_delay" in _lib.wfpt_last_error()


def test_python_argument_checks_without_gpu(monkeypatch):
    from hddm_amd import _lib, wfpt

    def no_context(*a, **k):
        raise AssertionError("a context was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "context", no_context)
    assert "gen_rts_from_cdf_nodes" in wfpt.__all__
    with pytest.raises(ValueError):
        wfpt.gen_rts_from_cdf_nodes([[0.5, 0, 2, 0.5, 0, 0.3, 0], [0.5, 0, 2]], 5)
    with pytest.raises(ValueError):
        wfpt.gen_rts_from_cdf_nodes(np.zeros((2, 6)), 5)
    with pytest.raises(ValueError):
        wfpt.gen_rts_from_cdf_nodes(table(2), [5, -1])
    with pytest.raises(ValueError):
        wfpt.gen_rts_from_cdf_nodes(table(2), [5, 4, 3])
    with pytest.raises(ValueError):
        wfpt.gen_rts_from_cdf_nodes(table(1), 3, u=np.array([0.1, 1.0, 0.2]))
    with pytest.raises(ValueError):
        wfpt.gen_rts_from_cdf_nodes(table(1), 3, u=np.array([0.1, -1e-9, 0.2]))
    with pytest.raises(ValueError):  # row 1 has st != 0: the delays need uniforms too
        wfpt.gen_rts_from_cdf_nodes(table(2), 2, u=np.full(4, 0.5))
    with pytest.raises(ValueError):
        wfpt.gen_rts_from_cdf_nodes(table(2), 2, u=np.full(4, 0.5), u_delay=np.full(4, 1.5))


def test_philox_restatement_known_answers():
    """Random123's known-answer vectors of philox4x32_10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2,
            (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert [int(w) for w in got] == list(want)
    # the uniform of (seed, row, draw, stream) is the counter (draw lo, draw hi, row, stream)
    # under the key (seed lo, seed hi), 53 bits of the first two words
    seed, row, draw = 0x299f31d0a4093822, 0x13198a2e, 0x85a308d3243f6a88
    u = philox_uniform(seed, row, draw, 0x03707344)
    assert u == ((0xd16cfe09 >> 5) * 2.0 ** 26 + (0x94fdcceb >> 6)) * 2.0 ** -53
    assert 0 <= u < 1


def test_ks_seed_passes_with_the_reference_alone(oracle_lib):
    """The distribution check of test_draws_follow_the_dmat_cdf, with the
    reference's sampler (oracle densities, the same Philox uniforms) against
    the oracle's DMAT CDF: the chosen seed passes without the device."""
    x = grid_of(KS_GRID)
    f, u = philox_streams(KS_SEED, np.array([KS_N]))
    draws = np.sort(reference_row(oracle_lib, KS_ROW, KS_GRID, f, u))
    F = oracle_lib.dmat_cdf_array(draws, *KS_ROW, 0.0, 0.1)
    bound = 1.63 / np.sqrt(KS_N) + (x[1] - x[0]) * oracle_pdf(oracle_lib, KS_ROW, KS_GRID).max()
    d = ks_distance(draws, F)
    print(f"reference KS distance {d:.5f}, bound {bound:.5f}")
    assert d < bound


class _NoDataset:
    """Stand-in for hddm_amd.wfpt.Dataset: post_pred_gen scores nothing."""

    def __init__(self, rt, node_id=None, n_nodes=None, device=None):
        self.n_nodes = n_nodes


def test_post_pred_gen_row_table_and_frame(oracle_lib, monkeypatch):
    import pandas as pd
    from hddm_amd import hierarchical as h
    monkeypatch.setattr(h._wfpt, "Dataset", _NoDataset)
    calls = []

    def stand_in(params, samples, cdf_lb=-6, cdf_ub=6, dt=1e-2, seed=None, **kw):
        """The reference loop over the oracle's densities."""
        assert not kw
        calls.append((np.array(params), np.array(samples), seed))
        rs = np.random.RandomState(seed % 2 ** 32)
        x = np.arange(cdf_lb, cdf_ub, dt)
        out = []
        for (v, sv, a, z, sz, t, st, _), n in zip(params, samples):
            pdf = oracle_lib.pdf_array(x[1:].copy(), v, sv, a, z, sz, 0.0, 0.0, 1e-4)
            l_cdf = np.r_[0.0, np.cumsum(pdf)]
            l_cdf /= l_cdf[-1]
            f = rs.rand(int(n))
            u = rs.rand(int(n)) if st != 0 else None
            out.append(draws_from(x, l_cdf, f, u, t, st))
        return np.concatenate(out), np.r_[0, np.cumsum(samples)]
    monkeypatch.setattr(h._wfpt, "gen_rts_from_cdf_nodes", stand_in)

    rng = np.random.default_rng(5)
    rows = []
    for s in range(3):
        for c, n in (("lo", 7 + s), ("hi", 4)):
            xs = rng.choice([-1.0, 1.0], n, p=[0.3, 0.7]) * (0.3 + rng.gamma(2.0, 0.3, n))
            rows.append(pd.DataFrame({"rt": xs, "subj_idx": s, "cond": c}))
    m = h.HDDM(pd.concat(rows, ignore_index=True), depends_on={"v": "cond"},
               include=("sv", "sz", "st"), seed=0)
    with pytest.raises(RuntimeError):
        m.post_pred_gen(samples=2)  # sample() has not run
    kept = 9
    m.trace_subj = {"a": 1.5 + rng.uniform(0, 1, (kept, m.n_units["a"])),
                    "v": rng.normal(1, 0.5, (kept, m.n_units["v"])),
                    "t": 0.2 + rng.uniform(0, 0.2, (kept, m.n_units["t"]))}
    m.trace = {"sv": rng.uniform(0, 0.5, kept), "sz": rng.uniform(0, 0.2, kept),
               "st": rng.uniform(0, 0.2, kept)}
    frame = m.post_pred_gen(samples=4, seed=123, cdf_range=(-4, 4), dt=1e-2)
    (params, samples, seed), = calls
    assert seed == 123
    picked, P = m.post_pred_rows(4)
    assert list(picked) == [0, 3, 5, 8] and params.shape == (4 * m.n_nodes, 8)
    np.testing.assert_array_equal(params, P.reshape(-1, 8))
    for k, sweep in enumerate(picked):  # node_table at the sweep's values
        for fam in m.FAMILIES:
            m.subj[fam] = m.trace_subj[fam][sweep]
        for name in ("sv", "sz", "st"):
            m.inter[name] = float(m.trace[name][sweep])
        np.testing.assert_array_equal(P[k], m.node_table())
    node_n = np.array([dict(zip([(s, c) for s in range(3) for c in ("lo", "hi")],
                                [7, 4, 8, 4, 9, 4]))[key] for key in m.node_keys])
    np.testing.assert_array_equal(samples, np.tile(node_n, 4))
    assert list(frame.columns) == ["sample", "node", "rt", "response"]
    assert len(frame) == node_n.sum() * 4
    got_n = frame.groupby(["sample", "node"]).size().unstack().to_numpy()
    np.testing.assert_array_equal(got_n, np.tile(node_n, (4, 1)))
    assert sorted(frame["sample"].unique()) == [0, 3, 5, 8]
    np.testing.assert_array_equal(frame["response"].to_numpy(), (frame["rt"] > 0).astype(int))
    with pytest.raises(NotImplementedError):
        h.HDDMChains.post_pred_gen(m)


# --------------------------------------------------------------------------- GPU

def special_uniforms(cdf_row, n, rng):
    """n uniforms for one row: the off-by-one places first (0, the largest
    double below 1, knots of the row's CDF and their neighbours), then random."""
    m = cdf_row.shape[0]
    knots = cdf_row[np.unique(np.r_[0, m // 3, m // 2, m - 2 if m > 1 else 0, m - 1])]
    sp = np.r_[0.0, np.nextafter(1.0, 0.0), knots, np.nextafter(knots, 0.0),
               np.nextafter(knots, 2.0)]
    sp = sp[(sp >= 0) & (sp < 1)]
    return np.r_[sp, rng.random(max(n - sp.size, 0))][:n]


@pytest.mark.gpu
@pytest.mark.parametrize("G,R", [(2, 3), (20, 3), (32, 8), (65, 65), (257, 130), (1200, 1),
                                 (1200, 130), (12000, 3)])
def test_exact_logic(gpu, G, R):
    """Running sum, normalisation, search and shift against NumPy on the
    returned densities, bit for bit, with uniforms on the CDF's knots."""
    lb, ub, dt = GRIDS[G]
    x = grid_of(G)
    P, cnt = table(R), counts_of(R, shift=G % 5)
    rng = np.random.default_rng(G * 1000 + R)
    tot = int(cnt.sum())
    _, off, d0 = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt, u=rng.random(tot),
                                            u_delay=rng.random(tot), return_debug=True)
    u = np.concatenate([special_uniforms(d0["cdf"][r], int(cnt[r]), rng) for r in range(R)])
    ud = rng.random(tot)
    ud[:min(tot, 2)] = (0.0, np.nextafter(1.0, 0.0))[:min(tot, 2)]
    rts, off, d = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt, u=u, u_delay=ud,
                                             return_debug=True)
    np.testing.assert_array_equal(off, np.r_[0, np.cumsum(cnt)])
    np.testing.assert_array_equal(d["x"], x)
    np.testing.assert_array_equal(d["pdf"], d0["pdf"])
    cum = np.cumsum(d["pdf"], axis=1)
    np.testing.assert_array_equal(d["cdf"], cum / cum[:, -1:])
    np.testing.assert_array_equal(d["u"], u)
    for r in range(R):
        lo, hi = off[r], off[r + 1]
        l_cdf = np.r_[0.0, d["cdf"][r]]
        np.testing.assert_array_equal(d["idx"][lo:hi], np.searchsorted(l_cdf, u[lo:hi]))
        assert d["idx"][lo:hi].max(initial=0) <= G - 1
        np.testing.assert_array_equal(
            rts[lo:hi], draws_from(x, l_cdf, u[lo:hi], ud[lo:hi], P[r, 5], P[r, 6]))
    at_zero = x[d["idx"]] == 0.0  # sign(0) = 0: a draw on the grid's zero stays there
    assert np.all(rts[at_zero] == 0.0)
    if x[0] == 0.0:
        assert at_zero.sum() >= np.count_nonzero(cnt)


@pytest.mark.gpu
def test_grid_densities(gpu, oracle_lib):
    """Every parameter row on the 12000-point grid against the reference."""
    G = 12000
    lb, ub, dt = GRIDS[G]
    _, _, d = gpu.gen_rts_from_cdf_nodes(PARAM_ROWS, 1, lb, ub, dt, seed=1, return_debug=True)
    for r, row in enumerate(PARAM_ROWS):
        ref = oracle_pdf(oracle_lib, row, G)
        got = d["pdf"][r]
        pos = ref > 0
        assert pos.sum() > G // 2
        np.testing.assert_array_equal(got[~pos], ref[~pos])
        err = np.abs(np.log(got[pos]) - np.log(ref[pos])).max()
        assert err < 1e-6, (r, err)


@pytest.mark.gpu
@pytest.mark.parametrize("G,R", [(2, 3), (65, 65), (257, 130), (1200, 1), (1200, 130),
                                 (12000, 3)])
def test_draws_match_reference_loop(gpu, oracle_lib, G, R):
    lb, ub, dt = GRIDS[G]
    P, cnt = table(R), counts_of(R, shift=1)
    np.random.seed(77 + G)
    want = reference_loop(oracle_lib, P, cnt, G)
    np.random.seed(77 + G)
    got, off = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt)
    assert_rows_match(got, off, want, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("G,R", [(1200, 3), (12000, 8)])
def test_batched_call_equals_loop_of_single_calls(gpu, G, R):
    lb, ub, dt = GRIDS[G]
    P, cnt = table(R), counts_of(R, shift=2)
    np.random.seed(5)
    want = [gpu.gen_rts_from_cdf(*row, samples=int(n), cdf_lb=lb, cdf_ub=ub, dt=dt)
            for row, n in zip(P, cnt)]
    np.random.seed(5)
    got, off = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt)
    assert_rows_match(got, off, want, dt)


@pytest.mark.gpu
def test_tiling_does_not_change_a_bit(gpu):
    G, R = 257, 65
    lb, ub, dt = GRIDS[G]
    P, cnt = table(R), counts_of(R)
    one_row = 8 * (G - 1)
    rng = np.random.default_rng(3)
    u, ud = rng.random(int(cnt.sum())), rng.random(int(cnt.sum()))
    for kw in ({"u": u, "u_delay": ud}, {"seed": 99}):
        a, _, da = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt, return_debug=True, **kw)
        b, _, db = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt, return_debug=True,
                                              max_workspace=one_row, **kw)
        c, _ = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt, max_workspace=7 * one_row + 5, **kw)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
        for k in ("pdf", "cdf", "idx", "u", "u_delay"):
            np.testing.assert_array_equal(da[k], db[k])


@pytest.mark.gpu
def test_device_rng(gpu):
    G, R = 257, 70
    lb, ub, dt = GRIDS[G]
    P, cnt = table(R), counts_of(R)
    seed = 0x9E3779B97F4A7C15
    a, off, d = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt, seed=seed, return_debug=True)
    f, u = philox_streams(seed, cnt)
    has_st = np.repeat(P[:, 6] != 0, cnt)
    np.testing.assert_array_equal(d["u"], f)
    np.testing.assert_array_equal(d["u_delay"], np.where(has_st, u, 0.0))
    assert np.all((f >= 0) & (f < 1))
    fed, _ = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt, u=d["u"], u_delay=d["u_delay"])
    np.testing.assert_array_equal(a, fed)
    again, _ = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt, seed=seed)
    np.testing.assert_array_equal(a, again)
    other, _ = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt, seed=seed + 1)
    assert np.mean(a != other) > 0.5
    # a row's stream depends on its own index and draw index only
    cnt2 = counts_of(R, shift=3)
    r = 5
    cnt2[r] = cnt[r] = 1000
    a1, off1 = gpu.gen_rts_from_cdf_nodes(P, cnt, lb, ub, dt, seed=seed)
    a2, off2 = gpu.gen_rts_from_cdf_nodes(P, cnt2, lb, ub, dt, seed=seed)
    assert off1[r] != off2[r]
    np.testing.assert_array_equal(a1[off1[r]:off1[r + 1]], a2[off2[r]:off2[r + 1]])


@pytest.mark.gpu
def test_rows_without_a_cdf_fail_the_call(gpu):
    lb, ub, dt = GRIDS[257]
    P = table(4).copy()
    P[1, 2] = -1.0  # invalid: every density 0
    P[2, 2] = 0.0   # a == 0: NaN
    with pytest.raises(RuntimeError, match=r"row 1\b"):
        gpu.gen_rts_from_cdf_nodes(P, 10, lb, ub, dt, seed=1)
    with pytest.raises(RuntimeError, match=r"row 2\b"):
        gpu.gen_rts_from_cdf_nodes(P[[0, 3, 2]], 10, lb, ub, dt, seed=1)
    rts, off = gpu.gen_rts_from_cdf_nodes(table(4), 10, lb, ub, dt, seed=1)  # still usable
    assert rts.shape == (40,) and np.all(np.isfinite(rts))


@pytest.mark.gpu
def test_draws_follow_the_dmat_cdf(gpu):
    """20,000 seeded draws of the full DDM against the DMAT CDF (Tuerlinckx's
    series: another algorithm than the density grid)."""
    from hddm_amd import cdfdif_wrapper
    lb, ub, dt = GRIDS[KS_GRID]
    rts, _, d = gpu.gen_rts_from_cdf_nodes(KS_ROW[None, :], KS_N, lb, ub, dt, seed=KS_SEED,
                                           return_debug=True)
    draws = np.sort(rts)
    F = cdfdif_wrapper.dmat_cdf_array(draws, *KS_ROW, 0.0, 0.1)
    bound = 1.63 / np.sqrt(KS_N) + dt * d["pdf"].max()
    dist = ks_distance(draws, F)
    print(f"KS distance {dist:.5f}, bound {bound:.5f}")
    assert dist < bound


@pytest.mark.gpu
def test_post_pred_gen_on_device(gpu):
    from hddm_amd.hierarchical import HDDM, gen_data
    data, _ = gen_data(n_subj=4, n_trials=60, seed=3)
    m = HDDM(data, depends_on={"v": "cond"}, include=("st",), seed=4)
    m.sample(30, burn=10)
    frame = m.post_pred_gen(samples=5, seed=11, dt=1e-3)
    picked, P = m.post_pred_rows(5)
    assert m.n_nodes == 8 and picked.size == 5
    assert list(frame.columns) == ["sample", "node", "rt", "response"]
    assert len(frame) == 5 * len(data)
    sizes = frame.groupby(["sample", "node"]).size().unstack().to_numpy()
    np.testing.assert_array_equal(sizes, np.tile(m.node_counts, (5, 1)))
    k = np.searchsorted(picked, frame["sample"].to_numpy())
    node = frame["node"].to_numpy()
    rt = frame["rt"].to_numpy()
    assert np.all(np.abs(rt) > P[k, node, 5] - P[k, node, 6] / 2)
    np.testing.assert_array_equal(frame["response"].to_numpy(), (rt > 0).astype(int))
    again = m.post_pred_gen(samples=5, seed=11, dt=1e-3)
    np.testing.assert_array_equal(again["rt"].to_numpy(), rt)
