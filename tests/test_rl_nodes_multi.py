"""wfpt_wiener_like_rlddm_nodes_multi: the RL node batch over several row tables
in one call. Every row must equal, bit for bit, the one-table call on that
table (sums, per-trial terms, drifts); the drifts equal the restated reference
loop exactly and the terms lie within the project's 1e-6 of the oracle.
"""
import numpy as np
import pytest

from test_rl import (DDM, HDDM_KNOBS, ROW_A, ROW_B, ROW_C, _node_data, make_data, oracle_terms,
                     restate_rlddm)

K = dict(HDDM_KNOBS, w_outlier=0.1)
ROWS = np.array([ROW_A, ROW_B, ROW_C])
#                  v    sv    a    z     sz   t     st    p_outlier
BASE = np.array([[2.4, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 0.05],
                 [-1.6, 0.2, 1.7, 0.45, 0.1, 0.28, 0.1, 0.05],
                 [3.0, 0.0, 2.2, 0.55, 0.1, 0.32, 0.1, 0.05]])


def _tables(T):
    """T tables over three nodes that differ in every column but sz, st and
    p_outlier, with ROW_A/B/C permuted from table to table."""
    rl = np.stack([np.roll(ROWS, t, axis=0) for t in range(T)])
    pm = np.stack([BASE + 0.013 * t * np.array([1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0])
                   for t in range(T)])
    for t in range(T):
        pm[t] = np.roll(pm[t], -t, axis=0)
    return rl, pm


def _check_rows(gpu, ds, rl, pm, oracle=None, data=None):
    """Row t of the multi call against the one-table call on table t; with
    `oracle` and `data` also against the restatement and the oracle."""
    T = rl.shape[0]
    sums, terms, drift = ds.wiener_like_rlddm_nodes_multi(rl, pm, **K, terms=True)
    assert sums.shape == (T, ds.n_nodes) and terms.shape == drift.shape == (T, ds.n)
    assert np.array_equal(ds.wiener_like_rlddm_nodes_multi(rl, pm, **K), sums)
    assert np.array_equal(gpu.wiener_like_rlddm_nodes_multi(ds, rl, pm, **K), sums)
    for t in range(T):
        s1, t1, d1 = ds.wiener_like_rlddm_nodes(rl[t], pm[t], **K, terms=True)
        assert np.array_equal(sums[t], s1), (t, sums[t], s1)
        assert np.array_equal(terms[t], t1), t
        assert np.array_equal(drift[t], d1), t
        if oracle is None:
            continue
        (x, response, feedback, split_by), node = data
        for j in range(ds.n_nodes):
            sel = node == j
            F = dict(zip(("v",) + DDM + ("p_outlier",), pm[t, j]), **K)
            want_drift, scored = restate_rlddm(response[sel], feedback[sel], split_by[sel],
                                               *rl[t, j], F["v"])
            assert np.array_equal(drift[t][sel], want_drift)
            if scored.any():
                want = oracle_terms(oracle, x[sel][scored], want_drift[scored], F)
                d = float(np.max(np.abs(terms[t][sel][scored] - want)))
                print(f"table {t} node {j}: max|dlogp|={d:.3e}")
                assert d < 1e-6
            assert np.all(terms[t][sel][~scored] == 0.0)
    return sums


def test_rl_nodes_multi_shape_refusals_without_gpu():
    """Shape errors raise before any device call: the dataset here has no
    device side at all."""
    from hddm_amd import _lib, wfpt
    ds = wfpt.RLDataset.__new__(wfpt.RLDataset)
    ds.n_nodes, ds.n, ds.handle, ds.ctx = 3, 10, None, None
    rl, pm = np.zeros((2, 3, 3)), np.zeros((2, 3, 8))
    for bad_rl, bad_pm in ((rl[0], pm[0]), (rl[:, :2], pm), (rl[:, :, :2], pm), (rl, pm[:1]),
                           (rl, pm[:, :, :7]), (rl, pm[:, :2]), (rl[:0], pm[:0]),
                           (np.zeros((0, 3, 3)), np.zeros((0, 3, 8)))):
        with pytest.raises(ValueError):
            ds.wiener_like_rlddm_nodes_multi(bad_rl, bad_pm)
        with pytest.raises(ValueError):
            wfpt.wiener_like_rlddm_nodes_multi(ds, bad_rl, bad_pm)
    ds.n_nodes = 0
    with pytest.raises(ValueError):
        ds.wiener_like_rlddm_nodes_multi(rl, pm)
    ds.handle = None  # nothing to destroy
    assert "wiener_like_rlddm_nodes_multi" in wfpt.__all__
    two = 2  # WFPT_ERR_ARG
    assert _lib.wfpt_wiener_like_rlddm_nodes_multi(None, None, None, None, 1, None, None) == two
    assert b"null" in _lib.wfpt_last_error()
    assert _lib.wfpt_wiener_like_rlddm_nodes_multi_ex(None, None, None, None, 0, None, None,
                                                      None, None) == two


@pytest.fixture(scope="module")
def nodes(gpu):
    data = _node_data()
    (x, response, feedback, split_by), node = data
    ds = gpu.RLDataset(x, response, feedback, split_by, node_id=node, n_nodes=3)
    yield ds, data
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 3])
def test_rl_nodes_multi_rows_equal_the_one_table_call(gpu, oracle_lib, nodes, T):
    ds, data = nodes
    assert (ds.n - 8) % 256 != 0  # 8 segments: table 1 starts mid-block and mid-wave
    rl, pm = _tables(T)
    _check_rows(gpu, ds, rl, pm, oracle_lib, data)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["table-st", "node-st", "family-between"])
def test_rl_nodes_multi_run_splitting(gpu, nodes, case):
    ds, _ = nodes
    rl, pm = _tables(3)
    if case == "table-st":      # one table's st differs from the others'
        pm[1, :, 6] = 0.15
    elif case == "node-st":     # one node's st differs inside a table
        pm[1, 1, 6] = 0.15
    else:                       # sz = st = 0: another integration family between two full tables
        pm[1, :, 4] = 0.0
        pm[1, :, 6] = 0.0
    _check_rows(gpu, ds, rl, pm)


@pytest.mark.gpu
def test_rl_nodes_multi_table_boundary_inside_a_scan_wave(gpu, oracle_lib):
    """65 segments of 1 to 5 trials, 13 per node: T = 2 gives 130 scan lanes,
    three waves, with the table boundary at lane 65."""
    lengths = [1 + (k % 5) for k in range(65)]
    x, response, feedback, split_by = make_data(12, lengths)
    node = (split_by // 13).astype(np.int32)
    ds = gpu.RLDataset(x, response, feedback, split_by, node_id=node, n_nodes=5)
    rl = np.stack([np.array([ROW_A, ROW_B, ROW_C, ROW_A, ROW_B]),
                   np.array([ROW_C, ROW_A, ROW_B, ROW_B, ROW_C])])
    pm = np.stack([np.tile(BASE[0], (5, 1)), np.tile(BASE[1], (5, 1))])
    pm[0, :, 0] += np.arange(5) * 0.1
    pm[1, :, 5] -= np.arange(5) * 0.01
    _check_rows(gpu, ds, rl, pm, oracle_lib, ((x, response, feedback, split_by), node))
    ds.close()


@pytest.mark.gpu
def test_rl_nodes_multi_special_values(gpu, nodes):
    ds, ((x, response, feedback, split_by), node) = nodes
    rl, pm = _tables(2)
    # a node made only of one-trial segments has no scored trial: exactly 0.0
    n1 = 6
    x1 = np.concatenate([x, np.full(n1, 0.9)])
    r1 = np.concatenate([response, np.ones(n1, dtype=np.int64)])
    f1 = np.concatenate([feedback, np.ones(n1)])
    s1 = np.concatenate([split_by, 100 + np.arange(n1, dtype=np.int64)])
    node1 = np.concatenate([node, np.full(n1, 3, dtype=np.int32)])
    d1 = gpu.RLDataset(x1, r1, f1, s1, node_id=node1, n_nodes=4)
    rl4 = np.concatenate([rl, rl[:, :1]], axis=1)
    pm4 = np.concatenate([pm, pm[:, :1]], axis=1)
    sums = _check_rows(gpu, d1, rl4, pm4)
    assert np.all(sums[:, 3] == 0.0) and np.all(np.isfinite(sums))
    d1.close()
    # t above an |rt| with p_outlier = 0: -inf for that (table, node) only
    pz = pm.copy()
    pz[:, :, 7] = 0.0
    ok = ds.wiener_like_rlddm_nodes_multi(rl, pz, **K)
    assert np.all(np.isfinite(ok))
    pz[1, 2, 5] = float(np.median(np.abs(x[node == 2])))  # above half the node's |rt|
    got = _check_rows(gpu, ds, rl, pz)
    assert got[1, 2] == -np.inf
    mask = np.ones_like(got, dtype=bool)
    mask[1, 2] = False
    assert np.array_equal(got[mask], ok[mask])
    # p_outlier outside [0, 1]: every sum -inf; differing between tables: refused
    po = pm.copy()
    po[:, :, 7] = 1.5
    assert np.all(ds.wiener_like_rlddm_nodes_multi(rl, po, **K) == -np.inf)
    po = pm.copy()
    po[1, :, 7] = 0.06
    with pytest.raises(NotImplementedError):
        ds.wiener_like_rlddm_nodes_multi(rl, po, **K)
    po = pm.copy()
    po[1, 2, 7] = 0.06
    with pytest.raises(NotImplementedError):
        ds.wiener_like_rlddm_nodes_multi(rl, po, **K)


@pytest.mark.gpu
def test_rl_nodes_multi_leaves_the_other_paths_unchanged(gpu, nodes):
    """Shared scratch buffers and the dataset's replicated view: Dataset.wiener_like,
    Dataset.wiener_like_multi and the one-table node batch return after multi
    calls (growing, then smaller) what they returned before."""
    ds, ((x, *_), _) = nodes
    rl, pm = _tables(3)
    args = (0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 1e-4)
    kn = dict(n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, p_outlier=0.05, w_outlier=0.1)
    plain = gpu.Dataset(x)
    ordered = gpu.Dataset(x, input_order=True)
    margs = (np.linspace(-1.0, 2.0, x.size), 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 1e-4)

    def others():
        one = ds.wiener_like_rlddm_nodes(rl[0], pm[0], **K, terms=True)
        return (plain.wiener_like(*args, **kn), ordered.wiener_like_multi(*margs, ["v"], **kn),
                *[a.tobytes() for a in one])

    before = others()
    big = ds.wiener_like_rlddm_nodes_multi(rl, pm, **K)
    assert others() == before
    small = ds.wiener_like_rlddm_nodes_multi(rl[:2], pm[:2], **K)  # fewer tables than replicated
    assert np.array_equal(small, big[:2])
    assert others() == before
    for d in (plain, ordered):
        d.close()
