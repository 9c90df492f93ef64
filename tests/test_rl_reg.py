"""RL regression likelihood: RLRegDataset.wiener_like_rl_reg_groups /
wiener_like_rl_reg (rl_reg_kernels.hip: rl_reg_fill_kernel, then the Q scan and
the per-trial-parameter pass; hddm_rl_regression.py:25-38 into
wfpt.pyx:277-320).

Every stage has a defined arithmetic, so it is checked bit for bit: the
predictions against test_reg.restate_pred, the learning rates against the host
build of rl_update.hpp (tests/c/rl_rate_host.cpp), the drifts against a
plain-Python recurrence over those rates. The densities are checked against
the oracle's wiener_like_multi at the device's own drifts and predictions with
the project's bars (max|dlogp| < 1e-6 per trial, the total within 1e-9
relative of math.fsum), and the whole call bit for bit against
wfpt.wiener_like_multi_rlddm per group wherever the correctly rounded rate
equals the host libm rate.
"""
import functools
import inspect
import math

import numpy as np
import pytest

from test_gpu_parity import assert_logp_parity
from test_reg import FAMILIES, SIZES, restate_pred
from test_rl_rate import build_rate_host

G = len(SIZES)
RUNS = (1, 7, 8, 9, 70, 30)        # around kRlAhead = 8, one run over 64 ...
LABELS = (10, 11, 12, 13, 14, 11, 15)  # ... and condition 11 recurs after 14 (Q restarts)
# Chosen on the host builds alone (test_fixture_conditions): under either link
# the correctly rounded rate of the regressed alpha equals the host libm rate on
# every trial of exactly four of the five groups, so both parts of
# test_same_bits_as_multi_rlddm_with_a_regressed_alpha run.
SEED = 20261022
# design columns: 0-1 v, 2-3 alpha, 4-5 a, 6-7 t (each 1, cov)
COEF = np.array([2.0, 0.3, -1.0, 0.5, 0.59, 0.05, -1.39, 0.05])
TERM = {"v": ("v", 0, 2, "identity"), "alpha": ("alpha", 2, 2, "identity"),
        "a": ("a", 4, 2, "exp"), "t": ("t", 6, 2, "exp"),
        "alpha_logit": ("alpha", 2, 2, "invlogit")}
VARIANTS = {"full": ("v", "alpha", "a", "t"), "v_only": ("v",), "alpha_only": ("alpha",),
            "alpha_invlogit": ("v", "alpha_logit", "a", "t")}
KW = ("err", "n_st", "n_sz", "use_adaptive", "simps_err", "w_outlier")


@functools.lru_cache(maxsize=None)
def fixture():
    """1000 trials in five groups of sizes 1, 255, 256, 257, 231, ids shuffled
    over the trials; inside each group (in the caller's order) split_by runs of
    lengths 1, 7, 8, 9, 70, 30 and the rest, the sixth repeating the second's
    condition."""
    rng = np.random.default_rng(SEED)
    n = sum(SIZES)
    group = np.repeat(np.arange(G, dtype=np.int32), SIZES)
    rng.shuffle(group)
    split = np.empty(n, dtype=np.int64)
    for g in range(G):
        idx = np.flatnonzero(group == g)
        lab = np.repeat(LABELS[:len(RUNS)], RUNS)[:idx.size]  # the one-trial group: one run
        split[idx] = np.r_[lab, np.full(idx.size - lab.size, LABELS[-1])]
    cov = rng.normal(size=n)
    rt = np.sign(rng.uniform(-0.3, 0.7, n)) * (0.32 + rng.gamma(2.0, 0.25, n))
    response = (rt > 0).astype(np.int64)
    feedback = rng.binomial(1, np.where(response == 1, 0.8, 0.3)).astype(np.float64)
    X = np.column_stack([np.ones(n), cov] * 4).astype(np.float64)
    return rt, response, feedback, split, X, group


def tables(variant):
    """(model, coef_table (G, 8), q (G,), alpha (G,)) of a variant."""
    model = [TERM[k] for k in VARIANTS[variant]]
    table = COEF[None, :] * (1.0 + 0.02 * np.arange(G))[:, None]
    q = 0.5 - 0.02 * np.arange(G)
    alpha = -1.2 + 0.3 * np.arange(G)
    return model, table, q, alpha


def params(F):
    P = np.tile([0.0, F["sv"], 1.8, F["z"], F["sz"], 0.25, F["st"], F["p_outlier"]], (G, 1))
    P[:, 0] = 2.0 + 0.1 * np.arange(G)
    P[:, 3] = F["z"] - 0.01 * np.arange(G)
    return P


def kw_of(F):
    return {k: F[k] for k in KW}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def runs_of(sel_split):
    """[(first, last + 1)] of the runs of equal adjacent values."""
    cut = np.flatnonzero(np.r_[True, sel_split[1:] != sel_split[:-1], True])
    return list(zip(cut[:-1].tolist(), cut[1:].tolist()))


def recurrence(response, feedback, split, q, rate, vmul):
    """wfpt.pyx:298-318 in plain Python floats over one group's trials: the
    drift is one subtraction and one product, the update three roundings, Q
    restarts at every run."""
    drift = np.empty(response.size)
    for lo, hi in runs_of(split):
        qs = [float(q), float(q)]
        for i in range(lo, hi):
            drift[i] = (qs[1] - qs[0]) * float(vmul[i])
            r = int(response[i])
            d = float(feedback[i]) - qs[r]
            prod = float(rate[i]) * d
            qs[r] = qs[r] + prod
    return drift


@pytest.fixture(scope="module")
def rates(tmp_path_factory):
    return build_rate_host(str(tmp_path_factory.mktemp("rl_reg") / "librl_rate_host.so"))


def alpha_pred(X, table, group, link):
    out = np.empty(X.shape[0])
    for g in range(G):
        sel = group == g
        out[sel] = restate_pred(X[sel], table[g], 2, 2, link)
    return out


# ---------------------------------------------------------------------------
# CPU tests

def test_rl_reg_signatures():
    from hddm_amd import wfpt
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert "RLRegDataset" in wfpt.__all__
    assert sig(wfpt.RLRegDataset.__init__)[1:] == [
        ("rt", E), ("response", E), ("feedback", E), ("split_by", E), ("design", E),
        ("group_id", None), ("n_groups", None), ("device", None), ("ctx", None)]
    assert sig(wfpt.RLRegDataset.wiener_like_rl_reg_groups)[1:] == [
        ("model", E), ("coef_table", E), ("q", E), ("alpha", E), ("params", E), ("err", 1e-4),
        ("n_st", 2), ("n_sz", 2), ("use_adaptive", 1), ("simps_err", 1e-3), ("w_outlier", 0.1),
        ("terms", False)]
    assert sig(wfpt.RLRegDataset.wiener_like_rl_reg)[1:] == [
        ("model", E), ("coef", E), ("q", E), ("alpha", E), ("v", E), ("sv", E), ("a", E),
        ("z", E), ("sz", E), ("t", E), ("st", E), ("err", E), ("n_st", 10), ("n_sz", 10),
        ("use_adaptive", 1), ("simps_err", 1e-3), ("p_outlier", 0), ("w_outlier", 0),
        ("terms", False)]


def test_rl_reg_shape_errors_without_gpu():
    from hddm_amd import wfpt
    one, X = np.ones(3), np.ones((3, 2))
    r = np.array([0, 1, 1])
    mk = wfpt.RLRegDataset
    for args, kw in (((one, r, one, r, np.ones(3)), {}),          # 1-D design
                     ((one, r, one, r, np.ones((4, 2))), {}),     # rows != trials
                     ((one, r, one, r, np.ones((3, 0))), {}),     # no columns
                     ((one, r[:2], one, r, X), {}),               # response != trials
                     ((one, r, one[:2], r, X), {}),               # feedback != trials
                     ((one, r, one, r[:2], X), {}),               # split_by != trials
                     ((one, np.array([0, 2, 1]), one, r, X), {}),  # response outside {0, 1}
                     ((np.array([1.0, -999.0, 1.0]), r, one, r, X), {}),  # no missing code
                     ((one, r, one, r, X), dict(group_id=[0, 1])),         # ids != trials
                     ((one, r, one, r, X), dict(group_id=[0, 1, 5], n_groups=2))):
        with pytest.raises(ValueError):
            mk(*args, **kw)
    # alpha is a term of this class only
    T, nt = wfpt._reg_terms([("alpha", 1, 1, "invlogit"), ("v", 0, 1, "identity")], 2,
                            wfpt.RL_REG_PARAMS)
    assert nt == 2 and (T[0].param, T[0].link, T[0].col0, T[0].ncol) == (7, 2, 1, 1)
    with pytest.raises(ValueError, match="unknown parameter 'alpha'"):
        wfpt._reg_terms([("alpha", 0, 1, "identity")], 2)
    # the call's shapes, before any device work: a bare instance has no handle
    d = object.__new__(mk)
    d.n, d.n_cols, d.n_groups, d.grouped = 6, 2, 3, True
    good = ([("alpha", 0, 2, "identity")], np.ones((3, 2)), np.ones(3), np.ones(3),
            np.ones((3, 8)))
    for pos, bad in ((0, [("q", 0, 1, "identity")]), (0, [("alpha", 1, 2, "identity")]),
                     (0, [("alpha", 0, 1, "identity"), ("alpha", 1, 1, "identity")]),
                     (1, np.ones((2, 2))), (1, np.ones((3, 3))), (2, np.ones(2)),
                     (3, np.ones(4)), (4, np.ones((3, 7)))):
        args = list(good)
        args[pos] = bad
        with pytest.raises(ValueError):
            d.wiener_like_rl_reg_groups(*args)
    with pytest.raises(ValueError, match="without group ids"):
        d.wiener_like_rl_reg(good[0], np.ones(2), 0.5, 0.0, 1, 0, 2, .5, 0, .3, 0, 1e-4)
    d.grouped, d.n_groups = False, 1
    with pytest.raises(ValueError, match="one entry per design column"):
        d.wiener_like_rl_reg(good[0], np.ones(3), 0.5, 0.0, 1, 0, 2, .5, 0, .3, 0, 1e-4)


def test_rl_reg_entry_points_reject_bad_arguments_without_gpu():
    from hddm_amd import _lib
    two = 2
    assert _lib.wfpt_rl_reg_dataset_create(None, None, None, None, None, 0, None, 1, None, 0,
                                           None) == two
    assert b"null" in _lib.wfpt_last_error()
    _lib.wfpt_rl_reg_dataset_destroy(None)
    good = (_lib.RegTerm * 1)(_lib.RegTerm(7, 0, 0, 1))
    for fn, tail in ((_lib.wfpt_wiener_like_rl_reg_groups, ()),
                     (_lib.wfpt_wiener_like_rl_reg_groups_ex, (None, None, None, None))):
        assert fn(None, None, good, 1, None, None, None, None, None, None, *tail) == two
        assert b"null" in _lib.wfpt_last_error()
        for term, word in ((_lib.RegTerm(8, 0, 0, 1), b"outside 0..7"),
                           (_lib.RegTerm(-1, 0, 0, 1), b"outside 0..7"),
                           (_lib.RegTerm(7, 0, 0, 0), b"ncol < 1"),
                           (_lib.RegTerm(7, 0, -1, 1), b"column range"),
                           (_lib.RegTerm(7, 3, 0, 1), b"link")):
            bad = (_lib.RegTerm * 1)(term)
            assert fn(None, None, bad, 1, None, None, None, None, None, None, *tail) == two
            assert word in _lib.wfpt_last_error(), (term.param, _lib.wfpt_last_error())
        twice = (_lib.RegTerm * 2)(_lib.RegTerm(7, 0, 0, 1), _lib.RegTerm(7, 0, 1, 1))
        assert fn(None, None, twice, 2, None, None, None, None, None, None, *tail) == two
        assert b"twice" in _lib.wfpt_last_error()
        assert fn(None, None, good, 9, None, None, None, None, None, None, *tail) == two
    # the regression entries keep rejecting alpha with their message
    assert _lib.wfpt_wiener_like_reg_groups(None, None, good, 1, None, None, None, None) == two
    assert b"outside 0..6" in _lib.wfpt_last_error()


def test_fixture_conditions(rates):
    """What the GPU tests rely on, from the host builds alone: the group sizes
    and run lengths, and that the correctly rounded rate of the regressed alpha
    equals the host libm rate on every trial of at least four of the five
    groups (both links)."""
    rt, response, feedback, split, X, group = fixture()
    assert np.bincount(group).tolist() == list(SIZES)
    for g in range(1, G):
        s = split[group == g]
        lens = [hi - lo for lo, hi in runs_of(s)]
        assert lens[:6] == list(RUNS) and lens[6] > 64 and s[lens[0]] == s[sum(lens[:5])]
    assert np.abs(rt).min() > 0.3
    _, table, _, _ = tables("full")
    for link in ("identity", "invlogit"):
        al = alpha_pred(X, table, group, link)
        same = bits(rates["rl_rate"](al)) == bits(rates["libm_rl_rate"](al))
        exact = [g for g in range(G) if same[group == g].all()]
        assert len(exact) == 4, (link, exact)


# ---------------------------------------------------------------------------
# GPU tests

@pytest.fixture(scope="module")
def ds(gpu):
    rt, response, feedback, split, X, group = fixture()
    d = gpu.RLRegDataset(rt, response, feedback, split, X, group_id=group, n_groups=G)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def call(ds, variant, fam):
    model, table, q, alpha = tables(variant)
    F = FAMILIES[fam]
    return ds.wiener_like_rl_reg_groups(model, table, q, alpha, params(F), **kw_of(F), terms=True)


def inputs_of(variant, fam, pred, rate):
    """Per trial: (drift scaling, a, t) as the call used them."""
    _, _, _, _, _, group = fixture()
    P = params(FAMILIES[fam])
    vm = pred["v"] if "v" in pred else P[group, 0]
    a = pred["a"] if "a" in pred else P[group, 2]
    t = pred["t"] if "t" in pred else P[group, 5]
    return vm, a, t


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_predictions_rates_and_drifts_bit_for_bit(gpu, ds, rates, variant):
    rt, response, feedback, split, X, group = fixture()
    model, table, q, alpha = tables(variant)
    sums, terms, pred, drift, rate = call(ds, variant, "simple")
    assert list(pred) == [m[0] for m in model]
    for g in range(G):
        sel = group == g
        for name, c0, nc, link in model:  # 1. predictions
            want = restate_pred(X[sel], table[g], c0, nc, link)
            assert np.array_equal(bits(pred[name][sel]), bits(want)), (variant, name, g)
    if "alpha" in pred:  # 2. rates: the host build of the same header
        want = rates["rl_rate"](pred["alpha"])
    else:  # the group's alpha through the host's libm route
        want = rates["libm_rl_rate"](alpha)[group]
    assert np.array_equal(bits(rate), bits(want)), variant
    vm, _, _ = inputs_of(variant, "simple", pred, rate)
    for g in range(G):  # 3. drifts
        sel = group == g
        want = recurrence(response[sel], feedback[sel], split[sel], q[g], rate[sel], vm[sel])
        assert np.array_equal(bits(drift[sel]), bits(want)), (variant, g)
        lo = [r[0] for r in runs_of(split[sel])]
        assert np.all(drift[sel][lo] == 0.0)  # Q restarts per run and per group


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["simple", "full"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_densities_against_the_oracle(gpu, ds, oracle_lib, variant, fam):
    rt, _, _, _, _, group = fixture()
    F = FAMILIES[fam]
    P = params(F)
    sums, terms, pred, drift, rate = call(ds, variant, fam)
    _, a, t = inputs_of(variant, fam, pred, rate)
    for g in range(G):
        sel = group == g
        _, want = oracle_lib.wiener_like_multi(
            rt[sel], drift[sel], F["sv"], a[sel], P[g, 3], F["sz"], t[sel], F["st"], F["err"],
            multi=["v", "a", "t"], n_st=F["n_st"], n_sz=F["n_sz"],
            use_adaptive=F["use_adaptive"], simps_err=F["simps_err"], p_outlier=F["p_outlier"],
            w_outlier=F["w_outlier"], terms=True)
        d = np.abs(terms[sel] - want)
        print(f"{variant} {fam} group {g}: max|dlogp| {d.max():.3e}")
        assert_logp_parity(terms[sel], want, f"{variant} {fam} group {g}")
        tot = math.fsum(want)
        assert abs(sums[g] - tot) < 1e-9 * abs(tot), (variant, fam, g, sums[g], tot)
    # the call without the extra outputs returns the same sums
    model, table, q, alpha = tables(variant)
    again = ds.wiener_like_rl_reg_groups(model, table, q, alpha, P, **kw_of(F))
    assert np.array_equal(bits(again), bits(sums))


def multi_rlddm(gpu, sel, pred, q, alpha, P_g, F, names):
    """wfpt.wiener_like_multi_rlddm on one group's trials with the call's own
    predicted arrays; alpha: scalar or per-trial array."""
    rt, response, feedback, split, _, _ = fixture()
    vals = dict(v=P_g[0], sv=F["sv"], a=P_g[2], z=P_g[3], sz=F["sz"], t=P_g[5], st=F["st"],
                alpha=alpha)
    vals.update({k: pred[k][sel] for k in names if k != "alpha"})
    return gpu.wiener_like_multi_rlddm_terms(
        rt[sel], response[sel], feedback[sel], split[sel], q,
        *[vals[k] for k in ("v", "sv", "a", "z", "sz", "t", "st", "alpha")], F["err"],
        multi=list(names), n_st=F["n_st"], n_sz=F["n_sz"], use_adaptive=F["use_adaptive"],
        simps_err=F["simps_err"], p_outlier=F["p_outlier"], w_outlier=F["w_outlier"])


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["simple", "full"])
def test_same_bits_as_multi_rlddm_with_a_scalar_alpha(gpu, ds, fam):
    """alpha not regressed: group g is bit for bit wiener_like_multi_rlddm on
    its trials with the predicted arrays and the scalar alpha."""
    _, _, _, _, _, group = fixture()
    F = FAMILIES[fam]
    P = params(F)
    _, _, q, alpha = tables("v_only")
    sums, terms, pred, drift, _ = call(ds, "v_only", fam)
    for g in range(G):
        sel = group == g
        tot, tr, dr = multi_rlddm(gpu, sel, pred, q[g], alpha[g], P[g], F, ("v",))
        assert np.array_equal(bits(dr), bits(drift[sel])), (fam, g)
        assert np.array_equal(bits(tr), bits(terms[sel])), (fam, g)
        assert bits(tot) == bits(sums[g]), (fam, g, tot, sums[g])


@pytest.mark.gpu
def test_one_group_form(gpu):
    """A data set made without group ids: wiener_like_rl_reg over all trials
    equals wiener_like_multi_rlddm on them, bit for bit."""
    rt, response, feedback, split, X, _ = fixture()
    F = FAMILIES["full"]
    one = gpu.RLRegDataset(rt, response, feedback, split, X)
    model = [TERM["v"], TERM["a"], TERM["t"]]
    args = (0.45, -0.7, 0.0, F["sv"], 0.0, F["z"], F["sz"], 0.0, F["st"], F["err"])
    kw = dict(n_st=F["n_st"], n_sz=F["n_sz"], use_adaptive=F["use_adaptive"],
              simps_err=F["simps_err"], p_outlier=F["p_outlier"], w_outlier=F["w_outlier"])
    tot, terms, pred, drift, rate = one.wiener_like_rl_reg(model, COEF, *args, **kw, terms=True)
    assert one.wiener_like_rl_reg(model, COEF, *args, **kw) == tot
    want = gpu.wiener_like_multi_rlddm_terms(
        rt, response, feedback, split, 0.45, pred["v"], F["sv"], pred["a"], F["z"], F["sz"],
        pred["t"], F["st"], -0.7, F["err"], multi=["v", "a", "t"], **kw)
    assert bits(want[0]) == bits(tot)
    assert np.array_equal(bits(want[1]), bits(terms))
    assert np.array_equal(bits(want[2]), bits(drift))
    with pytest.raises(ValueError):
        one.wiener_like_rl_reg_groups(model, np.ones((2, 8)), [0.5], [0.0], np.ones((1, 8)))
    one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["full", "alpha_invlogit"])
def test_same_bits_as_multi_rlddm_with_a_regressed_alpha(gpu, ds, rates, variant):
    """alpha regressed: bit for bit in every group whose trials all have the
    host libm rate equal to out_rate; elsewhere each trial within 1e-6."""
    _, _, _, _, _, group = fixture()
    F = FAMILIES["simple"]
    P = params(F)
    _, _, q, _ = tables(variant)
    sums, terms, pred, drift, rate = call(ds, variant, "simple")
    same = bits(rates["libm_rl_rate"](pred["alpha"])) == bits(rate)
    exact = [g for g in range(G) if same[group == g].all()]
    print(f"{variant}: {int((~same).sum())} of {same.size} rates differ from libm's; "
          f"bit-for-bit groups {exact}")
    assert len(exact) >= 4, exact
    for g in range(G):
        sel = group == g
        tot, tr, dr = multi_rlddm(gpu, sel, pred, q[g], pred["alpha"][sel], P[g], F,
                                  ("v", "a", "t", "alpha"))
        if g in exact:
            assert np.array_equal(bits(dr), bits(drift[sel])), (variant, g)
            assert np.array_equal(bits(tr), bits(terms[sel])), (variant, g)
            assert bits(tot) == bits(sums[g]), (variant, g)
        else:
            assert np.abs(tr - terms[sel]).max() < 1e-6, (variant, g)


@pytest.mark.gpu
def test_groups_are_independent_and_an_empty_group_is_zero(gpu, ds):
    rt, response, feedback, split, X, group = fixture()
    F = FAMILIES["full"]
    model, table, q, alpha = tables("full")
    P = params(F)
    base = call(ds, "full", "full")[0]
    for keep in (0, 3):
        t2, q2, a2, P2 = table * 1.1, q + 0.1, alpha - 1.0, P.copy()
        P2[:, 1:7] = [0.2, 1.5, 0.45, F["sz"], 0.2, F["st"]]  # sz, st: the same scoring runs
        for arr, src in ((t2, table), (q2, q), (a2, alpha), (P2, P)):
            arr[keep] = src[keep]
        got = ds.wiener_like_rl_reg_groups(model, t2, q2, a2, P2, **kw_of(F))
        assert bits(got[keep]) == bits(base[keep]), keep
        assert np.all(bits(np.delete(got, keep)) != bits(np.delete(base, keep)))
    # an empty group in the middle: 0.0, the others the bits they had
    wide = gpu.RLRegDataset(rt, response, feedback, split, X,
                            group_id=np.where(group >= 2, group + 1, group), n_groups=G + 1)
    ins = lambda a: np.insert(a, 2, a[2], axis=0)
    got, terms, _, _, _ = wide.wiener_like_rl_reg_groups(model, ins(table), ins(q), ins(alpha),
                                                         ins(P), **kw_of(F), terms=True)
    assert got[2] == 0.0 and bits(got[2]) == 0
    assert np.array_equal(bits(np.delete(got, 2)), bits(base))
    assert np.array_equal(bits(terms), bits(call(ds, "full", "full")[1]))
    wide.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["coef", "alpha"])
def test_a_nan_row_stays_in_its_group(gpu, ds, oracle_lib, what):
    """A NaN coefficient (of the v term) or a NaN alpha[g] in one group: that
    group's sum has the class (NaN, -inf or finite) the oracle gives at the
    device's own drifts and predictions; every other group keeps its bits
    (tests/test_invalid_rows.py's rules for wiener_like_reg_groups)."""
    from test_invalid_rows import total_class
    rt, _, _, _, _, group = fixture()
    F = FAMILIES["simple"]
    variant = "full" if what == "coef" else "v_only"
    model, table, q, alpha = tables(variant)
    P = params(F)
    base, bterms = call(ds, variant, "simple")[:2]
    bad_g = 3
    table, alpha = table.copy(), alpha.copy()
    if what == "coef":
        table[bad_g, 1] = np.nan
    else:
        alpha[bad_g] = np.nan
    sums, terms, pred, drift, rate = ds.wiener_like_rl_reg_groups(model, table, q, alpha, P,
                                                                  **kw_of(F), terms=True)
    sel = group == bad_g
    _, a, t = inputs_of(variant, "simple", pred, rate)
    ref_tot, want = oracle_lib.wiener_like_multi(
        rt[sel], drift[sel], F["sv"], a[sel], P[bad_g, 3], F["sz"], t[sel], F["st"], F["err"],
        multi=["v", "a", "t"], n_st=F["n_st"], n_sz=F["n_sz"], use_adaptive=F["use_adaptive"],
        simps_err=F["simps_err"], p_outlier=F["p_outlier"], w_outlier=F["w_outlier"], terms=True)
    assert np.isnan(drift[sel]).any()
    assert_logp_parity(terms[sel], want, what)
    assert total_class(sums[bad_g]) == total_class(ref_tot) == "nan", (sums[bad_g], ref_tot)
    others = np.arange(G) != bad_g
    assert np.array_equal(bits(sums[others]), bits(base[others])), what
    assert np.array_equal(bits(terms[~sel]), bits(bterms[~sel])), what
