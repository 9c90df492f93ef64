"""Out-of-range and NaN parameter rows on every batched path.

Three rules of the reference hold at the edge of the parameter space:
  * an invalid row (pdf.pxi:111-113) has a density of exactly 0, so each term
    is -inf, or log(w_outlier p_outlier) under an outlier mixture;
  * a NaN parameter passes the validity test (every comparison is false) and
    propagates as NaN (a NaN sz or st is not zeroed by the < 1e-3 test either:
    its integral is NaN), and a == 0 gives 0 / 0 = NaN;
  * wiener_like_multi scores a +-999 trial with prob_ub and applies no
    validity test to it (wfpt.pyx:267-271).
A sampler meets them constantly (z +- sz/2 and t - st/2 are not bounded by the
priors, an identity link predicts negative a or t for single trials, a slice
probe steps past a bound), and every kernel carries its own copy of the
validity handling. The cases are one module-level table (CASES) applied to a
valid row of each integration family.

Every expected value is the oracle's (oracle/wfpt_oracle.c), a Python
restatement the suite already has (restate_pred, restate_rlddm), or the bits
of another call of the library (a valid call before and after an invalid one;
the valid nodes of a table with and without invalid neighbours).

NaN rows and loop bounds (read before the first run): a NaN reaches the
series term count only through tt = (x - t) / a^2. decide32 rejects a tt
outside (1e-30, 1e30), NaN included; decide64 then gives kl = NaN, ks = 2, so
the large-time branch with K = ref_int(ceil(NaN)) = INT_MIN and no series
term (a == 0: tt = inf, K = 0); a NaN t makes x - t NaN, which is not > 0, so
the node has no series at all; NaN v and z enter values only, and a NaN sz or st
makes the z grid or the t nodes NaN in the same way. l0_hints shares
a decision only when x - ub > 0, which is false for NaN. Every stop test
reads NaN as "refine", but simpson_refine returns false at bottom <= 0
first, so a tree ends at depth n_st / n_sz (tree17, adaptive_walk, the exact
path's walk, whose stack and evaluation budget are capped besides). The
engine's rounds run over at most kTreeDepth levels of at most kQCap queued
tasks each, which is what a fully refining chunk queues.
"""
import math
from typing import NamedTuple

import numpy as np
import pytest

from test_gpu_parity import assert_logp_parity
from test_parity_summing import (KN, PINNED, SIMPLE, ST_ONLY, STRESS, SZ_ONLY, assert_chunks,
                                 assert_terms, path_names, ref_terms, summing_vs_trials)
from test_parity_trials import _ctx_env, node_terms_ref
from test_reg import FAMILIES as REG_FAMILIES
from test_reg import fixture as reg_data
from test_reg import oracle_multi, reg_args, reg_kw, restate_pred
from test_rl import FAMILIES as RL_FAMILIES
from test_rl import (ROW_A, ROW_B, ROW_C, _node_data, make_data, oracle_terms, restate_rlddm,
                     rlddm_args, rlddm_kw)

NAMES = ("v", "sv", "a", "z", "sz", "t", "st")
NAN = float("nan")
OUTLIERS = ((0.0, 0.0), (0.05, 0.1))  # p_outlier, w_outlier
BASES = {"simple": SIMPLE, "pinned": PINNED, "st_only": ST_ONLY, "sz_only": SZ_ONLY}


class Case(NamedTuple):
    name: str
    set: dict     # the overrides that make the row invalid (or NaN)
    axis: str     # "": the row keeps its base's family; "sz" / "st": the case sets that
    #               variability, so the family is the base's only if the base's sz (st) falls
    #               on the same side of full_pdf's < 1e-3 zeroing (pdf.pxi:122-123)
    repair: dict  # overrides of the valid row of the same family as the case's row


INVALID = (
    Case("a<0", dict(a=-0.1), "", {}),
    Case("z>1", dict(z=1.1), "", {}),
    Case("z<0", dict(z=-0.1), "", {}),
    Case("z-sz/2<0", dict(z=0.1, sz=0.25), "sz", dict(sz=0.25)),
    Case("z+sz/2>1", dict(z=0.9, sz=0.25), "sz", dict(sz=0.25)),
    Case("sz>1", dict(sz=1.2), "sz", dict(sz=0.25)),
    Case("sz<0", dict(sz=-0.1), "sz", dict(sz=0.0)),   # zeroed: the family without sz
    Case("t<0", dict(t=-0.3), "", {}),
    Case("t-st/2<0", dict(t=0.04, st=0.1), "st", dict(st=0.1)),
    Case("st<0", dict(st=-0.1), "st", dict(st=0.0)),   # zeroed: the family without st
    Case("sv<0", dict(sv=-0.2), "", {}),
)
NANS = (
    Case("v=nan", dict(v=NAN), "", {}),
    Case("a=nan", dict(a=NAN), "", {}),
    Case("t=nan", dict(t=NAN), "", {}),
    Case("z=nan", dict(z=NAN), "", {}),
    Case("a=0", dict(a=0.0), "", {}),
    # not below the zeroing threshold: the reference integrates over a NaN interval
    Case("sz=nan", dict(sz=NAN), "sz", dict(sz=0.25)),
    Case("st=nan", dict(st=NAN), "st", dict(st=0.1)),
)
CASES = INVALID + NANS


def apply(base, overrides):
    row = dict(zip(NAMES, base))
    row.update(overrides)
    return tuple(float(row[k]) for k in NAMES)


def family(row):
    """(sz integrated, st integrated) after full_pdf's zeroing (pdf.pxi:122-123)."""
    return (not row[4] < 1e-3, not row[6] < 1e-3)


def keeps_family(base, case):
    return family(apply(base, case.set)) == family(base)


def row_invalid(v, sv, a, z, sz, t, st):
    """The tests of pdf.pxi:111-113 that do not involve x (arrays broadcast; a
    NaN fails none of them)."""
    with np.errstate(invalid="ignore"):
        return ((z < 0) | (z > 1) | (a < 0) | (t < 0) | (st < 0) | (sv < 0) | (sz < 0) |
                (sz > 1) | (z + sz / 2. > 1) | (z - sz / 2. < 0) | (t - st / 2. < 0))


def knobs(po, w, use_adaptive=1):
    """KN (HDDM's knobs) with another mixture / Simpson variant."""
    return (KN[0], KN[1], KN[2], use_adaptive, KN[4], po, w)


def assert_layout(bad, what):
    """bad: the invalid trials in the stored (device) order. At least two
    64-trial waves hold both kinds; an invalid trial sits at lane 0 and at
    lane 63 of a wave, and is the first and the last trial of a 256-trial
    block."""
    bad = np.asarray(bad, dtype=bool)
    n = bad.size
    nw = (n + 63) // 64
    inv = np.zeros(nw * 64, dtype=bool)
    inv[:n] = bad
    val = np.zeros(nw * 64, dtype=bool)
    val[:n] = ~bad
    inv, val = inv.reshape(nw, 64), val.reshape(nw, 64)
    mixed = inv.any(axis=1) & val.any(axis=1)
    assert mixed.sum() >= 2, (what, "mixed waves", int(mixed.sum()))
    assert inv[:, 0].any() and inv[:, 63].any(), (what, "lanes 0 / 63")
    assert bad[0::256].any(), (what, "first trial of a 256-trial block")
    assert bad[255::256].any(), (what, "last trial of a 256-trial block")
    assert val.any() and inv.any(), what


def total_class(v):
    return "nan" if math.isnan(v) else ("-inf" if v == -math.inf else "finite")


# --------------------------------------------------------------------------- fixtures (host)

# B. ~20 nodes of sizes from {0, 1, 3, 63, 64, 65, 130} in a fixed shuffled order. Stored
# trials (grouped by node): node 0 = 0..63 (wave 0), node 4 = 197..259 (the last trial of
# block 0 and the first of block 1), node 13 = 651, node 15 = 716..845; node 10 is empty.
NODE_SIZES = (64, 3, 130, 0, 63, 1, 65, 64, 130, 3, 0, 63, 65, 1, 64, 130, 3, 65, 63, 1)
NODE_BAD = (0, 4, 9, 10, 13, 15)


def node_dataset():
    rng = np.random.default_rng(20261019)
    node = np.repeat(np.arange(len(NODE_SIZES)), NODE_SIZES)
    rng.shuffle(node)
    # every |rt| above every row's t + st / 2 <= 0.3 + 0.1: no zero density in a valid row
    x = rng.choice([-1.0, 1.0], node.size) * (0.42 + rng.gamma(2.0, 0.4, node.size))
    return x, node


def node_stored_bad(x, node):
    """The invalid trials in the dataset's stored order: grouped by node, by
    |rt| inside a node (wfpt_dataset_create_ex)."""
    order = np.lexsort((np.abs(x), node))
    return np.isin(node[order], NODE_BAD)


def node_rounds(base_name, keep):
    """[(cases of the NODE_BAD rows, has_nan)]: every case of the kind, six rows
    per table; the NaN cases in tables of their own."""
    base = BASES[base_name]
    inv = [c for c in INVALID if keeps_family(base, c) == keep]
    nans = [c for c in NANS if keeps_family(base, c) == keep]
    out = []
    for pool, has_nan in ((inv, False), (nans, True)):
        for r in range(0, len(pool), len(NODE_BAD)):
            out.append(([pool[(r + k) % len(pool)] for k in range(len(NODE_BAD))], has_nan))
    return out


def node_tables(base_name, cases, po):
    """(table with the invalid rows, the same with those rows repaired)."""
    base = BASES[base_name]
    m = len(NODE_SIZES)
    rng = np.random.default_rng(7 + sorted(BASES).index(base_name))
    good = np.tile(np.append(np.asarray(base, dtype=np.float64), po), (m, 1))
    good[:, 0] = rng.uniform(-2, 2, m)
    good[:, 2] = rng.uniform(0.8, 2.0, m)
    good[:, 3] = rng.uniform(0.4, 0.6, m)
    good[:, 5] = rng.uniform(0.2, 0.3, m)
    bad, fix = good.copy(), good.copy()
    for j, case in zip(NODE_BAD, cases):
        bad[j, :7] = apply(good[j, :7], case.set)
        fix[j, :7] = apply(good[j, :7], case.repair)
    return bad, fix


# C. per-trial parameters, n = 600 (input order is the stored order)
MULTI_N = 600
MULTI_FAMILIES = {"direct": dict(sv=0.0, sz=0.0, st=0.0), "adapt_t": dict(sv=0.3, sz=0.0, st=0.1),
                  "adapt_z": dict(sv=0.3, sz=0.2, st=0.0),
                  "adapt_tz": dict(sv=0.3, sz=0.2, st=0.1)}
MULTI_CONFIGS = [(c, f) for c in ("va", "vaz") for f in MULTI_FAMILIES] + [("generic", "adapt_tz")]
MULTI_PLACED = (0, 63, 64, 101, 206, 255, 256, 309, 511, 599)  # lanes 0 / 63, block edges, +-999
MULTI_KN = dict(n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3)
MULTI_NAN = {"va": dict(a=(7, 412), v=(11, 202)), "vaz": dict(z=(7, 412), a=(11,), v=(202,)),
             "generic": dict(t=(7, 412), v=(11, 202), sz=(13,), st=(17,))}  # 202: 999, 412: -999


def multi_fixture(config, fam, with_nan):
    """x, the seven parameters (arrays for those in `multi`), multi. +-999 sit
    on invalid rows (0, 101, 206, 309) and on valid ones."""
    rng = np.random.default_rng(31 + [c for c, _ in MULTI_CONFIGS].index(config))
    n = MULTI_N
    x = rng.choice([-1.0, 1.0], n) * (0.42 + rng.gamma(2.0, 0.4, n))
    x[::101] = 999.0
    x[::103] = -999.0
    bad = rng.random(n) < 0.1
    bad[list(MULTI_PLACED)] = True
    kind = rng.integers(0, 4, n)  # which invalid value a bad trial takes
    kind[x == 999.0] = 0          # (z = 1.1 / -0.1 there: prob_ub outside [0, 1], but the
    kind[x == -999.0] = 1         # term's argument stays positive)
    p = dict(v=rng.uniform(-1.5, 1.5, n), a=1.5, z=0.5, t=0.25, **MULTI_FAMILIES[fam])
    if config == "va":
        multi = ["v", "a"]
        p["a"] = np.where(bad, -0.2, rng.uniform(0.8, 2.2, n))
    elif config == "vaz":
        multi = ["v", "a", "z"]
        p["a"] = rng.uniform(0.8, 2.2, n)
        # outside [0, 1], or inside with z +- sz / 2 across a bound (sz = 0.2 families)
        z_bad = np.choose(kind, [1.1, -0.1, 0.03, 0.97])
        if p["sz"] == 0:
            z_bad = np.where(kind < 2, z_bad, np.where(kind == 2, 1.1, -0.1))
        p["z"] = np.where(bad, z_bad, rng.uniform(0.4, 0.6, n))
    else:
        multi = ["v", "sz", "st", "t"]
        p["sz"] = np.where(bad & (kind == 0), 1.2, np.where(bad & (kind == 1), -0.1,
                                                             rng.uniform(0.0, 0.3, n)))
        p["st"] = np.where(bad & (kind == 2), -0.1, rng.uniform(0.0, 0.2, n))
        p["t"] = np.where(bad & (kind == 3), np.where(rng.random(n) < 0.5, -0.3, 0.04),
                          rng.uniform(0.2, 0.3, n))
        p["st"] = np.where(bad & (kind == 3) & (p["t"] > 0), 0.1, p["st"])
    if with_nan:
        for k, idx in MULTI_NAN[config].items():
            p[k] = p[k].copy()
            p[k][list(idx)] = NAN
    args = [p[k] for k in NAMES]
    return x, args, multi


def multi_bad(args):
    return np.broadcast_to(row_invalid(*args), (MULTI_N,))


# D. test_reg.py's fixture, a ~ 1 + cov and t ~ 1 + cov through the identity link: a < 0 for
# cov < -4/3 (9 % of a standard normal), t < 0 for cov > 2.5
REG_MODEL = [("v", 0, 4, "identity"), ("a", 4, 2, "identity"), ("t", 6, 2, "identity")]
REG_COEF = np.array([0.7, 0.45, -0.3, 0.25, 1.6, 1.2, 0.2, -0.08])
REG_BAD_GROUP = 2  # 256 trials: stored 256..511 of the grouped layout


def reg_fixture():
    """(rt, X, group) of test_reg.fixture() with three design rows exchanged so
    that trial 1 (a -999), trial 255 and trial 256 have a predicted a < 0."""
    rt, X, group = reg_data()
    X = X.copy()
    a = restate_pred(X, REG_COEF, 4, 2, "identity")
    donors = [int(i) for i in np.flatnonzero(a < 0) if i > 256][:3]
    for dst, src in zip((1, 255, 256), donors):
        X[[dst, src]] = X[[src, dst]]
    return rt, X, group


def reg_pred(X):
    return {m[0]: restate_pred(X, REG_COEF, m[1], m[2], m[3]) for m in REG_MODEL}


# --------------------------------------------------------------------------- CPU tests

def test_oracle_rules_on_the_table(oracle_lib):
    """The oracle on CASES x the four family bases (adaptive and fixed
    Simpson): an invalid row has density exactly 0, so every term is -inf
    without a mixture and one repeated value within 1 ulp of
    math.log(w_outlier p_outlier) with it; a NaN row gives NaN; +-999 trials
    of wiener_like_multi on an invalid row keep their finite prob_ub term.
    The same through the reference's own compiled full_pdf where it is built."""
    x = np.array([0.6, -0.6, 1.3, -2.0, 0.45, -0.43, 3.1, -0.9])
    R = oracle_lib.load_ref()
    for bname, base in BASES.items():
        assert not row_invalid(*base) and np.all(np.abs(x) > base[5] + base[6] / 2)
        for case in CASES:
            row = apply(base, case.set)
            assert bool(row_invalid(*row)) == (case in INVALID), (bname, case.name)
            assert not row_invalid(*apply(base, case.repair)), (bname, case.name)
            assert family(apply(base, case.repair)) == family(row), (bname, case.name)
            assert set(case.set) & {"sz", "st"} == ({case.axis} if case.axis else set())
            for ua in (1, 0):
                dens = [oracle_lib.full_pdf(xi, *row, KN[0], KN[1], KN[2], ua, KN[4]) for xi in x]
                if R is not None:
                    rdens = [R.full_pdf(xi, *row, KN[0], KN[1], KN[2], ua, KN[4]) for xi in x]
                    assert np.array_equal(rdens, dens, equal_nan=True), (bname, case.name, ua)
                for po, w in OUTLIERS:
                    what = (bname, case.name, ua, po)
                    kn = knobs(po, w, ua)
                    terms = ref_terms(oracle_lib, x, row, kn)
                    tot = oracle_lib.wiener_like(x, *row, *kn)
                    if case in NANS:
                        assert np.all(np.isnan(dens)) and np.all(np.isnan(terms)), what
                        assert math.isnan(tot), what
                    elif po == 0:
                        assert dens == [0.0] * x.size, what
                        assert np.all(np.isneginf(terms)) and tot == -math.inf, what
                    else:
                        want = math.log(w * po)
                        assert np.all(terms == terms[0]), what
                        assert abs(terms[0] - want) <= math.ulp(want), what
                        assert abs(tot - x.size * want) <= 8 * x.size * math.ulp(tot), what
        # the table names both kinds for every base (the node and multi tests need both)
        kept = [keeps_family(base, c) for c in INVALID]
        assert any(kept) and not all(kept), bname
        assert all(keeps_family(base, c) for c in CASES if not c.axis), bname
    # wiener_like_multi: a per-trial a = -0.2 on an RT and on +-999 (wfpt.pyx:261-271)
    xm = np.array([0.8, 999.0, -999.0, -0.7])
    for po, w in OUTLIERS:
        _, terms = oracle_lib.wiener_like_multi(xm, 0.4, 0.1, np.full(4, -0.2), 0.5, 0.1, 0.3, 0.1,
                                                KN[0], multi=["a"], p_outlier=po, w_outlier=w,
                                                terms=True, **MULTI_KN)
        assert np.all(np.isfinite(terms[1:3])), (po, terms)
        assert terms[1] == math.log(oracle_lib.prob_ub(0.4, -0.2, 0.5))
        if po == 0:
            assert terms[0] == -math.inf and terms[3] == -math.inf
        else:
            assert terms[0] == terms[3] and abs(terms[0] - math.log(w * po)) <= math.ulp(terms[0])


def test_fixture_conditions(oracle_lib):
    """What the GPU tests rely on, from sizes and indices alone: every node,
    multi and regression fixture has two or more 64-trial waves holding both
    valid and invalid trials, an invalid trial at lanes 0 and 63 of a wave and
    as the first and the last trial of a 256-trial block; the regression
    coefficients predict 5-15 % negative a and a few negative t; the multi
    fixtures reach the reference's three classes of total."""
    # B
    x, node = node_dataset()
    assert set(NODE_SIZES) == {0, 1, 3, 63, 64, 65, 130} and len(NODE_SIZES) == 20
    assert np.array_equal(np.bincount(node, minlength=20), NODE_SIZES)
    assert not np.array_equal(node, np.sort(node))  # the caller's order is not the stored one
    assert_layout(node_stored_bad(x, node), "nodes")
    assert 0 in [NODE_SIZES[j] for j in NODE_BAD]  # an invalid row without trials
    for bname in BASES:
        for keep in (True, False):
            rounds = node_rounds(bname, keep)
            seen = {c.name for cases, _ in rounds for c in cases}
            want = {c.name for c in CASES if keeps_family(BASES[bname], c) == keep}
            assert seen == want, (bname, keep)
            for cases, has_nan in rounds:
                assert all((c in NANS) == has_nan for c in cases)
                for po, _ in OUTLIERS:
                    bad, fix = node_tables(bname, cases, po)
                    inv = row_invalid(*bad[:, :7].T)
                    assert np.array_equal(np.flatnonzero(inv), [] if has_nan else NODE_BAD)
                    assert not row_invalid(*fix[:, :7].T).any()
                    fams = {family(r) for r in bad[:, :7]}
                    assert (len(fams) == 1) == keep, (bname, keep, fams)
                    assert {family(r) for r in fix[:, :7]} == fams
                    # no RT below a row's t + st / 2: NaN and -inf never share a node
                    assert np.abs(x).min() > np.nanmax(bad[:, 5] + np.abs(bad[:, 6]) / 2)
    # C
    for config, fam in MULTI_CONFIGS:
        classes = set()
        for with_nan in (False, True):
            x, args, multi = multi_fixture(config, fam, with_nan)
            bad = multi_bad(args)
            assert_layout(bad, f"multi {config} {fam}")
            assert 0.08 <= bad.mean() <= 0.2, (config, fam, bad.mean())
            missing = np.abs(x) == 999.0
            assert (missing & bad).sum() >= 4 and (missing & ~bad).sum() >= 4
            assert (x[bad] == 999.0).any() and (x[bad] == -999.0).any()
            nans = np.isnan(np.sum([np.broadcast_to(a, x.shape) for a in args], axis=0))
            n_nan = sum(len(i) for i in MULTI_NAN[config].values())
            assert nans.sum() == (n_nan if with_nan else 0)
            for po, w in OUTLIERS:
                tot, terms = oracle_lib.wiener_like_multi(x, *args, KN[0], multi=multi,
                                                          p_outlier=po, w_outlier=w, terms=True,
                                                          **MULTI_KN)
                classes.add(total_class(tot))
                rts = bad & ~missing & ~nans
                assert np.all(terms[rts] == (-math.inf if po == 0 else terms[rts][0]))
                if config != "vaz":  # (a z outside [0, 1] takes prob_ub outside [0, 1] too)
                    assert np.all(np.isfinite(terms[missing & ~nans]))
        assert classes == {"nan", "-inf", "finite"}, (config, fam, classes)
    # D
    rt, X, group = reg_fixture()
    pred = reg_pred(X)
    neg_a, neg_t = pred["a"] < 0, pred["t"] < 0
    assert 0.05 <= neg_a.mean() <= 0.15, neg_a.mean()
    assert 3 <= neg_t.sum() <= 20 and not (neg_a & neg_t).any()
    bad = neg_a | neg_t
    assert rt[1] == -999.0 and bad[1] and rt[0] == 999.0 and not bad[0]
    assert_layout(bad, "regression, input order")
    order = np.argsort(group, kind="stable")  # reg_layout_host
    in_group = group[order] == REG_BAD_GROUP
    assert np.flatnonzero(in_group)[[0, -1]].tolist() == [256, 511]
    assert_layout(bad[order] | in_group, "regression, grouped")


# --------------------------------------------------------------------------- GPU contexts

@pytest.fixture(scope="module")
def lean_ctx(gpu):
    """Resident calls always take the lean level-0 pass (chunks that refine go
    to the engine's redo pass)."""
    ctx = _ctx_env({"WFPT_LEAN_TREE": "1.0"})
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def node_ctxs(gpu):
    """The node path's variants: default, the t-node split level 0 and the
    breadth-first records."""
    from hddm_amd import _lib
    ctxs = {"default": _lib.context(), "split": _ctx_env({"WFPT_NODE_SPLIT": "1"}),
            "rounds": _ctx_env({"WFPT_NODE_SPEC": "0"})}
    yield ctxs
    for name in ("split", "rounds"):
        ctxs[name].close()


# --------------------------------------------------------------------------- A. resident calls

A_CONFIGS = {"simple": (SIMPLE, 1), "pinned": (PINNED, 1), "st_only": (ST_ONLY, 1),
             "sz_only": (SZ_ONLY, 1), "stress0": (STRESS[0], 1), "fixed": (PINNED, 0)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _plain(ctx, ds, row, kn):
    tot = ds.wiener_like(*row, *kn)
    part, zero = ctx.partials((len(ds) + 63) // 64)
    return tot, part, zero, path_names(ctx.last_path())


def assert_blocks(ctx, ds, ref, what):
    """assert_chunks (its bound, its zero counts) for the fixed-Simpson kernel,
    whose partials are per 256-trial block."""
    nb = (len(ds) + 255) // 256
    part, zero = ctx.partials(nb)
    r = ref[ds.order()]
    for c in range(nb):
        seg = r[256 * c:256 * c + 256]
        fin = seg[np.isfinite(seg)]
        assert int(zero[c]) == int(np.isneginf(seg).sum()), (what, c, zero[c])
        want, scale = math.fsum(fin), math.fsum(np.abs(fin))
        assert abs(part[c] - want) <= 1e-12 * scale + 1e-12, (what, c, part[c], want, scale)


def _host_entries(gpu, oracle_lib, x, row, kn, what):
    """gpu.wiener_like, pdf_array (logp 0 and 1) and full_pdf on the case's
    row: exactly 0 (the mixture's w p), -inf or NaN where the oracle has them."""
    err, n_st, n_sz, ua, se, po, w = kn
    want = oracle_lib.pdf_array(x, *row, err, 0, n_st, n_sz, ua, se, po, w)
    got = gpu.pdf_array(x, *row, err, 0, n_st, n_sz, ua, se, po, w)
    assert np.array_equal(got, want, equal_nan=True), what
    wlog = oracle_lib.pdf_array(x, *row, err, 1, n_st, n_sz, ua, se, po, w)
    assert_logp_parity(gpu.pdf_array(x, *row, err, 1, n_st, n_sz, ua, se, po, w), wlog, str(what))
    tot, wtot = gpu.wiener_like(x, *row, *kn), oracle_lib.wiener_like(x, *row, *kn)
    assert total_class(tot) == total_class(wtot), (what, tot, wtot)
    if math.isfinite(wtot):
        assert abs(tot - math.fsum(wlog)) <= 1e-11 * math.fsum(np.abs(wlog)), (what, tot)
    for xi in x[:2]:
        g = gpu.full_pdf(xi, *row, err, n_st, n_sz, ua, se)
        o = oracle_lib.full_pdf(xi, *row, err, n_st, n_sz, ua, se)
        assert g == o or (math.isnan(g) and math.isnan(o)), (what, xi, g, o)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [200, 1000])
@pytest.mark.parametrize("config", sorted(A_CONFIGS))
def test_resident_calls_around_invalid_rows(gpu, oracle_lib, lean_ctx, config, n):
    """Dataset.wiener_like on the default and the forced-lean context: valid,
    valid, invalid, valid, invalid, valid for every case. Each step is two
    plain calls (the first one runs on the other kind's prediction) and
    summing_vs_trials. Every valid step returns the first one's bits (total,
    chunk partials, zero counts, per-trial terms); the invalid steps follow
    the oracle: -inf with every term -inf, or fsum of log(w p) per chunk and
    in total, or NaN."""
    from hddm_amd import _lib
    base, ua = A_CONFIGS[config]
    fixed = ua == 0
    if config == "stress0":  # data that refines: drawn from the model itself
        np.random.seed(100)
        x = gpu.gen_rts_from_cdf(*base, samples=n, dt=1e-3)
    else:
        rng = np.random.default_rng(300 + n)
        x = rng.choice([-1.0, 1.0], n) * (0.42 + rng.gamma(2.0, 0.4, n))
    assert np.all(np.abs(x) >= base[5] - base[6] / 2)
    refs = {}
    for po, w in OUTLIERS:
        kn = knobs(po, w, ua)
        refs[po, "valid"] = ref_terms(oracle_lib, x, base, kn)
        for case in CASES:
            row = apply(base, case.set)
            refs[po, case.name] = ref_terms(oracle_lib, x, row, kn)
            if n == 200:
                _host_entries(gpu, oracle_lib, x, row, kn, (config, case.name, po))
    reached = {}
    for cname, ctx in (("default", _lib.context()), ("lean", lean_ctx)):
        seen = reached.setdefault(cname, {"valid": set(), "invalid": set(), "nan": set()})
        ds = gpu.Dataset(x, ctx=ctx)
        for po, w in OUTLIERS:
            kn = knobs(po, w, ua)
            first = {}

            def settle(row, check, what):
                """Plain calls, each checked, until three in a row launch the same
                kernels: the first runs on the other row's prediction, and a chunk
                that refines heavily is split only from the next engine call on."""
                seq = []
                while len(seq) < 3 or not seq[-1] == seq[-2] == seq[-3]:
                    assert len(seq) < 8, (what, "the call sequence does not settle", seq)
                    tot, part, zero, names = _plain(ctx, ds, row, kn)
                    check(tot, part, zero, (what, len(seq), sorted(names)))
                    seq.append(names)
                return seq

            def same_as_first(tot, part, zero, what):
                if not first:
                    return
                assert tot == first["tot"], (what, tot, first["tot"])
                assert np.array_equal(_bits(part), _bits(first["part"])), what
                # (the word's upper bits say which pass completed the chunk)
                assert np.array_equal(zero & 0xFFFF, first["zero"] & 0xFFFF), what

            def valid_step(what):
                seq = settle(base, same_as_first, what)
                seen["valid"].update(*seq)
                tot, terms, path = summing_vs_trials(ctx, ds, base, kn)
                part, zero = ctx.partials((n + 63) // 64)
                if not first:
                    first.update(tot=tot, part=part, zero=zero, terms=terms)
                    assert_terms(terms, refs[po, "valid"], f"{what} valid")
                    assert np.all(np.isfinite(terms)), what
                    (assert_blocks if fixed else assert_chunks)(ctx, ds, refs[po, "valid"],
                                                                f"{what} valid")
                same_as_first(tot, part, zero, (what, sorted(path_names(path))))
                assert np.array_equal(_bits(terms), _bits(first["terms"])), \
                    (what, path_names(path))

            def invalid_step(case, what):
                row, ref = apply(base, case.set), refs[po, case.name]
                key = "nan" if case in NANS else "invalid"
                seq = settle(row, lambda tot, part, zero, w: check_total(case, tot, w), what)
                seen[key].update(*seq)
                if (case.name in ("v=nan", "a=nan", "z=nan") and cname == "default"
                        and not fixed and any(family(row))):
                    # NaN values at level 0 make every chunk refine in-wave (a NaN t
                    # has no x - t > 0 and a == 0 an ambiguous term count: those go
                    # to the exact path instead). Once a call has seen that, the next
                    # one is predicted as an engine call, not a lean one
                    assert all("engine" in s and "lean" not in s for s in seq[1:]), (what, seq)
                tot, terms, path = summing_vs_trials(ctx, ds, row, kn)
                seen[key] |= path_names(path)
                check_total(case, tot, what)
                assert_logp_parity(terms, ref, str(what))
                if case in NANS:
                    assert np.all(np.isnan(terms)), what
                    return
                assert_terms(terms, ref, str(what))
                if po == 0:
                    assert np.all(np.isneginf(terms)), what
                (assert_blocks if fixed else assert_chunks)(ctx, ds, ref, str(what))
                # a settled invalid call of one block is the one-block kernel
                if n <= 256 and not fixed:
                    assert "small" in path_names(path), (what, path_names(path))

            def check_total(case, tot, what):
                if case in NANS:
                    assert math.isnan(tot), (what, tot)
                elif po == 0:
                    assert tot == -math.inf, (what, tot)
                else:  # assert_chunks' bound, over the whole call
                    ref = refs[po, case.name]
                    assert abs(tot - math.fsum(ref)) <= 1e-12 * math.fsum(np.abs(ref)) + 1e-12, \
                        (what, tot, math.fsum(ref))

            valid_step((config, n, cname, po, "first"))
            for case in CASES:
                for rep in range(2):
                    what = (config, n, cname, po, case.name, rep)
                    invalid_step(case, what)
                    valid_step(what)
        ds.close()
    print(f"resident {config} n={n}: " + "; ".join(
        f"{c} {k}: {sorted(v)}" for c, d in reached.items() for k, v in d.items()))
    if config == "stress0" and n == 1000:  # the refining sequences were part of it
        assert reached["default"]["valid"] & {"engine", "redo"}, reached
        assert "redo" in reached["lean"]["valid"], reached
    if fixed:
        assert reached["default"]["valid"] == {"fixed"}, reached


# --------------------------------------------------------------------------- B. node tables

NODE_KN = (KN[0], KN[1], KN[2], 1, KN[4])  # + w_outlier


def _assert_node_sums(sums, terms, ref, node, what):
    """test_node_terms_per_trial's bounds (the sums are the sums of the terms),
    with the reference's -inf / NaN classes."""
    for j in range(len(NODE_SIZES)):
        tj, rj = terms[node == j], ref[node == j]
        if np.isnan(rj).any():
            assert np.isnan(sums[j]), (what, j)
        elif np.isneginf(rj).any():
            assert sums[j] == -np.inf, (what, j)
        elif tj.size:
            assert abs(sums[j] - math.fsum(tj)) <= 1e-12 * math.fsum(np.abs(tj)) + 1e-12, (what, j)
        else:
            assert sums[j] == 0.0, (what, j)


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [True, False], ids=["keeps-family", "changes-family"])
@pytest.mark.parametrize("base_name", sorted(BASES))
def test_node_tables_with_invalid_rows(gpu, oracle_lib, node_ctxs, base_name, keep):
    """wiener_like_nodes with invalid (or NaN) rows among valid ones: a
    uniform-family table (the level-0 node kernels) when the rows keep the
    family, a mixed one (the generic node kernel) when they change it."""
    from hddm_amd import _lib
    x, node = node_dataset()
    m = len(NODE_SIZES)
    valid_trial = ~np.isin(node, NODE_BAD)
    valid_node = ~np.isin(np.arange(m), NODE_BAD)
    dss = {name: gpu.Dataset(x, node_id=node, n_nodes=m, ctx=ctx)
           for name, ctx in node_ctxs.items()}
    paths = set()
    for cases, has_nan in node_rounds(base_name, keep):
        for po, w in OUTLIERS:
            what = (base_name, keep, [c.name for c in cases], po)
            kn = NODE_KN + (w,)
            bad, fix = node_tables(base_name, cases, po)
            ref = node_terms_ref(oracle_lib, x, node, bad, kn)
            out = {}
            for name, ctx in node_ctxs.items():
                ds = dss[name]
                fsums, fterms = ds.wiener_like_nodes(fix, *kn, trials=True)
                rare_before = bool(ctx.last_path() & _lib.PATH_NODE_RARE)
                sums, terms = ds.wiener_like_nodes(bad, *kn, trials=True)
                path = ctx.last_path()
                paths.add((name, "split" if path & _lib.PATH_NODE_SPLIT else "level0",
                           "rare" if path & _lib.PATH_NODE_RARE else ""))
                split = keep and family(BASES[base_name])[1] and name == "split"
                assert bool(path & _lib.PATH_NODE_SPLIT) == split, (what, name)
                if po == 0 and not has_nan:
                    # an invalid row's zero is structural: nothing for the rare list,
                    # and the next call is not pending either
                    assert not rare_before and not path & _lib.PATH_NODE_RARE, (what, name)
                assert np.array_equal(ds.wiener_like_nodes(bad, *kn), sums, equal_nan=True), what
                if po == 0 and not has_nan:
                    assert not ctx.last_path() & _lib.PATH_NODE_RARE, (what, name)
                assert_logp_parity(terms, ref, f"{what} {name}")
                _assert_node_sums(sums, terms, ref, node, (what, name))
                # isolation: the valid nodes do not see their neighbours
                assert np.array_equal(_bits(terms[valid_trial]), _bits(fterms[valid_trial])), \
                    (what, name)
                assert np.array_equal(_bits(sums[valid_node]), _bits(fsums[valid_node])), \
                    (what, name)
                out[name] = (sums, terms, fsums, fterms)
            for name in ("split", "rounds"):
                for k in range(4):
                    assert np.array_equal(out["default"][k], out[name][k], equal_nan=True), \
                        (what, name, k)
            # multi-table: [valid, with the invalid rows, valid] in one launch
            msums, mterms = dss["default"].wiener_like_nodes_multi(np.stack([fix, bad, fix]), *kn,
                                                                   trials=True)
            sums, terms, fsums, fterms = out["default"]
            for t, (s1, t1) in enumerate(((fsums, fterms), (sums, terms), (fsums, fterms))):
                assert np.array_equal(msums[t], s1, equal_nan=True), (what, "multi sums", t)
                assert np.array_equal(mterms[t], t1, equal_nan=True), (what, "multi terms", t)
    for ds in dss.values():
        ds.close()
    print(f"nodes {base_name} keep={keep}: {sorted(paths)}")


# --------------------------------------------------------------------------- C. per trial

@pytest.mark.gpu
@pytest.mark.parametrize("config,fam", MULTI_CONFIGS)
def test_multi_with_invalid_trials(gpu, oracle_lib, config, fam):
    """wiener_like_multi_terms (multi_fast_kernel for the uniform families,
    multi_kernel when sz / st / t are per trial) with invalid and NaN
    per-trial values and +-999 trials on invalid rows."""
    for with_nan in (False, True):
        x, args, multi = multi_fixture(config, fam, with_nan)
        ds = gpu.Dataset(x, input_order=True)
        for po, w in OUTLIERS:
            what = f"multi {config} {fam} nan={with_nan} po={po}"
            kn = dict(MULTI_KN, p_outlier=po, w_outlier=w)
            ref_tot, ref = oracle_lib.wiener_like_multi(x, *args, KN[0], multi=multi, terms=True,
                                                        **kn)
            tot, terms = gpu.wiener_like_multi_terms(x, *args, KN[0], multi, **kn)
            assert_logp_parity(terms, ref, what)
            assert total_class(tot) == total_class(ref_tot), (what, tot, ref_tot)
            if math.isfinite(ref_tot):
                assert abs(tot - ref_tot) <= 1e-10 * abs(ref_tot), (what, tot, ref_tot)
            tot2, terms2 = ds.wiener_like_multi(*args, KN[0], multi, trials=True, **kn)
            assert _bits(tot2) == _bits(tot) and np.array_equal(_bits(terms2), _bits(terms)), what
            assert _bits(gpu.wiener_like_multi(x, *args, KN[0], multi, **kn)) == _bits(tot), what
        ds.close()


# --------------------------------------------------------------------------- D. regression

def _reg_family(fam, po, w):
    return dict(REG_FAMILIES[fam], p_outlier=po, w_outlier=w)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["simple", "full", "fixed"])
def test_reg_identity_link_predicts_invalid_trials(gpu, oracle_lib, fam):
    """wiener_like_reg with a and t through the identity link: single trials
    of a valid wave get a < 0 or t < 0. The predictions bit for bit, the terms
    against the oracle at the device's predictions."""
    rt, X, _ = reg_fixture()
    want_pred = reg_pred(X)
    ds = gpu.RegDataset(rt, X)
    for po, w in OUTLIERS:
        what = f"reg {fam} po={po}"
        F = _reg_family(fam, po, w)
        total, terms, pred = ds.wiener_like_reg(REG_MODEL, REG_COEF, *reg_args(F), **reg_kw(F),
                                                terms=True)
        for name in ("v", "a", "t"):
            assert np.array_equal(_bits(pred[name]), _bits(want_pred[name])), (what, name)
        ref_tot, want = oracle_multi(oracle_lib, rt, pred, F, ["v", "a", "t"])
        assert_logp_parity(terms, want, what)
        bad = (pred["a"] < 0) | (pred["t"] < 0)
        scored = np.abs(rt) != 999.0
        assert np.all(terms[bad & scored] == (-np.inf if po == 0 else terms[255])), what
        assert np.all(np.isfinite(terms[~scored])), what  # +-999: not gated by validity
        assert total_class(total) == total_class(ref_tot), (what, total, ref_tot)
        if math.isfinite(ref_tot):
            assert abs(total - ref_tot) <= 1e-10 * abs(ref_tot), (what, total, ref_tot)
        assert _bits(ds.wiener_like_reg(REG_MODEL, REG_COEF, *reg_args(F), **reg_kw(F))) == \
            _bits(total), what
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["simple", "full", "fixed"])
def test_reg_groups_with_an_invalid_group_row(gpu, oracle_lib, fam):
    """wiener_like_reg_groups: the non-regressed row of one group is invalid
    (z = 1.1). That group's sum follows the oracle; every other group has the
    bits of the call with a valid row there."""
    rt, X, group = reg_fixture()
    G = 5
    table = REG_COEF[None, :] * (1.0 + 0.02 * np.arange(G))[:, None]
    ds = gpu.RegDataset(rt, X, group_id=group, n_groups=G)
    sel_bad = group == REG_BAD_GROUP
    for po, w in OUTLIERS:
        what = f"reg groups {fam} po={po}"
        F = _reg_family(fam, po, w)
        kw = {k: F[k] for k in ("err", "n_st", "n_sz", "use_adaptive", "simps_err", "w_outlier")}
        fix = np.tile([0.0, F["sv"], 0.0, F["z"], F["sz"], 0.0, F["st"], po], (G, 1))
        fix[:, 3] = F["z"] - 0.01 * np.arange(G)
        bad = fix.copy()
        bad[REG_BAD_GROUP, 3] = 1.1
        fsums, fterms, _ = ds.wiener_like_reg_groups(REG_MODEL, table, fix, **kw, terms=True)
        sums, terms, pred = ds.wiener_like_reg_groups(REG_MODEL, table, bad, **kw, terms=True)
        assert np.array_equal(ds.wiener_like_reg_groups(REG_MODEL, table, bad, **kw), sums,
                              equal_nan=True), what
        for g in range(G):
            sel = group == g
            for name, c0, nc, link in REG_MODEL:
                want_pred = restate_pred(X[sel], table[g], c0, nc, link)
                assert np.array_equal(_bits(pred[name][sel]), _bits(want_pred)), (what, g)
            Fg = dict(F, z=bad[g, 3])
            ref_tot, want = oracle_multi(oracle_lib, rt[sel], {k: v[sel] for k, v in pred.items()},
                                         Fg, ["v", "a", "t"])
            assert_logp_parity(terms[sel], want, f"{what} group {g}")
            assert total_class(sums[g]) == total_class(ref_tot), (what, g, sums[g], ref_tot)
            if math.isfinite(ref_tot):  # test_reg's bar against fsum
                assert abs(sums[g] - math.fsum(want)) < 1e-9 * abs(math.fsum(want)), (what, g)
        scored = np.abs(rt) != 999.0
        if po == 0:
            assert np.all(np.isneginf(terms[sel_bad & scored])) and sums[REG_BAD_GROUP] == -np.inf
        assert np.array_equal(_bits(terms[~sel_bad]), _bits(fterms[~sel_bad])), what
        others = np.arange(G) != REG_BAD_GROUP
        assert np.array_equal(_bits(sums[others]), _bits(fsums[others])), what
    ds.close()


# --------------------------------------------------------------------------- E. RL

@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["simple", "full", "fixed"])
def test_rlddm_with_an_invalid_row(gpu, oracle_lib, fam):
    """RLDataset.wiener_like_rlddm with a = -0.1: the unscored first trial of
    each condition stays 0.0, every scored term follows the oracle."""
    x, response, feedback, split_by = make_data(11, [1, 2, 63, 64, 130], labels=[20, 3, 12, 7, 11])
    ds = gpu.RLDataset(x, response, feedback, split_by)
    for po, w in OUTLIERS:
        F = dict(RL_FAMILIES[fam], a=-0.1, p_outlier=po, w_outlier=w)
        drift, scored = restate_rlddm(response, feedback, split_by, *ROW_A, F["v"])
        want = oracle_terms(oracle_lib, x[scored], drift[scored], F)
        total, terms, got_drift = ds.wiener_like_rlddm(*rlddm_args(ROW_A, F), **rlddm_kw(F),
                                                       terms=True)
        assert np.array_equal(got_drift, drift)
        assert scored.sum() == x.size - 5 and np.all(terms[~scored] == 0.0)
        assert_logp_parity(terms[scored], want, f"rlddm {fam} po={po}")
        if po == 0:
            assert np.all(np.isneginf(terms[scored])) and total == -np.inf
        else:
            assert np.all(terms[scored] == terms[scored][0])
            assert abs(total - math.fsum(want)) < 1e-9 * abs(math.fsum(want)), (fam, total)
        assert _bits(ds.wiener_like_rlddm(*rlddm_args(ROW_A, F), **rlddm_kw(F))) == _bits(total)
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bad_node", [0, 1, 2])
def test_rlddm_nodes_with_an_invalid_node_row(gpu, oracle_lib, bad_node):
    """wiener_like_rlddm_nodes with one invalid row of three: the other two
    nodes keep the bits of the all-valid call; the invalid node follows the
    oracle."""
    (x, response, feedback, split_by), node = _node_data()
    rows = np.array([ROW_A, ROW_B, ROW_C])
    ds = gpu.RLDataset(x, response, feedback, split_by, node_id=node, n_nodes=3)
    for po, w in OUTLIERS:
        fix = np.array([[2.4, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, po],
                        [-1.6, 0.2, 1.7, 0.45, 0.1, 0.28, 0.1, po],
                        [3.0, 0.0, 2.2, 0.55, 0.1, 0.32, 0.1, po]])
        bad = fix.copy()
        bad[bad_node, 2] = -0.1
        K = dict(err=KN[0], n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, w_outlier=w)
        fsums, fterms, _ = ds.wiener_like_rlddm_nodes(rows, fix, **K, terms=True)
        sums, terms, drift = ds.wiener_like_rlddm_nodes(rows, bad, **K, terms=True)
        assert np.array_equal(ds.wiener_like_rlddm_nodes(rows, bad, **K), sums, equal_nan=True)
        for j in range(3):
            sel = node == j
            if j != bad_node:
                assert _bits(sums[j]) == _bits(fsums[j]), (bad_node, po, j)
                assert np.array_equal(_bits(terms[sel]), _bits(fterms[sel])), (bad_node, po, j)
                continue
            F = dict(zip(("v",) + NAMES[1:] + ("p_outlier",), bad[j]), **K)
            want_drift, scored = restate_rlddm(response[sel], feedback[sel], split_by[sel],
                                               *rows[j], F["v"])
            assert np.array_equal(drift[sel], want_drift)
            want = oracle_terms(oracle_lib, x[sel][scored], want_drift[scored], F)
            assert_logp_parity(terms[sel][scored], want, f"rl node {j} po={po}")
            assert np.all(terms[sel][~scored] == 0.0)
            if po == 0:
                assert np.all(np.isneginf(want)) and sums[j] == -np.inf
            else:
                assert abs(sums[j] - math.fsum(want)) < 1e-9 * abs(math.fsum(want)), (j, sums[j])
    ds.close()
