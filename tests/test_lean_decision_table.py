"""The lean pass's table stage (lean_kernel<kAdaptTZ>: a wave looks up the tt
of its two extreme |rt| among the series decision's breakpoints instead of
estimating every lane's decision) against the per-lane code.

Every dataset takes tests/test_lean_uniform.py's three checks as they stand
(its helpers are imported): terms and total bit-equal to the engine context's
per-lane level 0; terms and chunk partials within the project's bars of the
oracle; the summing call equal to the trials call. The counting build tallies
the waves the table settled (wfpt_profile_lists counts[0], "lean_table") next
to the generic-site waves (counts[3], "lean_generic").

The lean context here also sets WFPT_SMALL=0: the datasets have 64 to 1,280
trials, and a call of at most 256 would otherwise take the one-block kernel,
not lean_kernel.

The breakpoints are bisected below from the reference's formula
(test_lean_uniform.decisions); at err = 1e-4 they are tt = 0.0552731,
0.153704, 0.216098, 0.449156, 1.54613. The table's guard band is 1e-6
relative (wfpt_lean_tables.hpp: kDecBand).
"""
import math

import numpy as np
import pytest

from test_lean_uniform import (KN, PINNED, _open_ctx, assert_chunks, assert_terms, decisions,
                               eng_ctx, node_decisions, ref_terms, summing_vs_trials)  # noqa: F401

SV0 = (0.5, 0.0, 2.0, 0.5, 0.1, 0.3, 0.1)
BAND = 1e-6
ENV = {"WFPT_LEAN_TREE": "1.0", "WFPT_SMALL": "0"}


def breakpoints(err, lo=1e-6, hi=1e3):
    """tt at which (small, K) of the reference's formula changes on [lo, hi]."""
    tt = np.exp(np.linspace(math.log(lo), math.log(hi), 200001))
    s, k = decisions(tt, err)
    code = s * 100 + k
    out = []
    for i in np.flatnonzero(code[1:] != code[:-1]):
        a, b, ca = tt[i], tt[i + 1], code[i]
        for _ in range(80):
            m = 0.5 * (a + b)
            sm, km = decisions(np.array([m]), err)
            if sm[0] * 100 + km[0] == ca:
                a = m
            else:
                b = m
        out.append(b)
    return out


BP = breakpoints(KN[0])
assert len(BP) == 5 and abs(BP[1] - 0.153704) < 1e-6 and abs(BP[4] - 1.54613) < 1e-5, BP


def t_nodes(args):
    t, st = args[5], args[6]
    lb, ub = t - st / 2.0, t + st / 2.0
    c = (ub + lb) / 2.0
    return np.array([lb, (lb + c) / 2.0, c, (c + ub) / 2.0, ub])


def with_sides(mag, sides, n_lower):
    """upper / lower / mixed: n_lower of the trials (spread over the whole range) lower."""
    if sides == "upper":
        return mag
    if sides == "lower":
        return -mag
    lower = np.zeros(mag.size, dtype=bool)
    lower[np.round(np.linspace(0, mag.size - 1, n_lower)).astype(int)] = True
    return np.where(lower, -mag, mag)


@pytest.fixture(scope="module")
def lean_ctx(gpu):
    ctx = _open_ctx(ENV)
    yield ctx
    ctx.close()


def run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, args, what, kn=KN, **ds_kw):
    """test_lean_uniform.run_case with both tallies: (table, generic, waves).
    ds_kw: Dataset keywords of both contexts' datasets (input_order)."""
    from hddm_amd import _lib
    ref = ref_terms(oracle_lib, x, args, kn)
    de = gpu.Dataset(x, ctx=eng_ctx, **ds_kw)
    tot_e, terms_e = de.wiener_like_trials(*args, *kn)
    assert eng_ctx.last_path() & _lib.PATH_ENGINE, (what, eng_ctx.last_path())
    assert not eng_ctx.last_path() & _lib.PATH_LEAN, (what, eng_ctx.last_path())
    de.close()
    ds = gpu.Dataset(x, ctx=lean_ctx, **ds_kw)
    ds.wiener_like(*args, *kn)
    tot, terms, path = summing_vs_trials(lean_ctx, ds, args, kn)  # check 3
    assert path & _lib.PATH_LEAN and not path & _lib.PATH_SMALL, (what, path)
    # check 1: bit for bit the engine's per-lane level 0
    assert np.array_equal(np.asarray(terms).view(np.int64), np.asarray(terms_e).view(np.int64)), (
        what, np.flatnonzero(np.asarray(terms) != np.asarray(terms_e))[:10])
    assert tot == tot_e or (math.isnan(tot) and math.isnan(tot_e)), (what, tot, tot_e)
    # check 2: the oracle
    assert_terms(terms, ref, what)
    assert_chunks(lean_ctx, ds, ref, what)
    lean_ctx.profile(lean_ctx.PROF_EVALS)
    try:
        lean_ctx.profile_lists(reset=True)
        tot_c = ds.wiener_like(*args, *kn)
        assert lean_ctx.last_path() & _lib.PATH_LEAN, (what, lean_ctx.last_path())
        counts = lean_ctx.profile_lists(reset=True)
    finally:
        lean_ctx.profile(0)
    assert tot_c == tot or (math.isnan(tot) and math.isnan(tot_c)), (what, tot, tot_c)
    ds.close()
    waves = (len(x) + 63) // 64
    table, generic = counts["lean_table"], counts["lean_generic"]
    print(f"{what}: n={len(x)} table {table} generic {generic} of {waves} waves")
    assert table + generic <= waves, (what, table, generic, waves)
    return table, generic, waves


@pytest.mark.gpu
@pytest.mark.parametrize("sides", ["upper", "lower", "mixed"])
@pytest.mark.parametrize("args", [PINNED, SV0], ids=["pinned", "sv0"])
@pytest.mark.parametrize("k", range(5))
def test_breakpoint_ramps(gpu, oracle_lib, lean_ctx, eng_ctx, k, args, sides):
    """For each t node j, an even ramp of 256 |rt| that carries node j's tt
    across breakpoint k: from 0.32 to 0.48 of the t nodes' spacing around it,
    so no other node meets the breakpoint and it falls inside a wave, not
    between two. The wave that holds it (of either boundary) takes the per-lane
    pre-pass and the generic site; the waves away from it are settled by the
    table."""
    a, tcs = args[2], t_nodes(args)
    step = tcs[1] - tcs[0]
    for j in range(5):
        mag = tcs[j] + (a * a) * BP[k] + step * np.linspace(-0.32, 0.48, 256)
        small, K = node_decisions(mag, args, KN[0])
        code = small[:, j] * 100 + K[:, j]
        assert code[0] != code[-1], (k, j, code[0], code[-1])
        x = with_sides(mag, sides, 100)  # 100 = 64 + 36: the boundary switch is mid-wave
        table, generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, args,
                                         f"ramp bp{k} node{j} {sides}")
        assert 0 < table < waves, (k, j, table, generic, waves)
        assert generic >= 1, (k, j, table, generic, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("sides", ["upper", "lower", "mixed"])
@pytest.mark.parametrize("args", [PINNED, SV0], ids=["pinned", "sv0"])
@pytest.mark.parametrize("rng_x", [(0.60, 0.80), (1.145, 1.16), (0.895, 0.91)],
                         ids=["one_piece", "two_K", "two_series"])
def test_one_wave_inside_pieces(gpu, oracle_lib, lean_ctx, eng_ctx, rng_x, args, sides):
    """One 64-trial wave every node of which stays inside one piece: all five
    in small-time K = 4; nodes 0, 1 in large-time K = 3 and nodes 2..4 in K = 4;
    nodes 0, 1 large-time and nodes 2..4 small-time (K = 4). The table settles
    it whether or not the nodes share a decision. (mixed: one such wave per
    boundary, 128 trials.)"""
    rng = np.random.default_rng(31)
    mag = rng.uniform(*rng_x, 128 if sides == "mixed" else 64)
    small, K = node_decisions(mag, args, KN[0])
    code = small * 100 + K
    assert (code == code[0]).all(), np.unique(code, axis=0)
    pieces = len(set(code[0].tolist()))
    assert pieces == (1 if rng_x[0] == 0.60 else 2), code[0]
    x = with_sides(mag, sides, 64)
    table, generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, args,
                                     f"one wave {rng_x} {sides}")
    assert (table, generic) == (waves, 0) and waves == len(x) // 64, (table, generic, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("sides", ["upper", "lower", "mixed"])
@pytest.mark.parametrize("args", [PINNED, SV0], ids=["pinned", "sv0"])
@pytest.mark.parametrize("k,j", [(0, 4), (1, 2), (2, 0), (3, 3), (4, 1)])
def test_inside_the_guard_band(gpu, oracle_lib, lean_ctx, eng_ctx, k, j, args, sides):
    """A wave whose tt at node j lies inside breakpoint k's guard band,
    x = tc_j + a^2 tt_bp (1 +- BAND / 4): the table does not answer."""
    rng = np.random.default_rng(100 * k + j)
    a, tcs = args[2], t_nodes(args)
    mag = tcs[j] + (a * a) * BP[k] * (1.0 + (BAND / 4) * rng.uniform(-1.0, 1.0, 64))
    x = with_sides(mag, sides, 24)
    table, generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, args,
                                     f"band bp{k} node{j} {sides}")
    assert table == 0, (table, generic, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_shortest_second_wave(gpu, oracle_lib, lean_ctx, eng_ctx, sign):
    """n = 65: one full wave and a wave of one trial. Both are inside one
    piece: the one-trial wave's first and last own lane are the same lane."""
    rng = np.random.default_rng(65)
    x = sign * rng.uniform(0.60, 0.80, 65)
    table, generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, PINNED, f"n65 {sign}")
    assert (table, generic, waves) == (2, 0, 2), (table, generic, waves)


def unordered_waves(args, k, j, n_waves, rng):
    """Waves of 64 |rt| in the caller's order whose tt at node j straddles
    breakpoint k (within +-0.3 of the t nodes' spacing, so no other node meets
    a breakpoint), shuffled, with the first and the last lane both below the
    breakpoint: a lookup of those two lanes alone would find one piece at
    every node."""
    a, tcs = args[2], t_nodes(args)
    step = tcs[1] - tcs[0]
    x_bp = tcs[j] + (a * a) * BP[k]
    out = []
    for _ in range(n_waves):
        w = x_bp + step * rng.uniform(-0.3, 0.3, 64)
        w[:8] = x_bp + step * rng.uniform(0.05, 0.3, 8)   # some above it for certain
        w[8:16] = x_bp - step * rng.uniform(0.05, 0.3, 8)  # and some below
        rng.shuffle(w)
        below = np.flatnonzero(w < x_bp - 0.01 * step)
        for lane, src in ((0, below[0]), (63, below[-1])):
            w[[lane, src]] = w[[src, lane]]
        assert w[0] < x_bp and w[63] < x_bp and w[1:63].max() > x_bp + 0.01 * step
        out.append(w)
    return np.concatenate(out)


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["upper", "lower"])
@pytest.mark.parametrize("args", [PINNED, SV0], ids=["pinned", "sv0"])
@pytest.mark.parametrize("k,j", [(1, 2), (0, 4), (2, 0)])
def test_unordered_waves_are_not_settled(gpu, oracle_lib, lean_ctx, eng_ctx, k, j, args, sign):
    """input_order=True keeps the caller's order, so the lean pass meets waves
    whose |rt| is not nondecreasing. Four such one-boundary waves straddle a
    breakpoint (k = 1: the small-time / large-time switch) while their first
    and last lanes lie in one piece: only the kernel's order check keeps the
    table from answering for them. The table settles none, the lanes disagree
    so every wave is generic, and the bits are the engine's."""
    rng = np.random.default_rng(400 + 10 * k + j)
    mag = unordered_waves(args, k, j, 4, rng)
    small, K = node_decisions(mag, args, KN[0])
    code = (small * 100 + K).reshape(4, 64, 5)
    for w in range(4):
        assert (code[w, 0] == code[w, 63]).all(), (w, code[w, 0], code[w, 63])
        assert (code[w, :, j] != code[w, 0, j]).any(), w
    table, generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, sign * mag, args,
                                     f"unordered bp{k} node{j} {sign}", input_order=True)
    assert (table, generic, waves) == (0, 4, 4), (table, generic, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["upper", "lower"])
def test_input_order_sorted_and_descending(gpu, oracle_lib, lean_ctx, eng_ctx, sign):
    """An input_order dataset inside one piece at every node (|rt| in [0.60,
    0.80]): two waves given in nondecreasing order (the second with ties) are
    settled by the table; two given in descending order fail the order check,
    so the table settles neither, and the per-lane vote still finds them
    uniform (no generic wave)."""
    rng = np.random.default_rng(64)
    w0 = np.sort(rng.uniform(0.60, 0.80, 64))
    w1 = np.sort(np.repeat(rng.uniform(0.60, 0.80, 32), 2))
    w2 = np.sort(rng.uniform(0.60, 0.80, 64))[::-1]
    w3 = np.sort(rng.uniform(0.60, 0.80, 64))[::-1]
    mag = np.concatenate([w0, w2, w1, w3])
    small, K = node_decisions(mag, PINNED, KN[0])
    assert small.all() and (K == 4).all()
    table, generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, sign * mag, PINNED,
                                     f"input order {sign}", input_order=True)
    assert (table, generic, waves) == (2, 0, 4), (table, generic, waves)


@pytest.mark.gpu
def test_err_changes_between_calls(gpu, lean_ctx):
    """err = 1e-4, 1e-10, 1e-4 on one context: every call gives the bits of a
    fresh context's first call at that err (the table is keyed by err), and the
    tallies of the two errs differ as their breakpoints do."""
    rng = np.random.default_rng(17)
    n = 1024 + 37
    x = rng.choice([-1.0, 1.0], n) * (0.36 + rng.gamma(2.0, 0.35, n))
    ds = gpu.Dataset(x, ctx=lean_ctx)
    seen = {}
    for err in (1e-4, 1e-10, 1e-4):
        kn = (err,) + KN[1:]
        tot, terms = ds.wiener_like_trials(*PINNED, *kn)
        lean_ctx.profile(lean_ctx.PROF_EVALS)
        try:
            lean_ctx.profile_lists(reset=True)
            tot_c = ds.wiener_like(*PINNED, *kn)
            table = lean_ctx.profile_lists(reset=True)["lean_table"]
        finally:
            lean_ctx.profile(0)
        assert tot_c == tot, (err, tot, tot_c)
        fresh = _open_ctx(ENV)
        try:
            df = gpu.Dataset(x, ctx=fresh)
            df.wiener_like(*PINNED, *kn)  # the first call takes the engine; then the lean pass
            tot_f, terms_f = df.wiener_like_trials(*PINNED, *kn)
            fresh.profile(fresh.PROF_EVALS)
            fresh.profile_lists(reset=True)
            df.wiener_like(*PINNED, *kn)
            table_f = fresh.profile_lists(reset=True)["lean_table"]
            df.close()
        finally:
            fresh.close()
        assert tot == tot_f, (err, tot, tot_f)
        assert np.array_equal(np.asarray(terms).view(np.int64), np.asarray(terms_f).view(np.int64))
        assert table == table_f and table > 0, (err, table, table_f)
        if err in seen:
            assert seen[err] == (tot, table), (err, seen[err], tot, table)
        seen[err] = (tot, table)
    ds.close()


@pytest.mark.gpu
def test_err_beyond_the_estimate(gpu, oracle_lib, lean_ctx, eng_ctx):
    """err = 1e-80 is outside the fp32 estimate's range, where the uniform
    site never ran: the context hands the kernel a table that does not answer,
    so no wave is settled by it and every wave is generic, as
    tests/test_lean_uniform.py's test_term_count_limits expects."""
    rng = np.random.default_rng(13)
    n = 1024 + 37
    x = rng.choice([-1.0, 1.0], n) * (0.36 + rng.gamma(2.0, 0.35, n))
    kn = (1e-80,) + KN[1:]
    table, generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, PINNED, "err 1e-80", kn)
    assert table == 0 and generic == waves, (table, generic, waves)
