"""The uniform site of the lean pass (lean_uniform_level0: its exponentials
evaluated level by level across the six / three chains of a node, exp_val_n,
and its clean test from one running minimum and one finiteness test) against
the generic site (eng_level0_t), whose bits are the contract.

1. Bit equality between the two sites of lean_kernel<kAdaptTZ>. A default
   (sorted) dataset of one boundary runs the uniform site; an input_order
   dataset that alternates the same |rt| between the two boundaries has both
   boundaries in every 64-trial chunk, so every wave runs the generic site.
   The per-trial terms of the first are bit-equal to the terms of the same
   signed RTs in the second. The counting build confirms which site ran.
   A total depends on which trials share a chunk, so the two datasets' totals
   are sums of different partials; the sorted dataset's total is compared
   with the total of the same dataset on a default context's first call,
   which takes the engine (the per-lane level 0 in the same chunks), as
   tests/test_lean_uniform.py does.
   The |rt| come from six ranges, one per series code the benchmark data meet
   at err = 1e-4 (small-time K = 3, 4; large-time K = 4, 3, 2, 1), each chosen
   so that all five t nodes of every trial have that code (asserted from the
   reference's formulas). n = 384: one wave per code. n = 128: two codes,
   three pairs. n = 65: a wave of one code and a one-trial wave of the next.
2. The |v| = 12 situation of tests/test_lean_uniform.py (drift exponents that
   fail the per-trial range test, so the per-node guards decide): terms and
   total bit-equal to the engine context's.
3. The counting call on 4,096 sorted trials of the benchmark's model: every
   wave is tallied as settled by the table (uniform site ran to its end) or
   as generic, and the generic tally is the parent build's.
"""
import math

import numpy as np
import pytest

from test_lean_uniform import KN, PINNED, _open_ctx, node_decisions

SV0 = (0.5, 0.0, 2.0, 0.5, 0.1, 0.3, 0.1)
ENV = {"WFPT_LEAN_TREE": "1.0", "WFPT_SMALL": "0"}
# |rt| ranges inside which all five t nodes (0.25 .. 0.35, a = 2) have one code
REGIONS = [((0.40, 0.46), (True, 3)), ((0.60, 0.80), (True, 4)), ((0.98, 1.10), (False, 4)),
           ((1.30, 1.90), (False, 3)), ((2.30, 6.00), (False, 2)), ((6.70, 8.00), (False, 1))]
# the generic-site waves of test_benchmark_model_tallies' dataset on the parent
# build (the commit before the uniform site's stream was shortened)
PARENT_GENERIC_4096 = 24


@pytest.fixture(scope="module")
def lean_ctx(gpu):
    ctx = _open_ctx(ENV)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def eng_ctx(gpu):
    ctx = _open_ctx({})
    yield ctx
    ctx.close()


def region_rts(r, n, rng):
    lo, hi = REGIONS[r][0]
    return rng.uniform(lo, hi, n)


def tallies(ctx, ds, args, kn=KN):
    from hddm_amd import _lib
    ctx.profile(ctx.PROF_EVALS)
    try:
        ctx.profile_lists(reset=True)
        tot = ds.wiener_like(*args, *kn)
        assert ctx.last_path() & _lib.PATH_LEAN, ctx.last_path()
        counts = ctx.profile_lists(reset=True)
    finally:
        ctx.profile(0)
    return tot, counts["lean_table"], counts["lean_generic"]


def lean_trials(gpu, ctx, x, args, **kw):
    """(total, terms, table, generic) of a dataset's lean-pass calls."""
    from hddm_amd import _lib
    ds = gpu.Dataset(x, ctx=ctx, **kw)
    ds.wiener_like(*args, *KN)  # a dataset's first call; the next ones take the lean pass
    tot, terms = ds.wiener_like_trials(*args, *KN)
    path = ctx.last_path()
    assert path & _lib.PATH_LEAN and not path & _lib.PATH_SMALL, path
    tot_c, table, generic = tallies(ctx, ds, args)
    assert tot_c == tot, (tot, tot_c)
    ds.close()
    return tot, np.asarray(terms), table, generic


def engine_trials(gpu, ctx, x, args):
    from hddm_amd import _lib
    ds = gpu.Dataset(x, ctx=ctx)
    tot, terms = ds.wiener_like_trials(*args, *KN)
    path = ctx.last_path()
    assert path & _lib.PATH_ENGINE and not path & _lib.PATH_LEAN, path
    ds.close()
    return tot, np.asarray(terms)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def datasets():
    """(name, |rt|, codes): the shapes of check 1."""
    rng = np.random.default_rng(9)
    out = [("n384", np.concatenate([region_rts(r, 64, rng) for r in range(6)]), list(range(6)))]
    for r in (0, 2, 4):
        out.append((f"n128 codes {r},{r + 1}",
                    np.concatenate([region_rts(r, 64, rng), region_rts(r + 1, 64, rng)]), [r, r + 1]))
    for r in range(6):
        q = min(r + 1, 5)  # a larger |rt|: the lone trial sorts last, into the second wave
        lone = region_rts(q, 1, rng) if q != r else np.array([REGIONS[r][0][1]])
        out.append((f"n65 code {r} + one of {q}", np.concatenate([region_rts(r, 64, rng), lone]),
                    [r, q]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["upper", "lower"])
@pytest.mark.parametrize("args", [PINNED, SV0], ids=["sv0.1", "sv0"])
def test_uniform_site_equals_generic_site(gpu, lean_ctx, eng_ctx, args, sign):
    seen = set()
    for name, mag, codes in datasets():
        what = (name, args[1], sign)
        small, K = node_decisions(mag, args, KN[0])
        for r in codes:
            (lo, hi), (s_r, k_r) = REGIONS[r]
            sel = (mag >= lo) & (mag <= hi)
            assert sel.any() and (small[sel] == s_r).all() and (K[sel] == k_r).all(), (what, r)
            seen.add(r)
        n = mag.size
        waves = (n + 63) // 64
        # the uniform site: one boundary, the dataset's own (sorted) order
        tot_u, terms_u, table_u, generic_u = lean_trials(gpu, lean_ctx, sign * mag, args)
        print(f"{what}: table {table_u} generic {generic_u} of {waves} waves")
        assert (table_u, generic_u) == (waves, 0), (what, table_u, generic_u, waves)
        # the generic site: the same |rt| alternating between the boundaries, order kept
        mixed = np.empty(2 * n)
        mixed[0::2] = mag
        mixed[1::2] = -mag
        _, terms_g, table_g, generic_g = lean_trials(gpu, lean_ctx, mixed, args, input_order=True)
        assert (table_g, generic_g) == (0, (2 * n + 63) // 64), (what, table_g, generic_g)
        same = terms_g[0::2] if sign > 0 else terms_g[1::2]
        assert np.all(np.isfinite(terms_u)), what
        assert np.array_equal(bits(terms_u), bits(same)), (
            what, np.flatnonzero(bits(terms_u) != bits(same))[:10])
        # the total: the same chunks through the engine's per-lane level 0
        tot_e, terms_e = engine_trials(gpu, eng_ctx, sign * mag, args)
        assert np.array_equal(bits(terms_u), bits(terms_e)), what
        assert bits([tot_u])[0] == bits([tot_e])[0], (what, tot_u, tot_e)
    assert seen == set(range(6))


@pytest.mark.gpu
def test_range_test_failures_match_the_generic_site(gpu, lean_ctx, eng_ctx):
    """|v| = 12 (tests/test_lean_uniform.py: test_guard_fallback, k = 3): most
    waves fail the per-trial range test or leave the uniform site, and the
    bits are the per-lane code's."""
    args = (12.0, 0.5, 1.0, 0.5, 0.1, 0.3, 0.1)
    rng = np.random.default_rng(2003)
    n = 2048
    x = rng.choice([-1.0, 1.0], n) * (0.32 + rng.gamma(2.0, 0.4, n))
    x = np.where(np.abs(x) < args[5] + args[6] / 2 + 0.01, np.sign(x) * 0.5, x)
    tot, terms, table, generic = lean_trials(gpu, lean_ctx, x, args)
    tot_e, terms_e = engine_trials(gpu, eng_ctx, x, args)
    waves = n // 64
    print(f"|v|=12: table {table} generic {generic} of {waves}")
    assert generic > waves // 2, (table, generic, waves)
    assert np.isfinite(terms).mean() >= 0.9
    assert np.array_equal(bits(terms), bits(terms_e)), np.flatnonzero(bits(terms) != bits(terms_e))[:10]
    assert bits([tot])[0] == bits([tot_e])[0], (tot, tot_e)


@pytest.mark.gpu
def test_benchmark_model_tallies(gpu, lean_ctx):
    """4,096 trials drawn from the benchmark's model (bench.py: PARAMS, KNOBS,
    p_outlier 0.05), in the dataset's sorted order: 64 waves, each tallied
    once, and as many generic ones as the parent build counts."""
    np.random.seed(20261015)
    x = gpu.gen_rts_from_cdf(*PINNED, samples=4096, dt=1e-3)
    assert x.size == 4096
    ds = gpu.Dataset(x, ctx=lean_ctx)
    ds.wiener_like(*PINNED, *KN)
    tot = ds.wiener_like(*PINNED, *KN)
    tot_c, table, generic = tallies(lean_ctx, ds, PINNED)
    ds.close()
    print(f"benchmark model n=4096: table {table} generic {generic}")
    assert tot_c == tot and math.isfinite(tot), (tot, tot_c)
    assert table + generic == 64, (table, generic)
    assert generic == PARENT_GENERIC_4096, (generic, PARENT_GENERIC_4096)
