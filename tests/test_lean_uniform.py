"""The lean pass's uniform waves (lean_kernel<kAdaptTZ>: per-t-node series
decisions in scalar registers, host tables, one range test per trial) against
the per-lane code they replace.

Every dataset below is checked three ways:
  1. Bitwise against the engine: the per-trial terms of wiener_like_trials on a
     forced-lean context (WFPT_LEAN_TREE=1.0, as tests/test_parity_summing.py's
     lean_ctx) are bit-equal, as int64 views, to the terms of the same
     dataset's first call on a default context, which takes the engine (per-lane
     level 0); totals equal too.
  2. Against the oracle: terms within 1e-6 of the reference's addends with -inf
     in the same places, every chunk partial within 1e-12 sum|terms| + 1e-12 of
     fsum (the project's bars, tests/test_parity_summing.py).
  3. The plain call's chunk partials are bit-equal to the per-trial build's.
The counting build tallies the lean waves that took the generic (per-lane)
site (wfpt_profile_lists counts[3], "lean_generic").

Two expectations of the change's write-up do not hold by the reference's own
formulas (pdf.pxi:36-60, `decisions` below) and are stated here as they are:
  * err = 1e-10 gives K = 3..5 at these parameters, inside the tables' limit of
    8, so those waves are uniform; K > 8 on both series needs err < ~1e-60,
    where the fp32 decision estimate is out of range and every wave is
    generic. Both err = 1e-10 and err = 1e-80 (K up to 12) are run.
  * the stress sets and |v| = 6, sv = 2, a = 0.6 mostly pass the per-trial
    range test (they refine instead); a set with |v| = 12 is added whose
    drift exponents fail it, so the per-node guards decide there.
"""
import math
import os

import numpy as np
import pytest

KN = (1e-4, 2, 2, 1, 1e-3, 0.05, 0.1)  # HDDM's knobs + p_outlier
PINNED = (0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1)  # the bench parameters
# tests/test_parity_summing.py STRESS[0:2]
STRESS = [(-1.2388, 1.3918, 1.4387, 0.4995, 0.2891, 0.277, 0.0698),
          (1.7431, 2.0137, 0.6119, 0.5386, 0.2108, 0.3567, 0.1981)]
THRESHOLDS = (0.522, 0.915, 1.165, 2.097)  # centre-node decision changes, bench parameters


def threads():
    env = os.environ.get("OMP_NUM_THREADS")
    return int(env) if env and env.isdigit() else len(os.sched_getaffinity(0))


def ref_terms(oracle_lib, x, args, kn=KN):
    return oracle_lib.pdf_array(x, *args, kn[0], 1, kn[1], kn[2], kn[3], kn[4], kn[5], kn[6],
                                n_threads=threads())


def assert_terms(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    zr, zg = np.isneginf(ref), np.isneginf(got)
    assert np.array_equal(zr, zg), (what, np.flatnonzero(zr != zg)[:10])
    fin = ~zr
    assert np.all(np.isfinite(got[fin])), (what, np.flatnonzero(~np.isfinite(got[fin]))[:10])
    d = np.abs(got[fin] - ref[fin])
    assert d.size == 0 or d.max() < 1e-6, (what, d.max(), np.argmax(d))


def assert_chunks(ctx, ds, ref, what):
    n = len(ds)
    nb = (n + 63) // 64
    part, zero = ctx.partials(nb)
    r = ref[ds.order()]
    for c in range(nb):
        seg = r[64 * c:64 * c + 64]
        fin = seg[np.isfinite(seg)]
        nz = int(np.isneginf(seg).sum())
        assert (int(zero[c]) & 0xFFFF) == nz, (what, c, zero[c], nz)
        want = math.fsum(fin)
        scale = math.fsum(np.abs(fin))
        assert abs(part[c] - want) <= 1e-12 * scale + 1e-12, (what, c, part[c], want, scale)


def summing_vs_trials(ctx, ds, args, kn):
    tot = ds.wiener_like(*args, *kn)
    path = ctx.last_path()
    nb = (len(ds) + 63) // 64
    part, zero = ctx.partials(nb)
    tot2, terms = ds.wiener_like_trials(*args, *kn)
    assert ctx.last_path() == path, (path, ctx.last_path())
    part2, zero2 = ctx.partials(nb)
    assert tot2 == tot or (math.isnan(tot) and math.isnan(tot2)), (tot, tot2)
    assert np.array_equal(part.view(np.int64), part2.view(np.int64))
    assert np.array_equal(zero, zero2)
    return tot, terms, path


def _open_ctx(env):
    from hddm_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def lean_ctx(gpu):
    """Resident calls always take the lean level-0 pass (chunks that refine go
    to the engine's redo pass)."""
    ctx = _open_ctx({"WFPT_LEAN_TREE": "1.0"})
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def eng_ctx(gpu):
    """A default context of this module's own: a new dataset's first call on it
    has nothing predicted and takes the engine."""
    ctx = _open_ctx({})
    yield ctx
    ctx.close()


def decisions(tt, err):
    """(small, K) of pdf.pxi:36-60 for an array of normalised times."""
    tt = np.asarray(tt, dtype=np.float64)
    sqt = np.sqrt(tt)
    ips = 1.0 / (np.pi * sqt)
    al = np.pi * tt * err
    as_ = 2.0 * np.sqrt(2.0 * np.pi * tt) * err
    with np.errstate(invalid="ignore", divide="ignore"):
        kl = np.where(al < 1.0, np.maximum(np.sqrt(-2.0 * np.log(al) / (np.pi ** 2 * tt)), ips), ips)
        ks = np.where(as_ < 1.0, np.maximum(2.0 + np.sqrt(-2.0 * tt * np.log(as_)), sqt + 1.0), 2.0)
    small = ks < kl
    return small, np.ceil(np.where(small, ks, kl)).astype(int)


def node_decisions(x, args, err):
    """Decisions at the five root t nodes of every trial: (n, 5) arrays."""
    a, t, st = args[2], args[5], args[6]
    lb, ub = t - st / 2.0, t + st / 2.0
    c = (ub + lb) / 2.0
    tcs = np.array([lb, (lb + c) / 2.0, c, (c + ub) / 2.0, ub])
    xx = np.abs(np.asarray(x))[:, None] - tcs[None, :]
    assert np.all(xx > 0)
    return decisions(xx / (a * a), err)


def run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, args, what, kn=KN):
    """The three checks; returns (generic-site waves of a counting call, waves)."""
    from hddm_amd import _lib
    ref = ref_terms(oracle_lib, x, args, kn)
    de = gpu.Dataset(x, ctx=eng_ctx)
    tot_e, terms_e = de.wiener_like_trials(*args, *kn)
    assert eng_ctx.last_path() & _lib.PATH_ENGINE, (what, eng_ctx.last_path())
    assert not eng_ctx.last_path() & _lib.PATH_LEAN, (what, eng_ctx.last_path())
    de.close()
    ds = gpu.Dataset(x, ctx=lean_ctx)
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
    # the counting build's tally (and the same total from that build)
    lean_ctx.profile(lean_ctx.PROF_EVALS)
    try:
        lean_ctx.profile_lists(reset=True)
        tot_c = ds.wiener_like(*args, *kn)
        assert lean_ctx.last_path() & _lib.PATH_LEAN, (what, lean_ctx.last_path())
        generic = lean_ctx.profile_lists(reset=True)["lean_generic"]
    finally:
        lean_ctx.profile(0)
    assert tot_c == tot or (math.isnan(tot) and math.isnan(tot_c)), (what, tot, tot_c)
    ds.close()
    waves = (len(x) + 63) // 64
    print(f"{what}: n={len(x)} generic waves {generic} of {waves}")
    return generic, waves


@pytest.mark.gpu
@pytest.mark.parametrize("sides", ["upper", "lower", "mixed"])
@pytest.mark.parametrize("th", THRESHOLDS)
def test_threshold_ramps(gpu, oracle_lib, lean_ctx, eng_ctx, th, sides):
    """|rt| on an even ramp of 2,048 values across a centre-node threshold
    +- 0.08 s (plus 37 more values in the same range: n is no multiple of 64),
    so the threshold of each of the five t nodes (offsets +-0.05) falls inside
    some wave: both the uniform and the generic site run. All upper, all
    lower, and both with the boundary switch in mid-wave."""
    rng = np.random.default_rng(int(th * 1000))
    mag = np.concatenate([np.linspace(th - 0.08, th + 0.08, 2048),
                          rng.uniform(th - 0.08, th + 0.08, 37)])
    if sides == "upper":
        x = mag
    elif sides == "lower":
        x = -mag
    else:
        lower = rng.permutation(mag.size) < 1000  # 1000 = 15 * 64 + 40: the switch is mid-wave
        x = np.where(lower, -mag, mag)
    # the centre node's decision does change inside the ramp, by the reference's formulas
    small, K = node_decisions(mag, PINNED, KN[0])
    code = small[:, 2] * 100 + K[:, 2]
    assert code[np.argmin(mag)] != code[np.argmax(mag)], (th, code.min(), code.max())
    generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, PINNED, f"ramp {th} {sides}")
    assert 0 < generic < waves, (generic, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_inside_one_region(gpu, oracle_lib, lean_ctx, eng_ctx, sign):
    """1,024 RTs in [0.60, 0.80] (small-time, K = 4 at every node) and 1,024 in
    [1.30, 1.90] (large-time, K = 3): no wave takes the generic site."""
    rng = np.random.default_rng(77)
    g1, g2 = rng.uniform(0.60, 0.80, 1024), rng.uniform(1.30, 1.90, 1024)
    s1, k1 = node_decisions(g1, PINNED, KN[0])
    s2, k2 = node_decisions(g2, PINNED, KN[0])
    assert s1.all() and (k1 == 4).all(), (s1.all(), np.unique(k1))
    assert (~s2).all() and (k2 == 3).all(), (s2.any(), np.unique(k2))
    x = sign * np.concatenate([g1, g2])
    generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, PINNED, f"regions {sign}")
    assert generic == 0, (generic, waves)


@pytest.mark.gpu
def test_near_and_below_t(gpu, oracle_lib, lean_ctx, eng_ctx):
    """RTs in (t - st/2, t + st/2 + 0.02]: some t nodes have x - t_node <= 0;
    with a few RTs below t - st/2 (invalid: density 0). Every wave is generic."""
    rng = np.random.default_rng(5)
    t, st = PINNED[5], PINNED[6]
    mag = np.concatenate([rng.uniform(t - st / 2 + 1e-6, t + st / 2 + 0.02, 620),
                          [t + st / 2 + 0.02], rng.uniform(0.20, t - st / 2 - 1e-6, 16)])
    x = mag * rng.choice([-1.0, 1.0], mag.size)
    generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, PINNED, "near t")
    assert generic == waves, (generic, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(0.5, 0.0, 2.0, 0.5, 0.1, 0.3, 0.1),   # sv = 0: the dm = 1 form
                                  (0.5, 0.1, 2.0, 0.2, 0.1, 0.3, 0.1),   # flipped grids
                                  (0.5, 0.1, 2.0, 0.8, 0.1, 0.3, 0.1)])
def test_other_families_of_the_kernel(gpu, oracle_lib, lean_ctx, eng_ctx, args):
    """sv = 0 and flipped grids on both series of the uniform site: RTs of both
    boundaries inside the two regions of test_inside_one_region (a, t, st as
    there, so the same decisions), n no multiple of 64. Only the wave at the
    boundary switch and the one per boundary where the region changes can be
    generic."""
    rng = np.random.default_rng(11)
    mag = np.concatenate([rng.uniform(0.60, 0.80, 1024 + 37), rng.uniform(1.30, 1.90, 1024)])
    small, K = node_decisions(mag, args, KN[0])
    assert set(zip(small.ravel().tolist(), K.ravel().tolist())) == {(True, 4), (False, 3)}
    x = rng.choice([-1.0, 1.0], mag.size) * mag
    generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, args, f"family {args}")
    assert generic <= 3, (generic, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("err", [1e-10, 1e-80])
def test_term_count_limits(gpu, oracle_lib, lean_ctx, eng_ctx, err):
    """err = 1e-10: K = 3..5, inside the tables (uniform waves run). err =
    1e-80: K > 8 at most nodes and the fp32 decision estimate is out of range,
    so every wave takes the generic site."""
    rng = np.random.default_rng(13)
    n = 1024 + 37
    mag = 0.36 + rng.gamma(2.0, 0.35, n)
    x = rng.choice([-1.0, 1.0], n) * mag
    kn = (err,) + KN[1:]
    _, K = node_decisions(mag, PINNED, err)
    generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, PINNED, f"err {err}", kn)
    if err == 1e-10:
        assert 4 < K.max() <= 8, np.unique(K)
    else:
        assert K.max() > 8, np.unique(K)
        assert generic == waves, (generic, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(4))
def test_guard_fallback(gpu, oracle_lib, lean_ctx, eng_ctx, k):
    """Parameters at which drift exponents are large: the two full-DDM stress
    sets, |v| = 6 with sv = 2, a = 0.6, and |v| = 12, whose exponents fail the
    per-trial range test (14 * 0.5 * v^2 (x - lb) > 600 from x - lb = 0.6 on),
    so the per-node guards of the generic site decide."""
    args = [STRESS[0], STRESS[1], (-6.0, 2.0, 0.6, 0.5, 0.2, 0.3, 0.1),
            (12.0, 0.5, 1.0, 0.5, 0.1, 0.3, 0.1)][k]
    rng = np.random.default_rng(2000 + k)
    n = 2048
    x = rng.choice([-1.0, 1.0], n) * (0.32 + rng.gamma(2.0, 0.4, n))
    x = np.where(np.abs(x) < args[5] + args[6] / 2 + 0.01, np.sign(x) * 0.5, x)
    ref = ref_terms(oracle_lib, x, args)
    assert np.isfinite(ref).mean() >= 0.9  # the comparison is not vacuous
    generic, waves = run_case(gpu, oracle_lib, lean_ctx, eng_ctx, x, args, f"guard {k}")
    if k == 3:
        assert generic > waves // 2, (generic, waves)
