"""The lean pass's dispatch order (lean_kernel's LeanFirst list: the chunks the
host predicts to hold a breakpoint of the series decision are taken by the
first waves of the grid) changes nothing but the order in which chunks are
taken.

A context with the list on (WFPT_LEAN_FIRST_MIN=0: the "more than one dispatch
round" threshold lowered so that small data exercises the path) against one
with it off (WFPT_LEAN_FIRST=0): byte-equal totals, byte-equal chunk partials
and zero words (wfpt_debug_partials, as tests/test_parity_summing.py reads
them) and the same last_path. The reported list (wfpt_debug_lean_first) equals
a brute-force prediction from the stored data: per boundary, t node and
breakpoint, the last chunk of that boundary whose smallest |rt| is <= tc_j +
a^2 hi (hi: the upper edge of the piece below the breakpoint, 1e-6 relative
under it), for an r within the boundary's data.

Shapes: n = 3,072 and 3,001 (a ragged last chunk), |rt| over 0.36-6 s on both
boundaries, the benchmark's parameters and knobs. Both contexts set
WFPT_LEAN_TREE=1.0 so that every call takes the lean pass.
"""
import struct

import numpy as np
import pytest

from test_lean_decision_table import BAND, BP, t_nodes
from test_lean_uniform import KN, PINNED, _open_ctx, eng_ctx, node_decisions  # noqa: F401


@pytest.fixture(scope="module")
def on_ctx(gpu):
    ctx = _open_ctx({"WFPT_LEAN_TREE": "1.0", "WFPT_LEAN_FIRST_MIN": "0"})
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def off_ctx(gpu):
    ctx = _open_ctx({"WFPT_LEAN_TREE": "1.0", "WFPT_LEAN_FIRST": "0"})
    yield ctx
    ctx.close()


def sample(n, seed, frac_upper=0.6, lo=0.36, hi=6.0):
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 1.0, n)
    mag = lo + (hi - lo) * u * u  # denser at short RTs
    return np.where(rng.uniform(0.0, 1.0, n) < frac_upper, mag, -mag)


def predicted(stored, args):
    """The brute-force list from the stored trials: every chunk's smallest
    |rt| per boundary, scanned for each (boundary, t node, breakpoint)."""
    a = args[2]
    nb = (len(stored) + 63) // 64
    out = set()
    for upper in (False, True):
        mine = (stored > 0) if upper else (stored <= 0)  # NaN RTs: neither
        if not mine.any():
            continue
        top = np.abs(stored[mine]).max()
        cmin = np.full(nb, np.inf)
        for c in range(nb):
            seg = stored[64 * c:64 * c + 64]
            m = mine[64 * c:64 * c + 64]
            if m.any():
                cmin[c] = np.abs(seg[m]).min()
        for tc in t_nodes(args):
            for bp in BP:
                # the piece below the breakpoint ends at the last double before it,
                # less the guard band
                r = tc + np.nextafter(bp, 0.0) * (1.0 - BAND) * (a * a)
                owners = np.flatnonzero(cmin <= r)
                if owners.size and r <= top:
                    out.add(int(owners[-1]))
    return sorted(out)[-64:]


def bits(v):
    return struct.pack("d", v)


def compare(gpu, on_ctx, off_ctx, x, args=PINNED, lean=True, calls=1, **ds_kw):
    """`calls` plain calls per context, the last one compared; returns (list of
    the on context, stored trials)."""
    from hddm_amd import _lib
    nb = (len(x) + 63) // 64
    got = []
    for ctx in (on_ctx, off_ctx):
        ds = gpu.Dataset(x, ctx=ctx, **ds_kw)
        for _ in range(calls):
            tot = ds.wiener_like(*args, *KN)
        path = ctx.last_path()
        part, zero = ctx.partials(nb)
        got.append((tot, path, part.copy(), zero.copy(), ctx.lean_first(), x[ds.order()]))
        ds.close()
    (tot, path, part, zero, first, stored), (tot0, path0, part0, zero0, first0, _) = got
    assert bits(tot) == bits(tot0), (tot, tot0)
    assert path == path0, (path, path0)
    assert bool(path & _lib.PATH_LEAN) and bool(path & _lib.PATH_SMALL) != lean, path
    assert np.array_equal(part.view(np.int64), part0.view(np.int64)), np.flatnonzero(part != part0)
    assert np.array_equal(zero, zero0)
    assert first0 == []
    return first, stored


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3072, 3001])
def test_list_on_equals_list_off(gpu, on_ctx, off_ctx, n):
    x = sample(n, 100 + n)
    first, stored = compare(gpu, on_ctx, off_ctx, x)
    want = predicted(stored, PINNED)
    print(f"n={n}: listed {first}")
    assert first == want, (first, want)
    # several breakpoints fall inside chunks, on both boundaries
    n_lower = int((stored <= 0).sum())
    assert len(first) >= 10 and first[0] * 64 < n_lower <= first[-1] * 64, (first, n_lower)


@pytest.mark.gpu
def test_ragged_last_chunk_is_listed(gpu, on_ctx, off_ctx):
    """n = 3,001: the last chunk holds 57 trials. The 40 largest upper |rt| are
    moved onto 6.40..6.60, around the K = 2 -> 1 breakpoint of the five t
    nodes (6.43..6.53 s at a = 2)."""
    x = sample(3001, 7)
    up = np.flatnonzero(x > 0)
    top = up[np.argsort(x[up])[-40:]]
    x[top] = np.linspace(6.40, 6.60, 40)
    first, stored = compare(gpu, on_ctx, off_ctx, x)
    assert first == predicted(stored, PINNED), first
    assert first[-1] == 3001 // 64, first


@pytest.mark.gpu
def test_mixed_boundary_chunk_is_listed(gpu, on_ctx, off_ctx):
    """1,300 lower trials (1,300 = 20 * 64 + 20: chunk 20 holds both
    boundaries) and 1,772 upper ones whose 30 smallest |rt| are 0.46..0.58,
    around the first breakpoint of the five t nodes (0.471..0.571 s)."""
    rng = np.random.default_rng(11)
    lower = -(0.36 + 5.64 * rng.uniform(0.0, 1.0, 1300) ** 2)
    upper = np.concatenate([np.linspace(0.46, 0.58, 30),
                            0.60 + 5.40 * rng.uniform(0.0, 1.0, 1742) ** 2])
    x = rng.permutation(np.concatenate([lower, upper]))
    first, stored = compare(gpu, on_ctx, off_ctx, x)
    assert first == predicted(stored, PINNED), first
    assert stored[20 * 64] <= 0 < stored[20 * 64 + 63] and 20 in first, first


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["upper", "lower"])
def test_one_boundary(gpu, on_ctx, off_ctx, sign):
    x = sign * np.abs(sample(3072, 13))
    first, stored = compare(gpu, on_ctx, off_ctx, x)
    assert first == predicted(stored, PINNED) and len(first) >= 5, first


@pytest.mark.gpu
def test_one_block_call_has_no_list(gpu, on_ctx, off_ctx):
    """n <= 256: a call predicted to defer nothing (the dataset's second call)
    takes the one-block kernel; the list is not used, and the first call's
    list (lean_kernel over four chunks) is not reported for it."""
    x = sample(200, 17)
    first, stored = compare(gpu, on_ctx, off_ctx, x)
    assert first == predicted(stored, PINNED) and first, first
    first, _ = compare(gpu, on_ctx, off_ctx, x, lean=False, calls=2)
    assert first == []


@pytest.mark.gpu
def test_input_order_has_no_index(gpu, on_ctx, off_ctx):
    first, _ = compare(gpu, on_ctx, off_ctx, sample(3001, 19), input_order=True)
    assert first == []


@pytest.mark.gpu
def test_nan_rts(gpu, on_ctx, off_ctx):
    """NaN RTs are stored last among the lower boundary's trials: they are no
    part of either boundary's range."""
    x = sample(3001, 23)
    x[[5, 700, 1500, 2222, 3000]] = np.nan
    first, stored = compare(gpu, on_ctx, off_ctx, x)
    n_lower = int((stored <= 0).sum())
    assert np.isnan(stored[n_lower:n_lower + 5]).all() and (stored[n_lower + 5:] > 0).all()
    assert first == predicted(stored, PINNED) and len(first) >= 10, first


@pytest.mark.gpu
def test_parameters_move_the_list(gpu, on_ctx, off_ctx):
    """The list follows (a, t, st) from call to call on one dataset."""
    x = sample(3072, 29)
    seen = []
    for args in (PINNED, (0.5, 0.1, 1.5, 0.5, 0.1, 0.25, 0.2)):
        first, stored = compare(gpu, on_ctx, off_ctx, x, args)
        assert first == predicted(stored, args), (args, first)
        seen.append(first)
    assert seen[0] != seen[1]


@pytest.mark.gpu
@pytest.mark.parametrize("k,j", [(3, 2), (1, 0), (4, 4)])
def test_wave_split_by_the_table(gpu, on_ctx, off_ctx, eng_ctx, k, j):
    """Five upper-boundary waves (two inside one piece at every node on either
    side); the middle one is an even ramp that carries
    node j's tt across breakpoint k (from 0.32 below to 0.48 above it in units
    of the t nodes' spacing, so every node of its two extreme lanes lies inside
    a piece): the table proves it split, it skips the per-lane pre-pass and
    takes the generic site. Its bits are the engine's per-lane level 0, and the
    counting build tallies it generic and the other four settled by the table."""
    from hddm_amd import _lib
    rng = np.random.default_rng(300 + 10 * k + j)
    a, tcs = PINNED[2], t_nodes(PINNED)
    step = tcs[1] - tcs[0]
    ramp = tcs[j] + (a * a) * BP[k] + step * np.linspace(-0.32, 0.48, 64)
    small, K = node_decisions(ramp, PINNED, KN[0])
    code = small * 100 + K
    assert code[0, j] != code[-1, j], (k, j, code[0], code[-1])
    # two waves below the ramp and two above it, each inside one piece at every node
    regions = [(0.60, 0.80), (1.30, 1.90), (2.6, 5.9), (6.6, 7.0)]
    lo = [r for r in regions if r[1] < ramp[0]][-1]
    hi = [r for r in regions if r[0] > ramp[-1]][0]
    below = np.sort(rng.uniform(*lo, 128))
    above = np.sort(rng.uniform(*hi, 128))
    for seg in (below[:64], below[64:], above[:64], above[64:]):
        s, kk = node_decisions(seg, PINNED, KN[0])
        c = s * 100 + kk
        assert (c == c[0]).all(), (k, j, np.unique(c, axis=0))
    x = np.concatenate([below, ramp, above])
    de = gpu.Dataset(x, ctx=eng_ctx)
    tot_e, terms_e = de.wiener_like_trials(*PINNED, *KN)
    assert eng_ctx.last_path() & _lib.PATH_ENGINE and not eng_ctx.last_path() & _lib.PATH_LEAN
    de.close()
    for ctx in (on_ctx, off_ctx):
        ds = gpu.Dataset(x, ctx=ctx)
        tot, terms = ds.wiener_like_trials(*PINNED, *KN)
        assert ctx.last_path() & _lib.PATH_LEAN and not ctx.last_path() & _lib.PATH_SMALL
        assert bits(tot) == bits(tot_e), (tot, tot_e)
        assert np.array_equal(np.asarray(terms).view(np.int64), np.asarray(terms_e).view(np.int64))
        ctx.profile(ctx.PROF_EVALS)
        try:
            ctx.profile_lists(reset=True)
            tot_c = ds.wiener_like(*PINNED, *KN)
            counts = ctx.profile_lists(reset=True)
        finally:
            ctx.profile(0)
        assert bits(tot_c) == bits(tot), (tot_c, tot)
        assert (counts["lean_table"], counts["lean_generic"]) == (4, 1), counts
        if ctx is on_ctx:
            assert 2 in ctx.lean_first(), ctx.lean_first()
        ds.close()
