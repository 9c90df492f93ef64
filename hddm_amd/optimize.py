"""`HDDM.optimize`: maximum-likelihood, chi-square and G-square point fits.

The reference's `model.optimize(method, quantiles, n_runs, n_bootstraps)`
(hddm/models/base.py:47-308) on the flat model of its average / single-subject
model: one free value per (family, condition level) of a, v and t, one each for
the included sv, sz and st, z fixed at 0.5. The quantile objectives evaluate
every condition's row in ONE `cdfdif_wrapper.dmat_cdf_rows` launch per
evaluation; 'ML' sums the existing per-node likelihood kernel.

The bootstrap (base.py:145-195) resamples the trials with replacement and
refits; the reference farms the replicates out to IPython.parallel. Here the
replicates are minimised in lockstep by a batched Nelder-Mead
(`_lockstep_minimize`), every stage of an iteration one launch over the rows
of all replicates that need it.
"""
import numpy as np

from . import cdfdif_wrapper
from .hierarchical import INTER, param_table
from .quantiles import DEFAULT_QUANTILES, pool_stats, quantile_stats

METHODS = ("ML", "chisquare", "gsquare")


# ---------------------------------------------------------------- lockstep simplex

def _lockstep_minimize(batch_objective, x0, xtol=1e-4, ftol=1e-4, maxiter=None):
    """Nelder-Mead (the steps and constants of scipy.optimize.fmin) on B
    independent problems at once.

    batch_objective(X, idx) -> f: X (n, d) points, idx (n,) the problem each
    point belongs to, f (n,) their values; one call per stage of an iteration
    (reflect, expand, contract, shrink) over the problems that need it. x0:
    (B, d) starting points. A problem stops when its simplex is within xtol and
    its values within ftol of the best vertex, or after maxiter (200 d)
    iterations. Every operation is elementwise over the problem axis or a loop
    over vertices in a fixed order, so a problem's trajectory does not depend on
    which other problems run beside it (given a batch_objective with the same
    property).

    Returns (x (B, d), f (B,), iterations (B,), evaluations (B,))."""
    x0 = np.array(x0, dtype=np.float64, ndmin=2)
    B, d = x0.shape
    if maxiter is None:
        maxiter = 200 * d
    rho, chi, psi, sigma = 1.0, 2.0, 0.5, 0.5
    sim = np.empty((B, d + 1, d))
    sim[:, 0] = x0
    for k in range(d):  # scipy's initial simplex: 5 % steps, 0.00025 from a zero
        y = x0.copy()
        y[:, k] = np.where(y[:, k] != 0, (1 + 0.05) * y[:, k], 0.00025)
        sim[:, k + 1] = y
    every = np.arange(B)
    fsim = batch_objective(sim.reshape(B * (d + 1), d),
                           np.repeat(every, d + 1)).reshape(B, d + 1).copy()
    evals = np.full(B, d + 1, dtype=np.int64)
    iters = np.zeros(B, dtype=np.int64)
    active = np.ones(B, dtype=bool)

    def order(p):
        o = np.argsort(fsim[p], axis=1, kind="stable")
        fsim[p] = np.take_along_axis(fsim[p], o, axis=1)
        sim[p] = np.take_along_axis(sim[p], o[:, :, None], axis=1)

    order(every)
    while True:
        p = np.flatnonzero(active)
        if p.size:
            dx = np.max(np.abs(sim[p, 1:] - sim[p, :1]).reshape(p.size, -1), axis=1)
            df = np.max(np.abs(fsim[p, :1] - fsim[p, 1:]), axis=1)
            active[p[((dx <= xtol) & (df <= ftol)) | (iters[p] >= maxiter)]] = False
            p = np.flatnonzero(active)
        if p.size == 0:
            break
        iters[p] += 1
        xbar = sim[p, 0].copy()
        for j in range(1, d):  # the d best vertices, in vertex order
            xbar = xbar + sim[p, j]
        xbar = xbar / d
        worst = sim[p, d]
        f0, fn, fw = fsim[p, 0], fsim[p, d - 1], fsim[p, d]
        xr = (1 + rho) * xbar - rho * worst
        fr = batch_objective(xr, p)
        evals[p] += 1
        new_x, new_f = xr.copy(), fr.copy()  # the vertex that replaces the worst
        shrink = np.zeros(p.size, dtype=bool)
        ex = np.flatnonzero(fr < f0)
        if ex.size:
            xe = (1 + rho * chi) * xbar[ex] - rho * chi * worst[ex]
            fe = batch_objective(xe, p[ex])
            evals[p[ex]] += 1
            better = fe < fr[ex]
            new_x[ex[better]] = xe[better]
            new_f[ex[better]] = fe[better]
        co = np.flatnonzero(~(fr < f0) & ~(fr < fn))
        if co.size:
            outside = fr[co] < fw[co]
            xc = np.where(outside[:, None],
                          (1 + psi * rho) * xbar[co] - psi * rho * worst[co],
                          (1 - psi) * xbar[co] + psi * worst[co])
            fc = batch_objective(xc, p[co])
            evals[p[co]] += 1
            ok = np.where(outside, fc <= fr[co], fc < fw[co])
            new_x[co[ok]] = xc[ok]
            new_f[co[ok]] = fc[ok]
            shrink[co[~ok]] = True
        keep = ~shrink
        sim[p[keep], d] = new_x[keep]
        fsim[p[keep], d] = new_f[keep]
        sh = p[shrink]
        if sh.size:
            for j in range(1, d + 1):
                sim[sh, j] = sim[sh, 0] + sigma * (sim[sh, j] - sim[sh, 0])
            fsim[sh, 1:] = batch_objective(sim[sh, 1:].reshape(sh.size * d, d),
                                           np.repeat(sh, d)).reshape(sh.size, d)
            evals[sh] += d
        order(p)
    return sim[:, 0].copy(), fsim[:, 0].copy(), iters, evals


# ---------------------------------------------------------------- the flat model

class _FlatModel:
    """The free values of the flat model and the rows they parameterise.

    names / slots: one entry per (family, condition level) of a, v, t in
    gen_stats()' group-node naming, then the included sv, sz, st. A row is an
    observed node (one subject) or a condition tag (several subjects: the
    average model, base.py:78-112)."""

    def __init__(self, m):
        self.m = m
        nodes = list(m.group_nodes()) + [(name, name, None) for name in m.inter_names]
        self.names = [name for name, _, _ in nodes]
        self.slots = [(s, k) for _, s, k in nodes]
        self.d = len(self.names)
        # rows: the nodes, or one per condition tag (its first node gives the levels)
        tags = [key[1:] for key in m.node_keys]
        if m.n_subj > 1:
            self.tags = sorted(set(tags))
            self.node_row = np.array([self.tags.index(t) for t in tags])
        else:
            self.tags = tags
            self.node_row = np.arange(m.n_nodes)
        first = [int(np.flatnonzero(self.node_row == r)[0]) for r in range(len(self.tags))]
        # column of the value vector behind each (row, parameter)
        col = {s: i for i, s in enumerate(self.slots)}
        self.row_col = {fam: np.array([col[(fam, int(m.node_level[fam][n]))] for n in first])
                        for fam in m.FAMILIES}
        self.node_col = {fam: np.array([col[(fam, int(k))] for k in m.node_level[fam]])
                         for fam in m.FAMILIES}
        self.inter_col = {n: col.get((n, None)) for n in INTER}

    def current(self):
        m = self.m
        return np.array([m.group[s][k] if k is not None else m.inter[s] for s, k in self.slots],
                        dtype=np.float64)

    def table(self, X, cols):
        """(n, rows, 8) parameter rows of the value vectors X (n, d); cols:
        row_col (quantile rows) or node_col (the observed nodes)."""
        X = np.asarray(X, dtype=np.float64)
        vals = {fam: X[:, c] for fam, c in cols.items()}
        for name, i in self.inter_col.items():
            vals[name] = self.m.inter[name] if i is None else X[:, i:i + 1]
        return param_table((X.shape[0], cols["a"].size), vals, self.m.p_outlier)

    def row_stats(self, rt, node, quantiles):
        """(emp_rt, freq_obs, n_samples) arrays over the rows for signed RTs
        `rt` with node codes `node` (the data, or a bootstrap resample)."""
        m = self.m
        per_node = []
        for n in range(m.n_nodes):
            key = m.node_keys[n]
            per_node.append(quantile_stats(rt[node == n], quantiles,
                                           name=f"wfpt{key[1:] if key[1:] else ''}.{key[0]}"))
        if m.n_subj > 1:
            rows = [pool_stats([per_node[n] for n in np.flatnonzero(self.node_row == r)])
                    for r in range(len(self.tags))]
        else:
            rows = per_node
        return (np.array([s["emp_rt"] for s in rows]), np.array([s["freq_obs"] for s in rows]),
                np.array([float(s["n_samples"]) for s in rows]))


def _quantile_scores(flat, method, X, emp_rt, freq, n):
    """The objective at each value vector of X (n, d) against the row
    statistics emp_rt / freq / n, (n, rows, ...) or (rows, ...) shared by all:
    one launch of n x rows rows."""
    P = flat.table(X, flat.row_col)
    k, R = P.shape[:2]
    if emp_rt.ndim == 2:
        emp_rt, freq, n = (np.broadcast_to(a, (k,) + a.shape) for a in (emp_rt, freq, n))
    _, chisq, gsq = cdfdif_wrapper.dmat_cdf_rows(
        emp_rt.reshape(k * R, -1), P.reshape(k * R, 8), flat.m.wp["w_outlier"],
        freq.reshape(k * R, -1), n.reshape(k * R))
    per = (chisq if method == "chisquare" else -gsq).reshape(k, R)
    out = per[:, 0].copy()
    for r in range(1, R):  # row order, whatever k
        out = out + per[:, r]
    return out


def optimize(m, method, quantiles=DEFAULT_QUANTILES, n_runs=3, n_bootstraps=0, seed=None):
    """The body of HDDM.optimize (see there)."""
    from scipy.optimize import fmin, fmin_powell
    if method not in METHODS:
        raise ValueError("unknown optimzation method")  # base.py:267
    if method == "ML" and m.n_subj > 1:
        raise TypeError("optimization method is not defined for group models")  # base.py:203
    if method == "ML" and n_bootstraps:
        raise NotImplementedError("optimize('ML') has no bootstrap: every replicate would need "
                                  "a resident data set of its own")
    flat = _FlatModel(m)
    rng = m.rng if seed is None else np.random.default_rng(seed)
    rt = m.signed_rt
    if method == "ML":
        def objective(values):
            P = flat.table(np.asarray(values, dtype=np.float64)[None], flat.node_col)[0]
            s = -float(np.sum(m.dataset.wiener_like_nodes(P, **m.wp)))
            return np.inf if s == -np.inf or s != s else s
    else:
        stats = flat.row_stats(rt, m.node_codes, quantiles)

        def objective(values):
            return float(_quantile_scores(flat, method, np.asarray(values)[None], *stats)[0])

    # base.py:270-296
    original = flat.current()
    values = original.copy()
    all_results = []
    inf_objective = False
    for _ in range(int(n_runs)):
        k = 0
        while inf_objective:
            k += 1
            values = original + rng.standard_normal(flat.d) * 2.0 ** -k
            inf_objective = np.isinf(objective(values))
        with np.errstate(invalid="ignore"):  # the line searches subtract infinite scores
            try:
                res = fmin_powell(objective, values, full_output=True, maxiter=100,
                                  maxfun=50000, disp=False)
            except Exception:
                res = fmin(objective, values, full_output=True, maxiter=100, maxfun=50000,
                           disp=False)
        all_results.append(res)
        inf_objective = True
    best = all_results[int(np.nanargmin([r[1] for r in all_results]))]
    best_values = np.atleast_1d(np.asarray(best[0], dtype=np.float64))
    results = dict(zip(flat.names, (float(v) for v in best_values)))
    if method == "gsquare":  # base.py:299-305
        score = objective(best_values)
        penalty = flat.d * np.log(m.n_trials)
        m.bic_info = {"likelihood": -score, "penalty": penalty, "bic": score + penalty}
    if m.n_subj == 1:
        m.set_values(results)
    if n_bootstraps:
        base = int(rng.integers(0, 2 ** 63)) if seed is None else int(seed)
        vals = bootstrap_fits(m, method, quantiles, best_values, base, range(int(n_bootstraps)),
                              flat=flat)
        import pandas as pd
        res = pd.DataFrame(vals, columns=flat.names)
        stats = res.describe()  # base.py:190-194
        for q in (2.5, 97.5):
            stats.loc[repr(q) + "%"] = res.quantile(q / 100.)
        m.bootstrap_values = res
        m.bootstrap_stats = stats.sort_index()
        m.bootstrap_seed = base
    return results


def bootstrap_fits(m, method, quantiles, x0, base_seed, replicates, flat=None):
    """The fitted values (len(replicates), d) of the given bootstrap replicates,
    minimised in lockstep from x0. Replicate b resamples the trials with its own
    generator seeded by (base_seed, b), so it is the same problem whichever
    replicates run beside it."""
    flat = flat or _FlatModel(m)
    rt, node = m.signed_rt, m.node_codes
    reps = []
    for b in replicates:
        idx = np.random.default_rng([int(b), int(base_seed)]).integers(0, rt.size, rt.size)
        reps.append(flat.row_stats(rt[idx], node[idx], quantiles))  # base.py:166
    emp_rt, freq, n = (np.array([r[i] for r in reps]) for i in range(3))

    def batch_objective(X, idx):
        return _quantile_scores(flat, method, X, emp_rt[idx], freq[idx], n[idx])

    x, _, _, _ = _lockstep_minimize(batch_objective, np.tile(np.asarray(x0), (len(reps), 1)))
    return x
