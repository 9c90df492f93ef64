"""Model comparison: DIC and WAIC from one device pass over the trace.

The reference reports `m.dic` / `m.dic_info()` (kabuki over PyMC's deviance
trace, docs/source/tutorial_python.rst:574-579); neither package is available
here, so the formulas are stated:

    D_s      = -2 sum_nodes logp(nodes | sweep s)
    deviance = mean_s D_s
    D_hat    = -2 sum_nodes logp(nodes | posterior mean of every likelihood parent)
    pD       = deviance - D_hat,   DIC = deviance + pD

WAIC (Watanabe 2010; Vehtari, Gelman & Gabry 2017) needs, per trial i, the log
of the mean density over the sweeps (lppd_i) and the sample variance of the log
density (p_waic_i). Both are reductions over the sweeps of the S x n matrix of
per-trial log terms, which the library forms next to the terms, on the device
(wfpt.Dataset.pointwise_nodes and its RL / regression siblings):

    elpd_waic = sum_i (lppd_i - p_waic_i),   waic = -2 elpd_waic
    se        = 2 sqrt(n var_i(lppd_i - p_waic_i))

`Pointwise` gives HDDM, HDDMrl and HDDMRegressor `pointwise_loglik`,
`dic_info`, `dic` and `waic`; `compare` ranks fitted models.
"""
import math

import numpy as np

HIGH_VAR = 0.4  # p_waic_i above this: the usual warning sign (Vehtari et al. 2017, §2.2)


def dic_from(sums, mean_sums):
    """{'DIC', 'deviance', 'pD'} from the (S, nodes) per-sweep node sums and
    the node sums at the posterior mean."""
    D = -2.0 * np.sum(np.asarray(sums, dtype=np.float64), axis=1)
    deviance = float(np.mean(D))
    d_hat = -2.0 * float(np.sum(mean_sums))
    pD = deviance - d_hat
    return {"DIC": deviance + pD, "deviance": deviance, "pD": pD}


def waic_from(pw):
    """The WAIC summary of a pointwise dict (`lppd`, `p_waic`, `n_inf`, `trial`
    per scored trial). A trial that no sweep gave a density (lppd = -inf) has
    elpd = -inf: waic is inf, not an error."""
    lppd = np.asarray(pw["lppd"], dtype=np.float64)
    p = np.asarray(pw["p_waic"], dtype=np.float64)
    dead = lppd == -np.inf
    with np.errstate(invalid="ignore"):
        elpd = np.where(dead, -np.inf, lppd - p)
        n = elpd.size
        se = 2.0 * math.sqrt(n * float(np.var(elpd))) if n and not dead.any() else float("nan")
    elpd_waic = math.fsum(elpd.tolist())
    return {"elpd_waic": elpd_waic, "waic": -2.0 * elpd_waic,
            "p_waic": math.fsum(p[~dead].tolist()), "lppd": math.fsum(lppd.tolist()),
            "se": se, "n_trials": int(n), "n_inf": int(np.sum(pw["n_inf"])),
            "n_high_var": int(np.sum(p[~dead] > HIGH_VAR)), "elpd": elpd,
            "trial": np.asarray(pw["trial"])}


class Pointwise:
    """pointwise_loglik / dic_info / dic / waic for a sampler that keeps its
    traces. A class states three things: `_pw_kept()` (kept sweeps),
    `_pw_score(picked)` (ONE binding call over the tables of those sweeps ->
    the pointwise dict) and `_pw_mean_logp(picked)` (one ordinary node call on
    the table of their trace means -> node sums)."""

    def _pw_kept(self):
        if not isinstance(getattr(self, "trace", None), dict) \
                or not isinstance(getattr(self, "trace_subj", None), dict):
            raise RuntimeError("model comparison needs the traces: run sample() first")
        return len(next(iter(self.trace.values())))

    def _pw_picked(self, samples):
        kept = self._pw_kept()
        if samples is None:
            if kept < 1:
                raise RuntimeError("model comparison: sample() kept no sweep")
            return np.arange(kept, dtype=np.int64)
        return self._picked_sweeps(samples, kept)

    def _pw_ddm_table(self, picked, mean=False):
        """The (S, n_nodes, 8) parameter tables of the picked sweeps, or with
        mean=True the (n_nodes, 8) table at the mean over them of every
        subject value and every included sv / sz / st."""
        from .hierarchical import INTER
        if mean:
            subj = {f: self.trace_subj[f][picked].mean(axis=0) for f in self.FAMILIES}
            inter = {n: float(np.mean(self.trace[n][picked])) if n in self.include
                     else self.inter[n] for n in INTER}
            return self._table_of((), subj, inter)
        subj = {f: self.trace_subj[f][picked] for f in self.FAMILIES}
        inter = {n: self.trace[n][picked][:, None] if n in self.include else self.inter[n]
                 for n in INTER}
        return self._table_of((picked.size,), subj, inter)

    def pointwise_loglik(self, samples=None):
        """The kept sweeps (all by default, else `samples` evenly spaced ones)
        through the model's table builder and ONE device pass: a dict of
        `sums` (S, n_nodes) per-sweep node log-likelihoods, per scored trial
        `lppd`, `p_waic`, `mean`, `n_inf` and `trial` (the row of the model's
        data), and `picked`. Cached for the current traces and `samples`."""
        cache = getattr(self, "_pw_cache", None)
        if cache is not None and cache[0] is self.trace and cache[1] == samples:
            return cache[2]
        picked = self._pw_picked(samples)
        pw = dict(self._pw_score(picked), picked=picked)
        self._pw_cache = (self.trace, samples, pw)
        return pw

    def dic_info(self, samples=None):
        """{'DIC', 'deviance', 'pD'}: the mean deviance over the kept sweeps,
        and the deviance at the posterior mean of every likelihood parent (one
        ordinary node call on the table of trace means)."""
        pw = self.pointwise_loglik(samples)
        return dic_from(pw["sums"], self._pw_mean_logp(pw["picked"]))

    @property
    def dic(self):
        return self.dic_info()["DIC"]

    def waic(self, samples=None):
        """WAIC from the per-trial statistics: a dict of elpd_waic, waic,
        p_waic, lppd, se, n_trials, n_inf ((sweep, trial) pairs with a zero
        density), n_high_var (trials with p_waic_i > 0.4) and the pointwise
        `elpd` with its `trial` index."""
        return waic_from(self.pointwise_loglik(samples))


def compare(models):
    """{'name': fitted model} -> DataFrame sorted by WAIC (best first) with
    columns waic, p_waic, d_waic (to the best model), dse (the standard error
    of that difference, from the pointwise elpd differences; NaN unless both
    models were scored on the same trials), dic and pD."""
    import pandas as pd
    if not models:
        raise ValueError("compare needs at least one model")
    w = {name: m.waic() for name, m in models.items()}
    d = {name: m.dic_info() for name, m in models.items()}
    order = sorted(w, key=lambda name: (w[name]["waic"], name))
    best = w[order[0]]
    rows = []
    for name in order:
        cur = w[name]
        dse = float("nan")
        if cur is best:
            dse = 0.0
        elif cur["n_trials"] == best["n_trials"] and np.array_equal(cur["trial"], best["trial"]):
            with np.errstate(invalid="ignore"):
                diff = best["elpd"] - cur["elpd"]
                dse = 2.0 * math.sqrt(diff.size * float(np.var(diff))) \
                    if np.all(np.isfinite(diff)) else float("nan")
        with np.errstate(invalid="ignore"):
            d_waic = cur["waic"] - best["waic"]
        rows.append({"waic": cur["waic"], "p_waic": cur["p_waic"], "d_waic": d_waic, "dse": dse,
                     "dic": d[name]["DIC"], "pD": d[name]["pD"]})
    return pd.DataFrame(rows, index=pd.Index(order, name="model"))
