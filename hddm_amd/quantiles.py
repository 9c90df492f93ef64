"""Quantile statistics of observed nodes for the chi-square / G-square fits.

Restates what the reference attaches to its wfpt stochastic
(hddm/likelihoods.py:107-239) and its `data_quantiles` (hddm/utils.py:646-666):
per node the empirical RT quantiles of each boundary (the E = 2 nq + 1 signed
edges the CDF is evaluated at), the observed count of each of the E + 1 bins
between them, and the trial count. The statistics themselves (theoretical bin
proportions, chi-square, G-square) are computed on the GPU for many nodes per
launch by `cdfdif_wrapper.dmat_cdf_rows`; `reduce_stats` is their host
restatement.

Chi-square is the Pearson sum itself. The reference calls
scipy.stats.chisquare (likelihoods.py:225), which in current SciPy raises when
the observed and expected totals differ by more than 1e-8 relative; after the
1e-6 clamp of the proportions they do, so that line cannot be evaluated as
written any more. The sum it used to return is what is computed here.
"""
import numpy as np
from scipy.stats.mstats import mquantiles

__all__ = ["quantile_stats", "pool_stats", "reduce_stats", "DEFAULT_QUANTILES"]

DEFAULT_QUANTILES = (.1, .3, .5, .7, .9)
PROPORTION_FLOOR = 1e-6  # likelihoods.py:212


def quantile_stats(rt_signed, quantiles=DEFAULT_QUANTILES, name="node"):
    """compute_quantiles_stats (likelihoods.py:131-154) over data_quantiles
    (utils.py:646-666) for one node's signed RTs (lower boundary negative).

    Returns a dict: n_samples, emp_rt (2 nq + 1 signed edges, ascending, 0 in
    the middle), freq_obs (2 nq + 2 bin counts), q_lower, q_upper (the RT
    quantiles of each boundary, positive) and p_upper."""
    rt = np.asarray(rt_signed, dtype=np.float64).ravel()
    if np.any(np.isnan(rt)) or np.any(np.abs(rt) >= 999):
        raise NotImplementedError(
            f"{name}: missing RTs (NaN or |rt| >= 999) have no quantile statistics here "
            "(the reference's no-response branch, likelihoods.py:156-175)")
    q = np.asarray(quantiles, dtype=np.float64)
    n_lower, n_upper = int(np.sum(rt < 0)), int(np.sum(rt > 0))
    if n_lower == 0 or n_upper == 0:
        raise ValueError(f"{name}: no response on the "
                         f"{'lower' if n_lower == 0 else 'upper'} boundary; the quantile "
                         "statistics need RTs on both")
    pos = np.diff(np.concatenate(([0.], q, [1.])))
    neg = pos[::-1]
    q_lower = np.asarray(mquantiles(-rt[rt < 0], q))
    q_upper = np.asarray(mquantiles(rt[rt > 0], q))
    emp_rt = np.concatenate((-q_lower[::-1], [0.], q_upper))
    freq_obs = np.concatenate((n_lower * neg, n_upper * pos))
    return {"n_samples": rt.size, "emp_rt": emp_rt, "freq_obs": freq_obs, "q_lower": q_lower,
            "q_upper": q_upper, "p_upper": float(np.mean(rt > 0))}


def pool_stats(stats):
    """The average model's statistics over the nodes of one condition tag
    (base.py:97-104): trial and bin counts summed, edges and p_upper averaged."""
    stats = list(stats)
    if not stats:
        raise ValueError("pool_stats: no statistics to pool")
    emp_rt = np.mean(np.array([s["emp_rt"] for s in stats]), 0)
    nq = (emp_rt.size - 1) // 2
    return {"n_samples": sum(s["n_samples"] for s in stats),
            "freq_obs": sum(np.array([s["freq_obs"] for s in stats]), 0),
            "emp_rt": emp_rt, "q_lower": -emp_rt[:nq][::-1], "q_upper": emp_rt[nq + 1:],
            "p_upper": float(np.mean([s["p_upper"] for s in stats]))}


def reduce_stats(cdf, freq_obs, n_samples):
    """(chisq, gsq) of one row from its CDF values at the edges, the bin counts
    and the trial count, in the order the kernel adds them (likelihoods.py:
    205-213, 239; chisq: the Pearson sum, see the module docstring)."""
    theo = np.concatenate(([0.], np.asarray(cdf, dtype=np.float64), [1.]))
    chisq = gs = 0.0
    for k in range(theo.size - 1):
        p = theo[k + 1] - theo[k]
        if p <= PROPORTION_FLOOR:
            p = PROPORTION_FLOOR
        f = float(freq_obs[k])
        ex = p * float(n_samples)
        chisq += ((f - ex) * (f - ex)) / ex
        gs += f * np.log(p)
    return chisq, 2 * gs
