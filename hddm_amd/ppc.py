"""Posterior predictive checks (hddm/utils.py:241-299) on the MI355X.

`gen_ppc_stats` is the reference's table of summary statistics as NumPy
callables (the CPU restatement the tests hold the device against);
`post_pred_stats` is the drop-in for `hddm.utils.post_pred_stats`, reducing
every simulated data set in one `wfpt.rt_stats_rows` call; `summarize`
compares the observed statistics with the sampled ones. Plots stay out of
scope.
"""
import warnings
from collections import OrderedDict

import numpy as np

from . import wfpt as _wfpt

PPC_QUANTILES = _wfpt.PPC_QUANTILES


def scoreatpercentile(s, q):
    """scipy.stats.scoreatpercentile(s, q) (interpolation 'fraction') restated
    operation for operation (_compute_qth_percentile); s need not be sorted."""
    s = np.sort(np.asarray(s, dtype=np.float64))
    idx = q / 100. * (s.shape[0] - 1)
    i = int(idx)
    if i == idx:
        return s[i]
    w0, w1 = (i + 1) - idx, idx - i
    return (s[i] * w0 + s[i + 1] * w1) / (w0 + w1)


def gen_ppc_stats(quantiles=PPC_QUANTILES):
    """hddm.utils.gen_ppc_stats (utils.py:241-267): an OrderedDict of statistic
    name -> function of one node's signed RTs. An empty boundary's mean and std
    are NaN (NumPy warns about the empty slice, as it does in the reference)."""
    stats = OrderedDict()
    stats["accuracy"] = lambda x: np.mean(x > 0)
    stats["mean_ub"] = lambda x: np.mean(x[x > 0])
    stats["std_ub"] = lambda x: np.std(x[x > 0])
    for q in quantiles:
        stats[str(q) + "q_ub"] = (
            lambda x, q=q: scoreatpercentile(x[x > 0], q) if np.any(x > 0) else np.nan)
    stats["mean_lb"] = lambda x: np.mean(x[x < 0])
    stats["std_lb"] = lambda x: np.std(x[x < 0])
    for q in quantiles:
        stats[str(q) + "q_lb"] = (
            lambda x, q=q: scoreatpercentile(np.abs(x[x < 0]), q) if np.any(x < 0) else np.nan)
    return stats


def _signed_rt(frame):
    """flip_errors (utils.py:15-37): rt negated where response == 0, unless the
    RTs are signed already."""
    rt = np.asarray(frame["rt"], dtype=np.float64)
    if "response" in frame and not np.any(rt < 0):
        rt = np.where(np.asarray(frame["response"]) == 0, -np.abs(rt), np.abs(rt))
    return rt


def _column(frame, name):
    if name in frame:
        return np.asarray(frame[name])
    if name in (frame.index.names or ()):
        return np.asarray(frame.index.get_level_values(name))
    return None


def _grouped_stats(rt, codes, n_groups, quantiles):
    """rt_stats_rows over the groups 0 .. n_groups of `codes`, each group's
    values in their order of appearance."""
    order = np.argsort(codes, kind="stable")
    offsets = np.zeros(n_groups + 1, dtype=np.int64)
    np.cumsum(np.bincount(codes, minlength=n_groups), out=offsets[1:])
    return _wfpt.rt_stats_rows(rt[order], offsets, quantiles)


def summarize(observed, sampled, names=None, nodes=None):
    """Compare each node's observed statistics (n_nodes, K) with the sampled
    ones (S, n_nodes, K). kabuki.analyze.post_pred_stats, which the reference
    delegates this to (utils.py:299), is not part of the reference tree, so the
    columns are defined here and not pinned to it. Returns a DataFrame indexed
    by (node, stat) with

      observed     the observed statistic
      mean, std    over the sweeps, ignoring NaN (std with ddof=0)
      SEM          (observed - mean)^2
      MSE          mean((sampled - observed)^2) over the sweeps, ignoring NaN
      credible     observed lies inside the sweeps' 2.5 .. 97.5 percentile interval
      quantile     percent of the sweeps' (non-NaN) values <= observed
      mahalanobis  |observed - mean| / std

    A statistic that is NaN in every sweep (a boundary never reached) or whose
    observed value is NaN gives NaN (credible: False). names: the K statistic
    names (default rt_stats_names() when K matches it); nodes: the node labels
    (default 0 .. n_nodes)."""
    import pandas as pd
    obs = np.asarray(observed, dtype=np.float64)
    sam = np.asarray(sampled, dtype=np.float64)
    if obs.ndim != 2 or sam.ndim != 3 or sam.shape[1:] != obs.shape or sam.shape[0] < 1:
        raise ValueError("observed must be (n_nodes, K) and sampled (S, n_nodes, K), S >= 1")
    n_nodes, K = obs.shape
    if names is None:
        names = _wfpt.rt_stats_names()
        if len(names) != K:
            raise ValueError(f"names is needed: K = {K}, the default statistics are {len(names)}")
    if len(names) != K:
        raise ValueError(f"names must hold K = {K} entries")
    nodes = list(range(n_nodes)) if nodes is None else list(nodes)
    if len(nodes) != n_nodes:
        raise ValueError(f"nodes must hold n_nodes = {n_nodes} entries")
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)  # all-NaN slices
        mean, std = np.nanmean(sam, axis=0), np.nanstd(sam, axis=0)
        mse = np.nanmean((sam - obs) ** 2, axis=0)
        lo, hi = np.nanpercentile(sam, [2.5, 97.5], axis=0)
        valid = np.sum(~np.isnan(sam), axis=0)
        quantile = 100. * np.sum(sam <= obs, axis=0) / valid
        quantile = np.where(np.isnan(obs) | (valid == 0), np.nan, quantile)
        cols = OrderedDict([
            ("observed", obs), ("mean", mean), ("std", std), ("SEM", (obs - mean) ** 2),
            ("MSE", mse), ("credible", (obs >= lo) & (obs <= hi)), ("quantile", quantile),
            ("mahalanobis", np.abs(obs - mean) / std)])
    index = pd.MultiIndex.from_product([nodes, list(names)], names=["node", "stat"])
    return pd.DataFrame({k: v.reshape(-1) for k, v in cols.items()}, index=index)


def post_pred_stats(data, sim_datasets, quantiles=PPC_QUANTILES, return_sampled=False):
    """hddm.utils.post_pred_stats (utils.py:270-299) with gen_ppc_stats' default
    statistics: both frames' RTs are signed by response (flip_errors), every
    simulated data set and every observed node is reduced by ONE
    wfpt.rt_stats_rows call each, and summarize() compares them.

    data: the observed trials, columns rt[, response] and optionally node (one
    node when absent). sim_datasets: the frame HDDM.post_pred_gen returns,
    columns (or index levels) sample, node, rt[, response]; the node labels are
    those of `data`. return_sampled=True also returns the sampled statistics
    (S, n_nodes, K), the samples in rising order of their label."""
    obs_node = _column(data, "node")
    obs_rt = _signed_rt(data)
    if obs_node is None:
        obs_node = np.zeros(obs_rt.size, dtype=np.int64)
    labels, obs_codes = np.unique(obs_node, return_inverse=True)
    sim_node, sim_sample = _column(sim_datasets, "node"), _column(sim_datasets, "sample")
    sim_rt = _signed_rt(sim_datasets)
    if sim_node is None:
        sim_node = np.full(sim_rt.size, labels[0])
    if sim_sample is None:
        sim_sample = np.zeros(sim_rt.size, dtype=np.int64)
    node_codes = np.searchsorted(labels, sim_node)
    if np.any(node_codes >= labels.size) or np.any(labels[np.minimum(node_codes, labels.size - 1)]
                                                   != sim_node):
        raise ValueError("sim_datasets names a node that data does not have")
    samples, sample_codes = np.unique(sim_sample, return_inverse=True)
    n_nodes, S = labels.size, samples.size
    observed = _grouped_stats(obs_rt, obs_codes, n_nodes, quantiles)
    sampled = _grouped_stats(sim_rt, sample_codes * n_nodes + node_codes, S * n_nodes, quantiles)
    sampled = sampled.reshape(S, n_nodes, -1)
    table = summarize(observed, sampled, _wfpt.rt_stats_names(quantiles), labels.tolist())
    return (table, sampled) if return_sampled else table
