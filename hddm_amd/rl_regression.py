"""HDDMrlRegressor on one MI355X: the RL-DDM with trial-wise regressed parameters.

The reference's HDDMrlRegressor (hddm/models/hddm_rl_regression.py) is
HDDMRegressor over the RL likelihood: per subject node it forms the regressed
outcomes in pandas, the learning rate's unbounded `alpha` among them, and calls
wfpt.wiener_like_multi_rlddm (hddm_rl_regression.py:25-38; wfpt.pyx:277-320)
with a fresh Q pair. Here the design matrix, responses, feedback and the
segment layout are resident (wfpt.RLRegDataset), and every evaluation is ONE
`wiener_like_rl_reg_groups` call that returns a sum per (subject x condition)
node, so the coefficient machinery and block slice updates are HDDMRegressor's
(regression.py).

* outcomes: v (the drift scaling), a, t and alpha.
* alpha, when not regressed, is a subject-level family with the prior of
  hddm_rl_regression.py:231-235 (RL_REG_MODEL below): group mean Normal(0,
  sd 50), std HalfNormal(10), start 0; slice widths as HDDMrl's. A regressed
  alpha's intercept takes that prior; every other coefficient is handled as in
  HDDMRegressor.
* segments: as in the reference, Q restarts at every adjacent change of
  split_by in frame order within a node. A node whose split_by value comes back
  after another one is almost always unsorted data: the class warns once per
  construction.
* a regressed alpha's learning rate is formed on the device with a correctly
  rounded power and may differ from the reference's libm value by one ulp of
  the power in a small share of trials.
"""
import time
import warnings

import numpy as np

from . import wfpt as _wfpt
from .hierarchical import MODEL, Family, _refuses, slice_widths
from .regression import HDDMRegressor
from .rl import RL_MODEL

# hddm_rl_regression.py:231-235 (value=0, g_tau=50**-2, std_std=10; the std
# node starts at 0.1 as every family's); slice widths: HDDMrl's (rl.py)
RL_REG_MODEL = {**MODEL, "alpha": Family(("normal", 0.0, 50.0), "normal", 10.0, (0.0, 0.0, 0.1),
                                         None, RL_MODEL["alpha"].widths)}
_POINTWISE = ("HDDMrlRegressor: model comparison needs a pointwise entry of the RL regression "
              "likelihood, which is not implemented")
_POST_PRED = ("HDDMrlRegressor: the posterior predictive of an RL regression model (a closed "
              "loop at trial-wise parameters) is not implemented")


class HDDMrlRegressor(HDDMRegressor):
    """HDDMrlRegressor(data, 'alpha ~ 1 + block').sample(n) on one MI355X.

    data: DataFrame with columns rt, response (1 upper / 0 lower), feedback,
    split_by, subj_idx, optionally q_init (a node's q is its first row's, 0.5
    without the column) and the covariates. models as HDDMRegressor's, with
    outcomes v, a, t and alpha.
    """

    MODEL, SLICE_WIDTHS = RL_REG_MODEL, slice_widths(RL_REG_MODEL)
    OUTCOMES, ALL_FAMILIES = ("v", "a", "t", "alpha"), ("a", "v", "t", "alpha")

    def __init__(self, data, models, group_only_regressors=True, include=(), p_outlier=0.05,
                 wiener_params=None, seed=None, device=None, depends_on=None):
        for col in ("response", "feedback", "split_by"):
            if col not in data:
                raise KeyError(f"HDDMrlRegressor: the data need a {col!r} column")
        super().__init__(data, models, group_only_regressors=group_only_regressors,
                         include=include, p_outlier=p_outlier, wiener_params=wiener_params,
                         seed=seed, device=device, depends_on=depends_on)

    def _make_dataset(self, rt, node_codes, device):
        data = self.data
        first = np.unique(node_codes, return_index=True)[1]  # each node's first row
        q_init = data["q_init"].to_numpy(dtype=np.float64) if "q_init" in data \
            else np.full(rt.size, 0.5)
        self.node_q = q_init[first]
        split = data["split_by"].to_numpy().astype(np.int64)
        _warn_if_unsorted(node_codes, split)
        return _wfpt.RLRegDataset(rt, data["response"].to_numpy().astype(np.int64),
                                  data["feedback"].to_numpy(dtype=np.float64), split, self.design,
                                  group_id=node_codes, n_groups=self.n_nodes, device=device)

    def alpha_rows(self, over=None):
        """(n_nodes,) unbounded alpha of each node; unused (0) when alpha is
        regressed."""
        if "alpha" not in self.FAMILIES:
            return np.zeros(self.n_nodes)
        val = over["alpha"] if over and "alpha" in over else self.subj["alpha"]
        return np.asarray(val, dtype=np.float64)[self.node_unit["alpha"]]

    def node_logp(self, over=None):
        """One wiener_like_rl_reg_groups call: the (n_nodes,) sums. Keys of
        `over` that name coefficients go to the coefficient table, `alpha` to
        the learning-rate rows, the others to the parameter table."""
        over = over or {}
        t0 = time.perf_counter()
        out = self.dataset.wiener_like_rl_reg_groups(
            self.reg_model, self.coef_table(over), self.node_q, self.alpha_rows(over),
            self.node_table(over), **self.wp)
        self._count_call(time.perf_counter() - t0, ",".join(sorted(over)) if over else "-")
        return out

    pointwise_loglik = dic_info = dic = waic = _refuses(_POINTWISE)
    post_pred_rows = post_pred_gen = post_pred_stats = _refuses(_POST_PRED)
    optimize = quantile_objective = _refuses(
        "HDDMrlRegressor: point fits are not implemented")


def _warn_if_unsorted(node_codes, split_by):
    """UserWarning when a node has a split_by value in two separate runs of the
    frame's order: each run restarts Q (wfpt.pyx:300-318)."""
    order = np.argsort(node_codes, kind="stable")
    node, split = np.asarray(node_codes)[order], split_by[order]
    if node.size == 0:
        return
    start = np.r_[True, (node[1:] != node[:-1]) | (split[1:] != split[:-1])]
    runs = np.stack([node[start], split[start]], axis=1)
    n_pairs = np.unique(runs, axis=0).shape[0]
    if n_pairs < runs.shape[0]:
        warnings.warn(
            f"HDDMrlRegressor: {runs.shape[0] - n_pairs} split_by run(s) repeat a value already "
            "seen in the same subject node. As in the reference, Q restarts at every adjacent "
            "change of split_by in the frame's order, so a condition whose trials are not "
            "contiguous is learned from scratch in each run; sort the data by subject and "
            "split_by if that is not intended.", UserWarning, stacklevel=4)
