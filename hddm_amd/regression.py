"""HDDMRegressor on one MI355X: trial-wise parameters link(design . coefficients).

The reference's HDDMRegressor (hddm/models/hddm_regression.py) builds a patsy
design matrix per regressed outcome, multiplies it by the coefficient nodes
in pandas on every likelihood evaluation and hands the trial-wise arrays to
wfpt.wiener_like_multi (hddm_regression.py:26-36). Here the design matrix is
resident (wfpt.RegDataset), the predictor runs on the device, and every
evaluation is ONE `wiener_like_reg_groups` call that returns a sum per
(subject x condition) node, so subject-level coefficients take the same block
slice update over subjects as HDDM's subject nodes (hierarchical.py).

* design_matrix: the subset of patsy's formula language the reference's
  docstring examples use (`1`, `0`, numeric columns, `C(name)`, joined by
  `+`); anything else goes to patsy when it is installed.
* priors (hddm_regression.py:250-284): a coefficient whose name contains
  `Intercept` (or, without an intercept, every plain `C(...)` column) takes
  the outcome's own prior (hierarchical.py's header); every other coefficient
  Normal(0, sd 15). With group_only_regressors=False every coefficient also
  has subject nodes: the intercept in the outcome's family, the others
  Normal(g, std) with std ~ Uniform(1e-10, 100) (base.py:310-369).
* slice width 0.05 for every coefficient node (hddm_regression.py:284).
* links run on the device and are named: identity, exp, invlogit.
"""
import functools
import re
import time

import numpy as np

from . import wfpt as _wfpt
from .hierarchical import (HDDM, INTER, LOGPDF, SLICE_WIDTHS, _refuses, halfnormal_logpdf, logpdf,
                           normal_logpdf, slice_step)

LINKS = ("identity", "exp", "invlogit")
COEF_SLICE_WIDTH = 0.05  # hddm_regression.py:284
_NAME = r"[A-Za-z_][A-Za-z_0-9.]*"


# ---------------------------------------------------------------- design matrix

def _patsy_or_raise(formula_rhs, data, term):
    try:
        import patsy
    except ImportError:
        raise NotImplementedError(
            f"design_matrix: term {term!r} needs patsy, which is not installed; without it "
            "only `1`, `0`, numeric columns and C(name) joined by `+` are supported")
    return patsy.dmatrix(formula_rhs, data, return_type="dataframe")


def design_matrix(formula_rhs, data):
    """The design matrix of `formula_rhs` over DataFrame `data` as a float64
    DataFrame with patsy's column names and column order: `Intercept` (implicit
    unless `0` is given), then the `C(name)` terms in formula order (treatment
    coding over the sorted levels, `C(name)[T.level]`; the first one full-coded
    as `C(name)[level]` when there is no intercept), then the numeric columns
    in formula order."""
    import pandas as pd
    terms = [t.strip() for t in formula_rhs.split("+")]
    intercept = True
    cats, nums = [], []
    for t in terms:
        if t == "1":
            intercept = True
        elif t in ("0", "-1"):
            intercept = False
        elif re.fullmatch(rf"C\(\s*({_NAME})\s*\)", t):
            name = re.fullmatch(rf"C\(\s*({_NAME})\s*\)", t).group(1)
            if name not in cats:
                cats.append(name)
        elif re.fullmatch(_NAME, t):
            if t not in nums:
                nums.append(t)
        else:
            return _patsy_or_raise(formula_rhs, data, t)
    for name in cats + nums:
        if name not in data:
            raise KeyError(f"design_matrix: no column {name!r} in the data")
    n = len(data)
    cols = {}
    if intercept:
        cols["Intercept"] = np.ones(n)
    for k, name in enumerate(cats):
        val = data[name].to_numpy()
        levels = sorted(pd.unique(val))
        full = k == 0 and not intercept
        for lv in (levels if full else levels[1:]):
            cols[f"C({name})[{lv}]" if full else f"C({name})[T.{lv}]"] = (val == lv).astype(
                np.float64)
    for name in nums:
        cols[name] = data[name].to_numpy(dtype=np.float64)
    return pd.DataFrame(cols, index=data.index, dtype=np.float64)


# ---------------------------------------------------------------- the model

def _parse_models(models, cls="HDDMRegressor", outcomes=("v", "a", "t")):
    """The model descriptors of a regressor class `cls` whose likelihood takes
    `outcomes` as trial-wise parameters (rl_regression.py adds alpha)."""
    if isinstance(models, (str, dict)):
        models = [models]
    out = []
    for m in models:
        if isinstance(m, str):
            m = {"model": m}
        link = m.get("link_func", "identity")
        if callable(link):
            raise TypeError(f"{cls}: the link runs on the device, so link_func is a "
                            f"name, one of {LINKS}, not a Python callable")
        if link not in LINKS:
            raise ValueError(f"{cls}: unknown link_func {link!r}; expected one of {LINKS}")
        if "~" not in m["model"]:
            raise ValueError(f"{cls}: model {m['model']!r} is not 'outcome ~ terms'")
        outcome, rhs = (s.strip() for s in m["model"].split("~", 1))
        if outcome not in outcomes:
            raise NotImplementedError(f"{cls}: outcome {outcome!r} is not supported at model "
                                      f"level ({', '.join(outcomes)})")
        if any(d["outcome"] == outcome for d in out):
            raise ValueError(f"{cls}: outcome {outcome!r} has two models")
        out.append({"outcome": outcome, "rhs": rhs, "link": link})
    return out


def _drift_only(method):
    if method != "drift":
        raise ValueError("HDDMRegressor's posterior predictive simulates every trial as a "
                         "diffusion path (method='drift'); a per-trial CDF grid is not offered")


def _needs_trial_sampler(fn):
    """The posterior predictive runs on the model's resident data set. A model
    whose data set does not offer the trial-wise sampler (a host stand-in of
    wfpt.RegDataset, or no data set at all) refuses before its arguments are
    looked at, as the subclasses' other unsupported methods do."""
    @functools.wraps(fn)
    def method(self, *args, **kw):
        if not hasattr(getattr(self, "dataset", None), "gen_rts_drift"):
            raise NotImplementedError(
                "the regressor's posterior predictive needs a data set with the on-device "
                "trial-wise sampler (wfpt.RegDataset.gen_rts_drift)")
        return fn(self, *args, **kw)
    return method


class HDDMRegressor(HDDM):
    """HDDMRegressor(data, 'v ~ BOLD').sample(n) on one MI355X.

    models: 'v ~ 1 + BOLD', {'model': ..., 'link_func': 'identity' | 'exp' |
    'invlogit'}, or a list of these; outcomes v, a, t. Coefficients are named
    `{outcome}_{design column}`. The non-regressed families stay as in HDDM.
    """

    # the outcomes a model may name and the families of the model without any
    # regression, in HDDM's order (rl_regression.py adds alpha to both)
    OUTCOMES, ALL_FAMILIES = ("v", "a", "t"), ("a", "v", "t")

    def __init__(self, data, models, group_only_regressors=True, include=(), p_outlier=0.05,
                 wiener_params=None, seed=None, device=None, depends_on=None):
        import pandas as pd
        cls = type(self).__name__
        self.model_descrs = _parse_models(models, cls, self.OUTCOMES)
        self.reg_outcomes = [d["outcome"] for d in self.model_descrs]
        for k in (depends_on or {}):
            if k in self.reg_outcomes:  # hddm_regression.py:214-216
                raise ValueError(f"{cls}: '{k}' is a regression outcome and cannot be "
                                 "used in depends_on")
        self.group_only_regressors = bool(group_only_regressors)
        self.FAMILIES = tuple(f for f in self.ALL_FAMILIES if f not in self.reg_outcomes)
        frame = pd.DataFrame(data).reset_index(drop=True)
        mats, col0 = [], 0
        self.coef_names, self.coef_outcome, self.coef_intercept = [], [], []
        self.reg_model = []  # RegDataset's (param, col0, ncol, link) terms
        for d in self.model_descrs:
            X = design_matrix(d["rhs"], frame)
            names = [f"{d['outcome']}_{c}" for c in X.columns]
            inter = ["Intercept" in nm for nm in names]
            if not any(inter):  # 0 + C(...): every condition is an intercept (:257-260)
                inter = ["C(" in nm and ":" not in nm for nm in names]
            d["params"] = names
            self.coef_names += names
            self.coef_outcome += [d["outcome"]] * len(names)
            self.coef_intercept += inter
            self.reg_model.append((d["outcome"], col0, X.shape[1], d["link"]))
            col0 += X.shape[1]
            mats.append(X.to_numpy(dtype=np.float64))
        self.design = np.ascontiguousarray(np.hstack(mats))
        self.n_coef = col0
        super().__init__(frame, depends_on=depends_on, include=include, p_outlier=p_outlier,
                         wiener_params=wiener_params, seed=seed, device=device,
                         paired_probes=False)

    def _make_dataset(self, rt, node_codes, device):
        return _wfpt.RegDataset(rt, self.design, group_id=node_codes, n_groups=self.n_nodes,
                                device=device)

    # -- state ---------------------------------------------------------------
    def _init_values(self):
        """HDDM's starting values (hddm_info.py:121-140) for the non-regressed
        families; an intercept starts where its outcome would, every other
        coefficient at 0."""
        super()._init_values()
        self.coef, self.coef_std, self.coef_subj = {}, {}, {}
        for nm, out, inter in zip(self.coef_names, self.coef_outcome, self.coef_intercept):
            g0, s0 = self.MODEL[out].start[:2] if inter else (0.0, 0.0)
            if self.group_only_regressors:
                # the group node feeds the likelihood directly: start where a
                # subject node would (t below every RT)
                self.coef[nm] = s0
            else:
                self.coef[nm] = g0
                self.coef_std[nm] = 0.1
                self.coef_subj[nm] = np.full(self.n_subj, s0)

    def coef_table(self, over=None):
        """(n_nodes, C) coefficient rows: a group-only coefficient in every
        row, a subject-level one through the node's subject. `over` replaces
        named coefficients (a scalar, or one value per subject)."""
        B = np.empty((self.n_nodes, self.n_coef))
        for j, nm in enumerate(self.coef_names):
            val = over[nm] if over and nm in over else (
                self.coef[nm] if self.group_only_regressors else self.coef_subj[nm])
            B[:, j] = val if np.ndim(val) == 0 else np.asarray(val)[self.node_subj]
        return B

    def node_table(self, over=None):
        """(n_nodes, 8) parameter table as HDDM.node_table; a regressed
        outcome's column is unused by the likelihood (0)."""
        over = over or {}
        return self._table_of((), {fam: over.get(fam, self.subj[fam]) for fam in self.FAMILIES},
                              {name: over.get(name, self.inter[name]) for name in INTER})

    def node_logp(self, over=None):
        """One wiener_like_reg_groups call: the (n_nodes,) sums. Keys of `over`
        that name coefficients go to the coefficient table, the others to the
        parameter table."""
        over = over or {}
        t0 = time.perf_counter()
        out = self.dataset.wiener_like_reg_groups(self.reg_model, self.coef_table(over),
                                                  self.node_table(over), **self.wp)
        self._count_call(time.perf_counter() - t0, ",".join(sorted(over)) if over else "-")
        return out

    # -- priors --------------------------------------------------------------
    def _coef_group_prior(self, nm, x):
        j = self.coef_names.index(nm)
        if self.coef_intercept[j]:
            return self._group_prior(self.coef_outcome[j], x)
        return normal_logpdf(x, 0.0, 15.0)

    def _coef_subj_prior(self, nm, x, g=None, std=None):
        j = self.coef_names.index(nm)
        g = float(self.coef[nm] if g is None else g)
        std = float(self.coef_std[nm] if std is None else std)
        kind = self.MODEL[self.coef_outcome[j]].subject if self.coef_intercept[j] else "normal"
        return LOGPDF[kind](x, g, std)

    def _coef_std_prior(self, nm, s):
        j = self.coef_names.index(nm)
        if self.coef_intercept[j]:
            return float(halfnormal_logpdf(s, self.MODEL[self.coef_outcome[j]].std_sd))
        return -np.log(100.0 - 1e-10) if 1e-10 <= s <= 100.0 else -np.inf

    def _coef_lower(self, nm):
        j = self.coef_names.index(nm)
        return self.MODEL[self.coef_outcome[j]].lower if self.coef_intercept[j] else None

    def logp(self):
        """Joint log density of the model at the current values."""
        lp = float(np.sum(self.node_logp()))
        for fam in self.FAMILIES:
            lp += float(np.sum(self.subj_prior(fam, self.subj[fam])))
            lp += float(np.sum(self._group_prior(fam, self.group[fam])))
            lp += float(halfnormal_logpdf(self.std[fam], self.MODEL[fam].std_sd))
        for nm in self.coef_names:
            lp += float(self._coef_group_prior(nm, self.coef[nm]))
            if not self.group_only_regressors:
                lp += float(np.sum(self._coef_subj_prior(nm, self.coef_subj[nm])))
                lp += self._coef_std_prior(nm, self.coef_std[nm])
        for name in self.inter_names:
            lp += float(logpdf(INTER[name].prior, self.inter[name]))
        return lp

    # -- updates -------------------------------------------------------------
    def _update_coef_group_only(self, nm):
        def logp(x):
            val = float(x[0])
            pr = float(self._coef_group_prior(nm, val))
            if not np.isfinite(pr):
                return np.array([-np.inf])
            return np.array([pr + float(np.sum(self.node_logp({nm: val})))])

        new, _ = slice_step(np.array([self.coef[nm]]), logp, COEF_SLICE_WIDTH, self.rng,
                            lower=self._coef_lower(nm))
        self.coef[nm] = float(new[0])

    def _update_coef_subject(self, nm):
        """All subjects' nodes of one coefficient in one block slice step from
        the per-node sums, like HDDM._update_subject."""
        def logp(x):
            ll = np.bincount(self.node_subj, weights=self.node_logp({nm: x}),
                             minlength=self.n_subj)
            return ll + self._coef_subj_prior(nm, x)

        self.coef_subj[nm], _ = slice_step(self.coef_subj[nm], logp, COEF_SLICE_WIDTH, self.rng,
                                           lower=self._coef_lower(nm))

    def _update_coef_group(self, nm):
        x = self.coef_subj[nm]

        def logp(g):
            val = float(g[0])
            pr = float(self._coef_group_prior(nm, val))
            if not np.isfinite(pr):
                return np.array([-np.inf])
            return np.array([pr + float(np.sum(self._coef_subj_prior(nm, x, g=val)))])

        new, _ = slice_step(np.array([self.coef[nm]]), logp, COEF_SLICE_WIDTH, self.rng,
                            lower=self._coef_lower(nm))
        self.coef[nm] = float(new[0])

        def logp_std(s):
            val = float(s[0])
            pr = self._coef_std_prior(nm, val) if val > 0 else -np.inf
            if not np.isfinite(pr):
                return np.array([-np.inf])
            return np.array([pr + float(np.sum(self._coef_subj_prior(nm, x, std=val)))])

        new, _ = slice_step(np.array([self.coef_std[nm]]), logp_std, SLICE_WIDTHS["v_std"],
                            self.rng, lower=0.0)
        self.coef_std[nm] = float(new[0])

    def sweep(self):
        """One MCMC iteration: every stochastic updated once."""
        for fam in self.FAMILIES:
            self._update_group(fam)
            self._update_subject(fam)
        for nm in self.coef_names:
            if self.group_only_regressors:
                self._update_coef_group_only(nm)
            else:
                self._update_coef_group(nm)
                self._update_coef_subject(nm)
        for name in self.inter_names:
            self._update_inter(name)

    def _record(self, nodes):
        """HDDM._record, so that sample() returns traces of the group-level
        nodes (dict name -> array): HDDM's names for the non-regressed
        families, then the coefficient names, each followed by its
        `{coefficient}_std` with subject-level coefficients, then sv / sz / st."""
        group, subj = super()._record(nodes)
        inter = {name: group.pop(name) for name in self.inter_names}
        for nm in self.coef_names:
            group[nm] = self.coef[nm]
            if not self.group_only_regressors:
                group[f"{nm}_std"] = self.coef_std[nm]
                subj[nm] = self.coef_subj[nm].copy()
        group.update(inter)
        return group, subj

    # -- model comparison ------------------------------------------------------
    def _pw_coef_table(self, picked, mean=False):
        """coef_table for the picked sweeps, (S, n_nodes, C), or at the mean
        over them of every coefficient."""
        B = np.empty((() if mean else (picked.size,)) + (self.n_nodes, self.n_coef))
        for j, nm in enumerate(self.coef_names):
            if self.group_only_regressors:
                val = self.trace[nm][picked]
                B[..., j] = float(np.mean(val)) if mean else val[:, None]
            else:
                val = self.trace_subj[nm][picked]
                B[..., j] = (val.mean(axis=0) if mean else val)[..., self.node_subj]
        return B

    def _pw_score(self, picked):
        return self.dataset.pointwise_reg_groups(self.reg_model, self._pw_coef_table(picked),
                                                 self._pw_ddm_table(picked), **self.wp)

    def _pw_mean_logp(self, picked):
        return self.dataset.wiener_like_reg_groups(
            self.reg_model, self._pw_coef_table(picked, mean=True),
            self._pw_ddm_table(picked, mean=True), **self.wp)

    # -- posterior predictive --------------------------------------------------
    @_needs_trial_sampler
    def post_pred_rows(self, samples=500):
        """The kept sweeps a posterior predictive draws from and their node
        rows: (picked, coef_tables (S, n_nodes, C), param_tables (S, n_nodes,
        8)), `picked` by HDDM.post_pred_rows' rule (evenly spaced kept sweeps).
        A group-only coefficient comes from its trace, a subject-level one
        from the subject traces through the node's subject."""
        if not isinstance(getattr(self, "trace", None), dict) \
                or not isinstance(getattr(self, "trace_subj", None), dict):
            raise RuntimeError("post_pred_gen needs the traces: run sample() first")
        picked = self._picked_sweeps(samples, len(self.trace[self.coef_names[0]]))
        B = np.empty((picked.size, self.n_nodes, self.n_coef))
        for j, nm in enumerate(self.coef_names):
            B[:, :, j] = self.trace[nm][picked][:, None] if self.group_only_regressors \
                else self.trace_subj[nm][picked][:, self.node_subj]
        subj = {fam: self.trace_subj[fam][picked] for fam in self.FAMILIES}
        inter = {name: self.trace[name][picked][:, None] if name in self.include
                 else self.inter[name] for name in INTER}
        return picked, B, self._table_of((picked.size,), subj, inter)

    @_needs_trial_sampler
    def post_pred_gen(self, samples=500, seed=None, dt=1e-4, method="drift"):
        """Posterior predictive data (kabuki.analyze.post_pred_gen over
        wfpt_reg_like's random(), hddm_regression.py:39-56): for each of
        `samples` evenly spaced kept sweeps, one RT per trial of the data,
        simulated as a diffusion path with time step dt at the trial's own
        regressed parameters by ONE RegDataset.gen_rts_drift call (the
        parameters are formed on the device; the reference loops over trials
        and needs keep_regressor_trace=True). The draws come from the DDM
        alone: p_outlier's mixture is not simulated.

        Returns a DataFrame with columns sample (index of the kept sweep), node
        (index into node_keys), trial (row of the model's data frame), rt
        (signed) and response (1 upper / 0 lower)."""
        import pandas as pd
        _drift_only(method)
        picked, B, P = self.post_pred_rows(samples)
        if seed is None:
            seed = int(self.rng.integers(0, 2 ** 63))
        rts = self.dataset.gen_rts_drift(self.reg_model, B, P, dt=dt, seed=seed).ravel()
        n = self.n_trials
        return pd.DataFrame({"sample": np.repeat(picked, n),
                             "node": np.tile(self.node_codes, picked.size),
                             "trial": np.tile(np.arange(n), picked.size),
                             "rt": rts, "response": (rts > 0).astype(np.int64)})

    @_needs_trial_sampler
    def post_pred_stats(self, samples=500, seed=None, dt=1e-4, method="drift",
                        quantiles=(10, 30, 50, 70, 90), return_sampled=False):
        """The posterior predictive check as HDDM.post_pred_stats:
        post_pred_gen's draws (same arguments, same seed: the same draws)
        reduced to gen_ppc_stats' statistics per (sweep, node) on the device by
        ONE RegDataset.gen_rts_drift_stats call (no draw is copied to the
        host), the observed nodes by one wfpt.rt_stats_rows call, and
        ppc.summarize compares the two. p_outlier's mixture is not simulated.

        Returns ppc.summarize's DataFrame indexed by (node, stat); with
        return_sampled=True also the sampled statistics (len(picked), n_nodes,
        K) in wfpt.rt_stats_names' order."""
        from . import ppc
        _drift_only(method)
        picked, B, P = self.post_pred_rows(samples)
        if seed is None:
            seed = int(self.rng.integers(0, 2 ** 63))
        sampled = self.dataset.gen_rts_drift_stats(self.reg_model, B, P, dt=dt, seed=seed,
                                                   quantiles=quantiles)
        table = ppc.summarize(self._observed_stats(quantiles), sampled,
                              _wfpt.rt_stats_names(quantiles))
        return (table, sampled) if return_sampled else table

    node_logp_multi = _refuses("HDDMRegressor scores one table per call")
    optimize = quantile_objective = _refuses("the regressor's point fits are not implemented")
