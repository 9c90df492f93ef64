"""HDDMrl on one MI355X: the hierarchical reinforcement-learning DDM.

The reference's HDDMrl (hddm/models/hddm_rl.py:16-73) is HDDM with a Q-learning
drift: within each `split_by` condition of a subject a pair of Q values is
updated trial by trial from the feedback, and trial i's drift is (q_up - q_low)
* v, so `v` is the drift scaling (hddm_rl.py:72). Its likelihood node calls
wiener_like_rlddm once per subject node. Here every slice evaluation is ONE
`RLDataset.wiener_like_rlddm_nodes` call over all nodes, and both stepping-out
probes of a slice step ONE `wiener_like_rlddm_nodes_multi` call with two
tables, each row bit for bit the one-table call's.

* model: HDDM's a, v, t families and sv / sz / st (hierarchical.py's header),
  plus the learning rate on the likelihood's unbounded scale
  (hddm_rl.py:41-42, base.py:310-369; RL_MODEL below):
    alpha_subj ~ Normal(alpha, alpha_std), alpha ~ Normal(0.2, sd 3),
    alpha_std ~ Uniform(1e-10, 10)
  and, with dual=True, an identical family pos_alpha for positive prediction
  errors; otherwise the likelihood gets pos_alpha = 100.0, "use alpha"
  (hddm_rl.py:52-53).
* step methods: the group mean of a learning-rate family is a Normal with
  Normal children and takes the conjugate update of `v`; the subject nodes are
  slice-sampled in one block over subjects (width 1.5, hddm_info.py:105); the
  std node is slice-sampled inside its Uniform support (width 1).
* a node's q is its first row's q_init (hddm_rl.py:69; default 0.5).

The posterior predictive of an RL model is a closed loop: every simulated
choice picks the reward that moves the Q values behind the next trial's drift.
`HDDMrl.post_pred_sim` / `post_pred_sim_stats` run it on the device, one lane
per (sweep, node, condition) sequence in ONE `wfpt.gen_rlddm_rows` launch
(DESIGN.md §22), given the reward schedule to run on, or one step ahead of the
observed choices (mode='onestep'). `gen_rl_data` below makes synthetic data by
the host-driven loop or, with closed_loop='device', by the same launch.
"""
import time

import numpy as np

from . import wfpt as _wfpt
from .hierarchical import HDDM, MODEL, Family, _refuses, slice_widths

RL_BASE = 2.718281828459  # the reference's literal (wfpt.pyx:123)
NO_POS_ALPHA = 100.0      # hddm_rl.py:52-53: the likelihood then uses alpha

# hddm_rl.py:41-45 (g_mu=0.2, g_tau=3**-2, std in [1e-10, 10], value 0, std
# value 0.1); slice widths hddm_info.py:105 (alpha) and :174 (the std default)
_LEARNING_RATE = Family(("normal", 0.2, 3.0), "normal", None, (0.0, 0.0, 0.1), None, (1.5, 1),
                        ("uniform", 1e-10, 10.0))
RL_MODEL = {**MODEL, "alpha": _LEARNING_RATE, "pos_alpha": _LEARNING_RATE}
_RL_COL = {"q": 0, "alpha": 1, "pos_alpha": 2}  # the columns of an RL row table


def learning_rate(alpha):
    """The rate of the unbounded `alpha` as the likelihood forms it
    (wfpt.pyx:123-125)."""
    e = RL_BASE ** float(alpha)
    return e / (1 + e)


class HDDMrl(HDDM):
    """HDDMrl(data).sample(n) on one MI355X.

    data: DataFrame with columns rt, response (1 upper / 0 lower), feedback,
    split_by (integer condition of the two-armed bandit: one Q pair each),
    subj_idx and optionally q_init. Nodes are subject x depends_on cells as in
    HDDM; split_by only sets the segments inside a node. depends_on may name
    alpha / pos_alpha like a, v, t.
    """

    MODEL, SLICE_WIDTHS = RL_MODEL, slice_widths(RL_MODEL)

    def __init__(self, data, depends_on=None, include=(), dual=False, p_outlier=0.05,
                 wiener_params=None, seed=None, device=None, paired_probes=True,
                 non_centered=False):
        if non_centered:
            raise NotImplementedError("HDDMrl: the non_centered parameterisation is not "
                                      "implemented")
        self.dual = bool(dual)
        self.rl_families = ("alpha", "pos_alpha") if self.dual else ("alpha",)
        self.FAMILIES = HDDM.FAMILIES + self.rl_families
        for col in ("response", "feedback", "split_by"):
            if col not in data:
                raise KeyError(f"HDDMrl: the data need a {col!r} column")
        super().__init__(data, depends_on=depends_on, include=include, p_outlier=p_outlier,
                         wiener_params=wiener_params, seed=seed, device=device,
                         paired_probes=paired_probes)

    def _make_dataset(self, rt, node_codes, device):
        data = self.data
        first = np.unique(node_codes, return_index=True)[1]  # each node's first row
        q_init = data["q_init"].to_numpy(dtype=np.float64) if "q_init" in data \
            else np.full(rt.size, 0.5)
        self.node_q = q_init[first]
        return _wfpt.RLDataset(rt, data["response"].to_numpy().astype(np.int64),
                               data["feedback"].to_numpy(dtype=np.float64),
                               data["split_by"].to_numpy().astype(np.int64),
                               node_id=node_codes, n_nodes=self.n_nodes, device=device)

    # -- likelihood ----------------------------------------------------------
    def rl_table(self, over=None):
        """(n_nodes, 3) rows of q, alpha, pos_alpha; `over` replaces the
        subject values of alpha / pos_alpha. pos_alpha is 100.0 without dual."""
        over = over or {}
        R = np.empty((self.n_nodes, 3))
        R[:, 0] = self.node_q
        R[:, 2] = NO_POS_ALPHA
        for fam in self.rl_families:
            val = over[fam] if fam in over else self.subj[fam]
            R[:, _RL_COL[fam]] = np.asarray(val)[self.node_unit[fam]]
        return R

    def _tables(self, over):
        over = over or {}
        ddm = {k: v for k, v in over.items() if k not in _RL_COL}
        return self.rl_table(over), self.node_table(ddm)

    def node_logp(self, over=None):
        """One wiener_like_rlddm_nodes call: the (n_nodes,) sums. Keys of `over`
        that name alpha / pos_alpha go to the RL rows, the others to the
        parameter table."""
        rows, table = self._tables(over)
        t0 = time.perf_counter()
        out = self.dataset.wiener_like_rlddm_nodes(rows, table, **self.wp)
        self._count_call(time.perf_counter() - t0, ",".join(sorted(over)) if over else "-")
        return out

    def node_logp_multi(self, overs):
        """node_logp for several overrides in ONE call (wiener_like_rlddm_nodes_multi):
        (len(overs), n_nodes), each row bit for bit the one-table call's."""
        pairs = [self._tables(o) for o in overs]
        t0 = time.perf_counter()
        out = self.dataset.wiener_like_rlddm_nodes_multi(np.stack([p[0] for p in pairs]),
                                                         np.stack([p[1] for p in pairs]),
                                                         **self.wp)
        self._count_call(time.perf_counter() - t0, ",".join(sorted(overs[0])) + f" x{len(overs)}")
        return out

    # -- model comparison ----------------------------------------------------
    def _pw_rl_table(self, picked, mean=False):
        """rl_table for the picked sweeps, (S, n_nodes, 3), or at the mean over
        them of alpha / pos_alpha on their sampled (unbounded) scale."""
        R = np.empty((() if mean else (picked.size,)) + (self.n_nodes, 3))
        R[..., 0] = self.node_q
        R[..., 2] = NO_POS_ALPHA
        for fam in self.rl_families:
            val = self.trace_subj[fam][picked]
            val = val.mean(axis=0) if mean else val
            R[..., _RL_COL[fam]] = val[..., self.node_unit[fam]]
        return R

    def _pw_score(self, picked):
        return self.dataset.pointwise_rlddm_nodes(self._pw_rl_table(picked),
                                                  self._pw_ddm_table(picked), **self.wp)

    def _pw_mean_logp(self, picked):
        return self.dataset.wiener_like_rlddm_nodes(self._pw_rl_table(picked, mean=True),
                                                    self._pw_ddm_table(picked, mean=True),
                                                    **self.wp)

    def _record(self, nodes):
        """HDDM._record with the learning-rate keys after the a / v / t keys:
        ..., t_std, alpha, alpha_std[, pos_alpha, pos_alpha_std], then sv / sz / st."""
        group, subj = super()._record(nodes)
        rl = {k: group.pop(k) for k in list(group) if k.split("(")[0].replace("_std", "")
              in self.rl_families}
        inter = {name: group.pop(name) for name in self.inter_names}
        for fam in self.rl_families:
            group.update((k, v) for k, v in rl.items() if k.split("(")[0] == fam)
            group[f"{fam}_std"] = rl[f"{fam}_std"]
        group.update(inter)
        return group, subj

    optimize = quantile_objective = _refuses("HDDMrl: point fits are not implemented")
    post_pred_rows = post_pred_gen = post_pred_stats = _refuses(
        "HDDMrl: a data-only posterior predictive has no reward schedule to run on; use "
        "post_pred_sim / post_pred_sim_stats")

    # -- posterior predictive ------------------------------------------------
    def post_pred_sim_rows(self, samples=500):
        """The sequence rows post_pred_sim simulates, as a dict: `picked` (S,)
        the kept sweeps (HDDM.post_pred_rows' choice); `node`, `split_by`,
        `counts` (Rn,) the (node, condition) sequences of the data, conditions
        rising inside a node, with their trial counts; `params` (S * Rn, 8) and
        `rl_rows` (S * Rn, 3) the rows in (sweep, node, condition) order, q the
        node's node_q and the other values the sweep's; `order` the data's
        trials sorted into that sequence order (the caller's order kept inside
        a sequence) and `first` (Rn,) each sequence's first element there."""
        picked, P = HDDM.post_pred_rows(self, samples)
        split = self.data["split_by"].to_numpy().astype(np.int64)
        order = np.lexsort((np.arange(split.size), split, self.node_codes))
        pairs, first, counts = np.unique(np.stack([self.node_codes[order], split[order]], axis=1),
                                         axis=0, return_index=True, return_counts=True)
        node = pairs[:, 0]
        S = picked.size
        rl = np.empty((S, node.size, 3))
        rl[:, :, 0] = self.node_q[node]
        rl[:, :, 2] = NO_POS_ALPHA
        for fam in self.rl_families:
            rl[:, :, _RL_COL[fam]] = self.trace_subj[fam][picked][:, self.node_unit[fam][node]]
        return {"picked": picked, "node": node, "split_by": pairs[:, 1],
                "counts": counts.astype(np.int64), "params": P[:, node].reshape(-1, 8),
                "rl_rows": rl.reshape(-1, 3), "order": order, "first": first.astype(np.int64)}

    def _sim_source(self, T, rewards, mode):
        """gen_rlddm_rows' reward source for the rows T of post_pred_sim_rows."""
        S = T["picked"].size
        if mode == "onestep":
            data = self.data
            return {"observed": (data["response"].to_numpy().astype(np.int64)[T["order"]],
                                 data["feedback"].to_numpy(dtype=np.float64)[T["order"]],
                                 np.tile(T["first"], S))}
        if mode != "closed":
            raise ValueError("mode must be 'closed' or 'onestep'")
        if rewards is None:
            raise ValueError("mode='closed' needs rewards: {split_by value: (p_upper, p_lower)}")
        missing = sorted(set(T["split_by"].tolist()) - {int(k) for k in rewards})
        if missing:
            raise KeyError(f"rewards has no entry for the split_by values {missing}")
        by_cond = {int(k): v for k, v in rewards.items()}
        p = np.array([by_cond[c] for c in T["split_by"].tolist()], dtype=np.float64)
        return {"rewards": np.tile(p.reshape(-1, 2), (S, 1))}

    def post_pred_sim(self, rewards=None, samples=500, seed=None, dt=1e-4, mode="closed",
                      return_debug=False):
        """Posterior predictive data of the RL model (the reference's workflow
        over gen_rand_rlddm_data, hddm/generate.py:430-516): for each of
        `samples` evenly spaced kept sweeps, each node and each split_by
        condition of the node, one simulated sequence of as many trials as the
        node has in that condition, at the sweep's parameters and from the
        node's initial Q value -- all sequences in ONE wfpt.gen_rlddm_rows
        launch (post_pred_sim_rows documents its rows).

        rewards: {split_by value: (p_upper, p_lower)}, the reward schedule the
        simulated choices run on (binary rewards drawn on the device); needed
        for mode='closed'. mode='onestep' is the reference's one-step-ahead
        simulator (generate.py:608-661): Q follows the observed responses and
        feedback, and every trial's RT is simulated at the drift they give.

        Returns a DataFrame with columns sample (index of the kept sweep), node
        (index into node_keys), split_by, trial (1-based inside the sequence),
        rt (signed), response (1 upper / 0 lower: the simulated choice) and
        feedback (the value that moved Q); with return_debug also q_up, q_low
        and sim_drift."""
        import pandas as pd
        T = self.post_pred_sim_rows(samples)
        source = self._sim_source(T, rewards, mode)
        S = T["picked"].size
        if seed is None:
            seed = int(self.rng.integers(0, 2 ** 63))
        cnt = np.tile(T["counts"], S)
        rts, _, dbg = _wfpt.gen_rlddm_rows(T["params"], T["rl_rows"], cnt, dt=dt, seed=seed,
                                           return_debug=True, **source)
        rep = lambda per_row: np.repeat(np.tile(per_row, S), cnt)
        frame = pd.DataFrame({
            "sample": np.repeat(np.repeat(T["picked"], T["node"].size), cnt),
            "node": rep(T["node"]), "split_by": rep(T["split_by"]),
            "trial": np.concatenate([np.arange(1, c + 1) for c in cnt]),
            "rt": rts, "response": (rts > 0).astype(np.int64), "feedback": dbg["feedback"]})
        if return_debug:
            for k in ("q_up", "q_low", "sim_drift"):
                frame[k] = dbg[k]
        return frame

    def post_pred_sim_stats(self, rewards=None, samples=500, seed=None, dt=1e-4, mode="closed",
                            quantiles=(10, 30, 50, 70, 90), return_sampled=False):
        """The posterior predictive check over post_pred_sim's sequences without
        the data sets: the same draws (same arguments, same seed) are reduced to
        gen_ppc_stats' statistics per (sweep, node) on the device by ONE fused
        call (wfpt.gen_rlddm_stats_rows: a node's statistics row covers its
        condition sequences; no draw is copied to the host), the observed nodes
        by one wfpt.rt_stats_rows call, and ppc.summarize compares the two.

        Returns ppc.summarize's DataFrame indexed by (node, stat), shaped like
        HDDM.post_pred_stats'; with return_sampled=True also the sampled
        statistics (len(picked), n_nodes, K)."""
        from . import ppc
        T = self.post_pred_sim_rows(samples)
        source = self._sim_source(T, rewards, mode)
        S = T["picked"].size
        if seed is None:
            seed = int(self.rng.integers(0, 2 ** 63))
        per_node = np.bincount(T["node"], minlength=self.n_nodes)
        groups = np.r_[0, np.cumsum(np.tile(per_node, S))]
        sampled, _ = _wfpt.gen_rlddm_stats_rows(T["params"], T["rl_rows"], np.tile(T["counts"], S),
                                                groups, quantiles=quantiles, dt=dt, seed=seed,
                                                **source)
        sampled = sampled.reshape(S, self.n_nodes, -1)
        order = np.argsort(self.node_codes, kind="stable")
        offsets = np.zeros(self.n_nodes + 1, dtype=np.int64)
        np.cumsum(self.node_counts, out=offsets[1:])
        observed = _wfpt.rt_stats_rows(self.signed_rt[order], offsets, quantiles)
        table = ppc.summarize(observed, sampled, _wfpt.rt_stats_names(quantiles))
        return (table, sampled) if return_sampled else table


def gen_rl_data(n_subj, n_trials, conds, a, t, v, alpha, pos_alpha=None, z=0.5, q_init=0.5,
                jitter=0.1, seed=20261020, dt=1e-3, draw=None, closed_loop="host"):
    """Synthetic two-armed-bandit data from the RLDDM in closed loop
    (hddm/generate.py:430-516): n_trials trials for each of n_subj subjects in
    each condition of `conds`, {split_by value: (p_upper, p_lower)} the reward
    probabilities of the two options. a, t and the drift scaling v are jittered
    per subject by +-jitter (relative), alpha (and pos_alpha, when given) by
    +-jitter on the likelihood's unbounded scale; the rate is RL_BASE**alpha /
    (1 + RL_BASE**alpha).

    The binary rewards are drawn up front. Then all (subject, condition)
    sequences advance in lockstep: at step k ONE sampler call draws one RT per
    sequence at the current drifts (q_up - q_low) * v, the chosen option's
    reward is the feedback, and its Q value moves by q + alfa * (f - q) in
    plain Python floats, so the recorded `sim_drift` equals the likelihood's
    drift exactly. draw(drifts) -> signed RTs replaces the device draw
    (wfpt.gen_rts_from_cdf_nodes with a device seed per step).

    closed_loop='device' runs the whole loop in ONE wfpt.gen_rlddm_rows launch
    instead: the same up-front rewards from the same generator stream go in as
    supplied arrays, every RT is a simulated diffusion path with time step dt,
    and the Q values move on the device in the likelihood's rounding (`draw`
    is not used). The columns are the same.

    Returns (DataFrame, truth): columns rt (signed), response, feedback,
    split_by, subj_idx, q_init, trial, q_up, q_low, sim_drift; truth the true
    subject parameters {'a', 't', 'v', 'alpha'[, 'pos_alpha']}."""
    rng = np.random.default_rng(seed)
    labels = [int(c) for c in conds]
    jit = lambda: jitter * rng.uniform(-1, 1)
    truth = {k: [] for k in ("a", "t", "v", "alpha") + (("pos_alpha",) if pos_alpha is not None
                                                        else ())}
    for _ in range(n_subj):
        truth["a"].append(a * (1 + jit()))
        truth["t"].append(t * (1 + jit()))
        truth["v"].append(v * (1 + jit()))
        truth["alpha"].append(alpha + jit())
        if pos_alpha is not None:
            truth["pos_alpha"].append(pos_alpha + jit())
    seqs = [(s, c) for s in range(n_subj) for c in labels]
    S = len(seqs)
    rew = {(s, c): (rng.binomial(1, conds[c][0], n_trials).astype(np.float64),
                    rng.binomial(1, conds[c][1], n_trials).astype(np.float64))
           for s, c in seqs}
    if closed_loop not in ("host", "device"):
        raise ValueError("closed_loop must be 'host' or 'device'")
    P = np.zeros((S, 8))
    P[:, 2] = [truth["a"][s] for s, _ in seqs]
    P[:, 3] = z
    P[:, 5] = [truth["t"][s] for s, _ in seqs]
    if closed_loop == "device":
        P[:, 0] = [truth["v"][s] for s, _ in seqs]
        rows = np.empty((S, 3))
        rows[:, 0] = q_init
        rows[:, 1] = [truth["alpha"][s] for s, _ in seqs]
        rows[:, 2] = [truth["pos_alpha"][s] for s, _ in seqs] if pos_alpha is not None \
            else NO_POS_ALPHA
        arrays = tuple(np.concatenate([rew[sc][i] for sc in seqs]) for i in (0, 1))
        rts, _, dbg = _wfpt.gen_rlddm_rows(P, rows, n_trials, reward_arrays=arrays, dt=dt,
                                           seed=int(rng.integers(0, 2 ** 63)), return_debug=True)
        cols = {"rt": rts, "response": rts > 0, **{k: dbg[k] for k in ("feedback", "q_up",
                                                                       "q_low", "sim_drift")}}
        return _rl_frame(cols, seqs, n_trials, q_init), truth
    if draw is None:
        def draw(drifts):
            P[:, 0] = drifts
            rts, _ = _wfpt.gen_rts_from_cdf_nodes(P, 1, dt=dt, seed=int(rng.integers(0, 2 ** 63)))
            return rts
    scale = [float(truth["v"][s]) for s, _ in seqs]
    neg = [learning_rate(truth["alpha"][s]) for s, _ in seqs]
    pos = [learning_rate(truth["pos_alpha"][s]) for s, _ in seqs] if pos_alpha is not None \
        else neg
    q_up, q_low = [float(q_init)] * S, [float(q_init)] * S
    cols = {k: np.empty((S, n_trials)) for k in ("rt", "response", "feedback", "q_up", "q_low",
                                                 "sim_drift")}
    for k in range(n_trials):
        drifts = [(q_up[i] - q_low[i]) * scale[i] for i in range(S)]
        rts = np.asarray(draw(np.array(drifts)), dtype=np.float64)
        for i, (s, c) in enumerate(seqs):
            up = bool(rts[i] > 0)
            f = float(rew[s, c][0 if up else 1][k])
            cols["rt"][i, k], cols["response"][i, k], cols["feedback"][i, k] = rts[i], up, f
            cols["q_up"][i, k], cols["q_low"][i, k] = q_up[i], q_low[i]
            cols["sim_drift"][i, k] = drifts[i]
            q = q_up[i] if up else q_low[i]
            alfa = pos[i] if f > q else neg[i]
            q = q + alfa * (f - q)
            if up:
                q_up[i] = q
            else:
                q_low[i] = q
    return _rl_frame(cols, seqs, n_trials, q_init), truth


def _rl_frame(cols, seqs, n_trials, q_init):
    """gen_rl_data's frame from per-trial columns, sequence after sequence."""
    import pandas as pd
    return pd.DataFrame({
        "rt": cols["rt"].ravel(), "response": cols["response"].ravel().astype(np.int64),
        "feedback": cols["feedback"].ravel(),
        "split_by": np.repeat([c for _, c in seqs], n_trials).astype(np.int64),
        "subj_idx": np.repeat([s for s, _ in seqs], n_trials).astype(np.int64),
        "q_init": float(q_init), "trial": np.tile(np.arange(1, n_trials + 1), len(seqs)),
        "q_up": cols["q_up"].ravel(), "q_low": cols["q_low"].ravel(),
        "sim_drift": cols["sim_drift"].ravel()})
