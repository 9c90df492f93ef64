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

The posterior predictive of an RL model needs a closed-loop simulator on the
device (every draw feeds the next trial's drift) and is not part of this
module; `gen_rl_data` below is the host-driven closed loop for synthetic data.
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
        "HDDMrl: the posterior predictive needs a closed-loop simulator and is not implemented")


def gen_rl_data(n_subj, n_trials, conds, a, t, v, alpha, pos_alpha=None, z=0.5, q_init=0.5,
                jitter=0.1, seed=20261020, dt=1e-3, draw=None):
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

    Returns (DataFrame, truth): columns rt (signed), response, feedback,
    split_by, subj_idx, q_init, trial, q_up, q_low, sim_drift; truth the true
    subject parameters {'a', 't', 'v', 'alpha'[, 'pos_alpha']}."""
    import pandas as pd
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
    P = np.zeros((S, 8))
    P[:, 2] = [truth["a"][s] for s, _ in seqs]
    P[:, 3] = z
    P[:, 5] = [truth["t"][s] for s, _ in seqs]
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
    frame = pd.DataFrame({
        "rt": cols["rt"].ravel(), "response": cols["response"].ravel().astype(np.int64),
        "feedback": cols["feedback"].ravel(),
        "split_by": np.repeat([c for _, c in seqs], n_trials).astype(np.int64),
        "subj_idx": np.repeat([s for s, _ in seqs], n_trials).astype(np.int64),
        "q_init": float(q_init), "trial": np.tile(np.arange(1, n_trials + 1), S),
        "q_up": cols["q_up"].ravel(), "q_low": cols["q_low"].ravel(),
        "sim_drift": cols["sim_drift"].ravel()})
    return frame, truth
