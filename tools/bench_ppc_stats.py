"""The posterior predictive check on one GPU: the fused statistics against the
host reduction they replace.

  fused   `HDDM.post_pred_stats`: one sampler call whose draws are reduced to
          gen_ppc_stats' statistics on the device (wfpt_gen_rts_nodes_stats);
          no draw is copied out
  host    `HDDM.post_pred_gen` (the draws copied out into a DataFrame), then
          `ppc.gen_ppc_stats()`'s NumPy callables applied to every (sample,
          node) group on the host: what the check took before

Shape: config 4, 400 nodes x 250 trials (hierarchical.gen_data), `--sweeps`
kept sweeps of parameters jittered around the generating values (the traces
are made up: only their shape matters here), the stochastic's default grid dt
= 1e-4 over (-5, 5). The two paths alternate on the same device, `--rounds`
times each; the figures are host clocks around the whole call (median over
the rounds). The sampler's stage times and the statistics kernels' time come
from the context's profile events in a pass of its own. Writes
profiles/ppc/stats.json with the build digest.

    python tools/bench_ppc_stats.py [--sweeps 500] [--rounds 3] [--out profiles/ppc/stats.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hddm_amd import _lib, build as hb, ppc, wfpt  # noqa: E402
from hddm_amd.hierarchical import HDDM, gen_data  # noqa: E402


def model_config4(sweeps, n_subj, n_trials, seed=20261020):
    data, _ = gen_data(n_subj=n_subj, n_trials=n_trials)
    m = HDDM(data, depends_on={"v": "cond"}, seed=0)
    rng = np.random.default_rng(seed)
    m.trace_subj = {"a": 2.0 * (1 + 0.1 * rng.uniform(-1, 1, (sweeps, m.n_units["a"]))),
                    "v": 0.75 * (1 + 0.4 * rng.uniform(-1, 1, (sweeps, m.n_units["v"]))),
                    "t": 0.3 * (1 + 0.1 * rng.uniform(-1, 1, (sweeps, m.n_units["t"])))}
    m.trace = {}
    return m


def host_stats(frame, names):
    """gen_ppc_stats applied per (sample, node) group: (groups, len(names))."""
    stats = ppc.gen_ppc_stats()
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)  # empty boundaries
        return np.array([[stats[k](x) for k in names]
                         for x in (g.to_numpy() for _, g in
                                   frame.groupby(["sample", "node"], sort=True)["rt"])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--subjects", type=int, default=200)
    ap.add_argument("--trials", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppc", "stats.json"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_ppc_stats: no HIP device")
    ctx = _lib.context()
    m = model_config4(a.sweeps, a.subjects, a.trials)
    S = a.sweeps
    names = wfpt.rt_stats_names()[3:]
    fused = lambda: m.post_pred_stats(samples=S, seed=1, return_sampled=True)

    def host():
        t0 = time.perf_counter()
        frame = m.post_pred_gen(samples=S, seed=1)
        t1 = time.perf_counter()
        return host_stats(frame, names), (t1 - t0) * 1e3
    m.post_pred_stats(samples=2, seed=1)  # warm-up: workspaces, code objects
    tf, th, tg = [], [], []
    for r in range(a.rounds):  # alternating
        t0 = time.perf_counter()
        _, sampled = fused()
        t1 = time.perf_counter()
        ref, gen_ms = host()
        t2 = time.perf_counter()
        tf.append((t1 - t0) * 1e3)
        th.append((t2 - t1) * 1e3)
        tg.append(gen_ms)
        print(json.dumps({"round": r, "fused_ms": tf[-1], "host_ms": th[-1],
                          "host_post_pred_gen_ms": gen_ms}), flush=True)
    got = sampled.reshape(-1, sampled.shape[-1])[:, 3:]
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    moments = [names.index(k) for k in ("mean_ub", "std_ub", "mean_lb", "std_lb")]
    exact = [k for k in range(len(names)) if k not in moments]
    ctx.profile(1)
    ctx.profile_read(reset=True)
    ctx.profile_stages(reset=True)
    fused()
    total_ms = ctx.profile_read(reset=True)[0]
    stages = ctx.profile_stages(reset=True)
    ctx.profile(0)
    out = {"build": hb.built_digest(_lib.LIB_PATH), "source": hb.source_digest(),
           "nodes": m.n_nodes, "trials_per_node": int(m.node_counts[0]), "sweeps": S,
           "rows": S * m.n_nodes, "draws": int(S * m.node_counts.sum()), "rounds": a.rounds,
           "fused_ms": float(np.median(tf)), "host_ms": float(np.median(th)),
           "host_post_pred_gen_ms": float(np.median(tg)),
           "fused_ms_all": tf, "host_ms_all": th, "host_post_pred_gen_ms_all": tg,
           "speedup": float(np.median(th) / np.median(tf)),
           "stage_kernel_ms": stages,
           # both reductions of the pass: the sweeps' rows and the observed nodes
           "stats_kernel_ms": total_ms - sum(stages.values()),
           "exact_columns_equal_host": bool(same[:, exact].all()),
           "moment_columns_max_rel_diff": float(np.nanmax(
               np.abs(got[:, moments] - ref[:, moments]) / np.abs(ref[:, moments])))}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "build": out["build"]}))


if __name__ == "__main__":
    main()
