"""The regressor's posterior predictive (`RegDataset.gen_rts_drift[_stats]`,
wfpt_gen_rts_reg_drift) on one GPU.

Shape: `--subjects` 200 x `--trials` 500 trials x `--sweeps` 100 sweeps at the
reference's documented dt = 1e-4, `v ~ 1 + cov` (identity) and `a ~ 1` (exp),
one coefficient and parameter row per (sweep, subject).

  (a) the new call: host clock around it (median of `--rounds` after a
      warm-up), kernel time under the context's profile events, draws/s and,
      from one debugging pass, steps/s of kernel time and the wave-efficiency
      proxy sum(steps) / (64 x sum over waves of the steps that wave's loop ran)
  (b) the statistics call (no draw leaves the device): host clock
  (c) the route by hand on the same inputs: the predicted parameters of every
      sweep pulled back with wiener_like_reg_groups(terms=True), stacked into
      an (S n, 8) host table, one gen_rts_from_drift_nodes call with one draw
      per row; host clock over all of it, and the table build alone
  (d) the walk alone: gen_rts_from_drift_nodes over one row per subject with as
      many draws as (a) has: kernel time, steps/s, wave efficiency. The gap
      between (d)'s and (a)'s steps/s, less what the wave efficiencies explain,
      is what forming the parameters at refill costs.

    python tools/bench_reg_sim.py [--rounds 3] [--out profiles/reg_sim/shape.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hddm_amd import _lib, build as hb, wfpt  # noqa: E402

DT = 1e-4
MODEL = [("v", 0, 2, "identity"), ("a", 2, 1, "exp")]


def inputs(n_subj, n_trials, S, seed=1):
    rng = np.random.default_rng(seed)
    n = n_subj * n_trials
    gid = np.repeat(np.arange(n_subj), n_trials).astype(np.int32)
    X = np.column_stack([np.ones(n), rng.normal(size=n), np.ones(n)])
    rt = rng.choice([-1.0, 1.0], n, p=[0.3, 0.7]) * (0.4 + rng.gamma(2.0, 0.3, n))
    coef = np.empty((S, n_subj, 3))
    coef[..., 0] = rng.normal(1.0, 0.3, (S, n_subj))
    coef[..., 1] = rng.normal(0.3, 0.1, (S, n_subj))
    coef[..., 2] = np.log(rng.uniform(1.6, 2.2, (S, n_subj)))
    par = np.zeros((S, n_subj, 8))
    par[..., 3] = 0.5
    par[..., 5] = rng.uniform(0.25, 0.35, (S, n_subj))
    return rt, X, gid, coef, par


def clock(fn, rounds):
    fn()  # warm-up: workspaces, code objects
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), ms


def kernel_ms(ctx, fn):
    ctx.profile(1)
    ctx.profile_read(reset=True)
    fn()
    ms = ctx.profile_read(reset=True)[0]
    ctx.profile(0)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=200)
    ap.add_argument("--trials", type=int, default=500)
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reg_sim", "shape.json"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_reg_sim: no HIP device")
    ctx = _lib.context()
    G, S = a.subjects, a.sweeps
    rt, X, gid, coef, par = inputs(G, a.trials, S)
    n = rt.size
    draws = S * n
    ds = wfpt.RegDataset(rt, X, group_id=gid, n_groups=G)
    out = {"build": hb.built_digest(_lib.LIB_PATH), "source": hb.source_digest(), "dt": DT,
           "rounds": a.rounds, "subjects": G, "trials": a.trials, "sweeps": S, "draws": draws}

    # (a)
    new = lambda: ds.gen_rts_drift(MODEL, coef, par, dt=DT, seed=1)
    call_ms, all_ms = clock(new, a.rounds)
    k_ms = kernel_ms(ctx, new)
    wd = 64 * min(16, max(1, draws // (64 * 4096)))  # the library's default for this call
    dbg = ds.gen_rts_drift(MODEL, coef, par, dt=DT, seed=1, wave_draws=wd, return_debug=True)[1]
    steps = int(dbg["n_steps"].sum())
    eff = steps / (64.0 * float(dbg["wave_steps"].sum()))
    table = np.zeros((draws, 8))
    table[:, :7] = dbg["params"].reshape(draws, 7)
    del dbg
    out["new_call"] = {"call_ms": call_ms, "call_ms_all": all_ms, "kernel_ms": k_ms,
                       "draws_per_second": draws / (k_ms * 1e-3), "steps": steps,
                       "mean_steps": steps / draws, "steps_per_second": steps / (k_ms * 1e-3),
                       "wave_draws": wd, "wave_efficiency": eff}
    print(json.dumps({"new_call": out["new_call"]}), flush=True)

    # (b)
    st_ms, st_all = clock(lambda: ds.gen_rts_drift_stats(MODEL, coef, par, dt=DT, seed=1),
                          a.rounds)
    out["stats_call"] = {"call_ms": st_ms, "call_ms_all": st_all}
    print(json.dumps({"stats_call": out["stats_call"]}), flush=True)

    # (c)
    def by_hand():
        t0 = time.perf_counter()
        T = np.zeros((S, n, 8))
        T[..., 3] = 0.5
        for s in range(S):
            pred = ds.wiener_like_reg_groups(MODEL, coef[s], par[s], terms=True)[2]
            T[s, :, 0], T[s, :, 2] = pred["v"], pred["a"]
            T[s, :, 5] = par[s][gid, 5]
        build = time.perf_counter() - t0
        wfpt.gen_rts_from_drift_nodes(T.reshape(draws, 8), 1, dt=DT, seed=1)
        return build * 1e3

    build_ms = by_hand()  # warm-up
    hand, builds = [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        builds.append(by_hand())
        hand.append((time.perf_counter() - t0) * 1e3)
    pred0 = ds.wiener_like_reg_groups(MODEL, coef[0], par[0], terms=True)[2]
    assert np.array_equal(table[:n, 0], pred0["v"]) and np.array_equal(table[:n, 2], pred0["a"])
    hand_k = kernel_ms(ctx, lambda: wfpt.gen_rts_from_drift_nodes(table, 1, dt=DT, seed=1))
    out["by_hand"] = {"call_ms": float(np.median(hand)), "call_ms_all": hand,
                      "table_build_ms": float(np.median(builds)), "first_build_ms": build_ms,
                      "table_bytes": int(table.nbytes), "sampler_kernel_ms": hand_k}
    print(json.dumps({"by_hand": out["by_hand"]}), flush=True)
    del table

    # (d)
    rows = np.zeros((G, 8))
    rows[:, 0], rows[:, 2], rows[:, 3], rows[:, 5] = 1.0, 1.9, 0.5, 0.3
    per = draws // G
    walk = lambda: wfpt.gen_rts_from_drift_nodes(rows, per, dt=DT, seed=1)
    walk()
    w_ms = kernel_ms(ctx, walk)
    w_dbg = wfpt.gen_rts_from_drift_nodes(rows, per, dt=DT, seed=1, wave_draws=wd,
                                          return_debug=True)[2]
    w_steps = int(w_dbg["n_steps"].sum())
    out["walk_only"] = {"rows": G, "draws": per * G, "kernel_ms": w_ms, "steps": w_steps,
                        "steps_per_second": w_steps / (w_ms * 1e-3), "wave_draws": wd,
                        "wave_efficiency": w_steps / (64.0 * float(w_dbg["wave_steps"].sum()))}
    print(json.dumps({"walk_only": out["walk_only"]}), flush=True)
    out["new_over_by_hand"] = out["by_hand"]["call_ms"] / call_ms
    out["refill_cost"] = 1.0 - out["new_call"]["steps_per_second"] / \
        out["walk_only"]["steps_per_second"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "build": out["build"],
                      "new_over_by_hand": out["new_over_by_hand"],
                      "refill_cost": out["refill_cost"]}))


if __name__ == "__main__":
    main()
