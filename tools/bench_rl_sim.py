"""The closed-loop RLDDM simulator (`wfpt.gen_rlddm_rows`) on
one GPU.

  (a) host loop against device loop at bench_rl's shape, 40 subjects x 4
      conditions x 75 trials: `rl.gen_rl_data` with closed_loop='host' and its
      default inverse-CDF draw, the same with draw= bound to
      `gen_rts_from_drift_nodes` at the same dt (the like-for-like: one walk
      launch per trial step, the Q update in Python in between), and
      closed_loop='device' (one launch); jitter = 0, so that the walk draw can
      use one a and t for every subject. The three run interleaved, `--rounds`
      times each; a host clock around the whole call, which ends in the
      library's wait for the stream.
  (b) the predictive shape, 500 sweeps x 40 nodes x 4 conditions x 75 trials at
      dt = 1e-4: seconds per call (host clock, `--rounds` calls after a
      warm-up), the kernel time under the context's profile events in a pass of
      its own, the walk steps from a debugging pass, steps per second of kernel
      time. For the comparison the open-loop kernel
      (`gen_rts_from_drift_nodes`) draws 75 RTs for each of the same rows in
      the same process (v = 0: the first trial's drift), measured the same way.
      Both rows carry the wave efficiency (lanes stepping over lanes held).
      Then the closed loop alone on four times the sequences, which puts four
      times the waves on every SIMD.

    python tools/bench_rl_sim.py [--rounds 3] [--sweeps 500] [--out profiles/rl_sim/rows.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hddm_amd import _lib, build as hb, rl, wfpt  # noqa: E402

CONDS = {0: (0.8, 0.2), 1: (0.7, 0.3), 2: (0.6, 0.4), 3: (0.9, 0.1)}
TRUTH = dict(a=2.0, t=0.3, v=2.5, alpha=-0.5)
N_SUBJ, N_TRIALS = 40, 75
DT_DATA = 1e-3  # gen_rl_data's default
DT = 1e-4       # the reference's documented step


def spread(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)),
            "all": [float(x) for x in ms]}


def walk_draw(dt):
    """gen_rl_data's draw(drifts) by the open-loop walk: one launch per step."""
    state = {"k": 0}

    def draw(drifts):
        state["k"] += 1
        T = np.zeros((drifts.size, 7))
        T[:, 0], T[:, 2], T[:, 3], T[:, 5] = drifts, TRUTH["a"], 0.5, TRUTH["t"]
        return wfpt.gen_rts_from_drift_nodes(T, 1, dt=dt, seed=1000 + state["k"])[0]
    return draw


def data_loops(rounds):
    kinds = {
        "host_cdf_draw": lambda: rl.gen_rl_data(N_SUBJ, N_TRIALS, CONDS, dt=DT_DATA, jitter=0,
                                                **TRUTH),
        "host_walk_draw": lambda: rl.gen_rl_data(N_SUBJ, N_TRIALS, CONDS, dt=DT_DATA, jitter=0,
                                                 draw=walk_draw(DT_DATA), **TRUTH),
        "device": lambda: rl.gen_rl_data(N_SUBJ, N_TRIALS, CONDS, dt=DT_DATA, jitter=0,
                                         closed_loop="device", **TRUTH)}
    for f in kinds.values():  # warm-up: code objects, workspaces
        f()
    ms = {k: [] for k in kinds}
    for _ in range(rounds):  # interleaved
        for k, f in kinds.items():
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"shape": f"{N_SUBJ} subjects x {len(CONDS)} conditions x {N_TRIALS} trials",
           "dt": DT_DATA, "call_ms": {k: spread(v) for k, v in ms.items()}}
    med = {k: out["call_ms"][k]["median"] for k in kinds}
    out["host_walk_over_device"] = med["host_walk_draw"] / med["device"]
    out["host_cdf_over_device"] = med["host_cdf_draw"] / med["device"]
    return out


def kernel_ms(ctx, f):
    ctx.profile(1)
    ctx.profile_read(reset=True)
    f()
    ms = ctx.profile_read(reset=True)[0]
    ctx.profile(0)
    return ms


def predictive(ctx, sweeps, rounds, open_too=True):
    rng = np.random.default_rng(7)
    n_seq = sweeps * N_SUBJ * len(CONDS)
    # one value per (sweep, subject), repeated over the subject's conditions
    per = lambda centre, width: np.repeat(centre + width * rng.uniform(-1, 1, sweeps * N_SUBJ),
                                          len(CONDS))
    P = np.zeros((n_seq, 8))
    P[:, 0] = per(TRUTH["v"], 0.25)
    P[:, 2] = per(TRUTH["a"], 0.2)
    P[:, 3] = 0.5
    P[:, 5] = per(TRUTH["t"], 0.03)
    RL = np.empty((n_seq, 3))
    RL[:, 0], RL[:, 1], RL[:, 2] = 0.5, per(TRUTH["alpha"], 0.1), 100.0
    p = np.tile(np.array([CONDS[c] for c in CONDS]), (sweeps * N_SUBJ, 1))
    closed = lambda **kw: wfpt.gen_rlddm_rows(P, RL, N_TRIALS, rewards=p, dt=DT, seed=1, **kw)
    P0 = P.copy()
    P0[:, 0] = 0.0
    open_loop = lambda **kw: wfpt.gen_rts_from_drift_nodes(P0, N_TRIALS, dt=DT, seed=1, **kw)
    out = {"shape": f"{sweeps} sweeps x {N_SUBJ} nodes x {len(CONDS)} conditions x {N_TRIALS} "
                    "trials", "sequences": n_seq, "trials": n_seq * N_TRIALS, "dt": DT}
    # the schedules the two calls take by default at this size, named so that
    # the debugging pass also returns the steps each wave's loop ran
    sched = {"closed_loop": {"wave_rows": 64 * min(16, max(1, n_seq // (64 * 4096)))},
             "open_loop_same_rows": {"wave_draws": 64 * min(16, max(1, n_seq * N_TRIALS
                                                                    // (64 * 4096)))}}
    runs = (("closed_loop", closed), ("open_loop_same_rows", open_loop))
    for name, f in runs[:2 if open_too else 1]:
        f()  # warm-up
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            f()
            ms.append((time.perf_counter() - t0) * 1e3)
        k_ms = [kernel_ms(ctx, f) for _ in range(rounds)]
        d = f(return_debug=True, **sched[name])[2]
        steps = int(d["n_steps"].sum())
        k_med = float(np.median(k_ms))
        out[name] = {"call_ms": spread(ms), "kernel_ms": spread(k_ms), "steps": steps,
                     **sched[name], "waves": int(d["wave_steps"].size),
                     # lanes stepping over lanes held: the rest waits for the wave's last lane
                     "wave_efficiency": steps / (64.0 * float(d["wave_steps"].sum())),
                     "mean_steps_per_trial": steps / (n_seq * N_TRIALS),
                     "steps_per_second_of_kernel_time": steps / (k_med * 1e-3),
                     "steps_per_second_of_call_time": steps / (float(np.median(ms)) * 1e-3)}
    if open_too:
        out["closed_over_open_step_rate"] = (
            out["closed_loop"]["steps_per_second_of_kernel_time"] /
            out["open_loop_same_rows"]["steps_per_second_of_kernel_time"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rl_sim", "rows.json"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_rl_sim: no HIP device")
    ctx = _lib.context()
    out = {"build": hb.built_digest(_lib.LIB_PATH), "source": hb.source_digest(),
           "rounds": a.rounds}
    out["data_loops"] = data_loops(a.rounds)
    print(json.dumps(out["data_loops"]), flush=True)
    out["predictive"] = predictive(ctx, a.sweeps, a.rounds)
    print(json.dumps(out["predictive"]), flush=True)
    # four times the sequences: four times the waves on every SIMD
    out["predictive_x4"] = predictive(ctx, 4 * a.sweeps, a.rounds, open_too=False)
    print(json.dumps(out["predictive_x4"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "build": out["build"]}))


if __name__ == "__main__":
    main()
