"""The on-device diffusion-path simulator (`wfpt.gen_rts_from_drift_nodes`,
the 'drift' sampling method, hddm/generate.py:208-319) on one GPU.

Two shapes at the reference's documented dt = 1e-4:
  rows400x250   400 rows x 250 draws of config 4's truth-like parameters
                (bench_ppc.rows_config4)
  row1x1e6      one row of the bench model x 1,000,000 draws

Per shape, the schedules wave_draws = default, 64 (one draw per lane), 256 and
1024 (lanes take the next draw of their wave's range as they finish) run
interleaved, `--rounds` times each: host clock around the whole call (median),
then one pass each under the context's profile events for the kernel time,
and one debugging pass for the steps taken: steps per second of kernel time
and the wave-efficiency proxy sum(steps) / (64 x sum over waves of the steps
that wave's loop ran). For context the inverse-CDF sampler runs on the same
rows (grid (-5, 5, dt)).

The baseline is a NumPy restatement of the reference's per-trial loop (blocks
of 1000 uniforms, cumsum, first crossing), timed here on `--baseline-trials`
trials of the shape's first row; its time for the whole shape is that
per-trial time times the shape's draws: an extrapolation, labelled as such.

    python tools/bench_drift.py [--rounds 3] [--out profiles/drift/rows.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ppc import rows_config4  # noqa: E402
from hddm_amd import _lib, build as hb, wfpt  # noqa: E402

DT = 1e-4
SCHEDULES = (None, 64, 256, 1024)


def numpy_trial(v, a, y0, dt, rng, nn=1000):
    """One trial the way the reference walks it: nn uniforms at a time, their
    running sum, the first position outside (0, a). Returns the steps
    generated (whole blocks)."""
    step = np.sqrt(dt)
    p = 0.5 * (1 + np.sqrt(dt) * v)
    made, y = 0, y0
    while True:
        pos = ((rng.random(nn) < p) * 2 - 1) * step
        pos[0] += y
        pos = np.cumsum(pos)
        made += nn
        if np.flatnonzero((pos < 0) | (pos > a)).size:
            return made
        y = pos[-1]


def numpy_baseline(row, trials, dt):
    rng = np.random.default_rng(1)
    v, sv, a, z, sz = row[:5]
    t0 = time.perf_counter()
    made = sum(numpy_trial(v + sv * rng.standard_normal(), a,
                           (z + sz * (rng.random() - 0.5)) * a, dt, rng) for _ in range(trials))
    sec = time.perf_counter() - t0
    return {"trials": trials, "seconds": sec, "ms_per_trial": sec * 1e3 / trials,
            "ns_per_generated_step": sec * 1e9 / made}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-trials", type=int, default=200)
    ap.add_argument("--big", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drift", "rows.json"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_drift: no HIP device")
    ctx = _lib.context()
    shapes = [("rows400x250", rows_config4(200), 250),
              ("row1x1e6", np.array([(0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1)]), a.big)]
    out = {"build": hb.built_digest(_lib.LIB_PATH), "source": hb.source_digest(), "dt": DT,
           "rounds": a.rounds, "shapes": []}
    for name, P, n in shapes:
        draws = P.shape[0] * n
        call = {wd: (lambda wd=wd: wfpt.gen_rts_from_drift_nodes(P, n, dt=DT, seed=1,
                                                                 wave_draws=wd))
                for wd in SCHEDULES}
        ref = call[None]()[0]  # warm-up: workspaces, code objects
        wall = {wd: [] for wd in SCHEDULES}
        for _ in range(a.rounds):  # interleaved
            for wd in SCHEDULES:
                t0 = time.perf_counter()
                rts = call[wd]()[0]
                wall[wd].append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(rts, ref), "a schedule changed a draw"
        sched = []
        for wd in SCHEDULES:
            ctx.profile(1)
            ctx.profile_read(reset=True)
            call[wd]()
            kernel_ms = ctx.profile_read(reset=True)[0]
            ctx.profile(0)
            row = {"wave_draws": "default" if wd is None else wd,
                   "call_ms": float(np.median(wall[wd])), "call_ms_all": wall[wd],
                   "kernel_ms": kernel_ms}
            if wd is not None:
                d = wfpt.gen_rts_from_drift_nodes(P, n, dt=DT, seed=1, wave_draws=wd,
                                                  return_debug=True)[2]
                steps = int(d["n_steps"].sum())
                row.update(steps=steps, mean_steps=steps / draws,
                           longest_trial=int(d["n_steps"].max()), waves=int(d["wave_steps"].size),
                           steps_per_second=steps / (kernel_ms * 1e-3),
                           wave_efficiency=steps / (64.0 * float(d["wave_steps"].sum())))
            sched.append(row)
        lb, ub = -5, 5
        cdf = lambda: wfpt.gen_rts_from_cdf_nodes(P, n, lb, ub, DT, seed=1)
        cdf()
        tc = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            cdf()
            tc.append((time.perf_counter() - t0) * 1e3)
        base = numpy_baseline(P[0], a.baseline_trials, DT)
        base["extrapolated_ms_for_shape"] = base["ms_per_trial"] * draws
        row = {"shape": name, "rows": int(P.shape[0]), "draws": draws, "schedules": sched,
               "cdf_sampler_call_ms": float(np.median(tc)), "cdf_sampler_call_ms_all": tc,
               "numpy_baseline": base,
               "extrapolated_speedup_default": base["extrapolated_ms_for_shape"] / sched[0]["call_ms"]}
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "build": out["build"]}))


if __name__ == "__main__":
    main()
