"""Call time of the RL regression likelihood on one GPU, against the only route
that existed without it.

Workloads: S subjects x T trials (40 x 300 and 200 x 500), two split_by
conditions per subject in contiguous runs, HDDM's knobs, p_outlier 0.05,
sv = sz = st = 0; models `v ~ 1 + cov, alpha ~ 1 + cov` ("v_alpha") and
`v ~ 1 + cov` alone ("v"). Routes:

  a. ONE `RLRegDataset.wiener_like_rl_reg_groups` call: a sum per subject;
  b. today's route: the predictions `X @ b` in NumPy, then one
     `wfpt.wiener_like_multi_rlddm` per subject (eight uploads, a relayout and,
     with alpha regressed, a host pow per trial in every call).

Each figure is a host clock around calls that end in the library's wait for
the device's completion word; every shape is warmed up; a window lasts at
least --seconds; the routes alternate in one process for --rounds rounds and
each route's median and spread (max - min) over the rounds are reported, with
the ratio b / a of the medians. Route (a)'s device time per call comes from the
library's HIP events around its three launches (fill, scan, scoring pass +
per-group sums), a window of its own. The per-subject sums of the two routes
are compared in the same run (relative difference below 1e-9: `X @ b` is
another summation order than the device's, and libm's pow may differ from the
correctly rounded one by an ulp).

    python tools/bench_rl_reg.py [--seconds 0.5] [--rounds 5] [--sizes 40x300 200x500]
                                 [--routes ab] [--out profiles/rl_reg/rows.json]
    python tools/bench_rl_reg.py --merge-trace 40x300:v_alpha=stats.csv ... --out ...

--merge-trace adds the average time per launch of each kernel of route (a)
from `rocprofv3 --kernel-trace --stats --output-format csv` runs of their own
(one per size and model, started with --sizes S --models M --routes a) to an
existing rows file.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {"v_alpha": [("v", 0, 2, "identity"), ("alpha", 2, 2, "identity")],
          "v": [("v", 0, 2, "identity")]}
COEF = np.array([2.5, 0.3, -0.8, 0.4])
DDM = dict(sv=0.0, a=1.8, z=0.5, sz=0.0, t=0.3, st=0.0)
KNOBS = dict(err=1e-4, n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, w_outlier=0.1)
P_OUTLIER = 0.05
Q, ALPHA = 0.5, -0.8
KERNELS = ("rl_reg_fill_kernel", "rl_scan_kernel", "multi_fast_kernel", "rl_node_sum_kernel")


def workload(subjects, per, seed=11):
    rng = np.random.default_rng(seed)
    n = subjects * per
    subj = np.repeat(np.arange(subjects, dtype=np.int32), per)
    split = np.tile(np.repeat(np.arange(2, dtype=np.int64), [per // 2, per - per // 2]), subjects)
    cov = rng.normal(size=n)
    X = np.ascontiguousarray(np.column_stack([np.ones(n), cov, np.ones(n), cov]))
    rt = (DDM["t"] + 0.1 + rng.gamma(2.0, 0.3, n)) * rng.choice([-1.0, 1.0], n, p=[0.3, 0.7])
    response = (rt > 0).astype(np.int64)
    feedback = rng.binomial(1, np.where(response == 1, 0.8, 0.2)).astype(np.float64)
    return rt, response, feedback, split, X, subj


def window(call, seconds):
    """ms per call over one window of at least `seconds`."""
    reps = 4
    while True:
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        el = time.perf_counter() - t0
        if el >= seconds:
            return el / reps * 1e3
        reps *= 2


def measure(a):
    from hddm_amd import _lib, build as hb, wfpt
    if _lib.device_count() < 1:
        raise SystemExit("bench_rl_reg: no HIP device")
    out = {"build": hb.built_digest(_lib.LIB_PATH), "source": hb.source_digest(),
           "seconds": a.seconds, "rounds": a.rounds, "rows": []}
    for size in a.sizes:
        S, per = (int(v) for v in size.split("x"))
        rt, response, feedback, split, X, subj = workload(S, per)
        ds = wfpt.RLRegDataset(rt, response, feedback, split, X, group_id=subj, n_groups=S)
        table = np.tile(COEF, (S, 1))
        params = np.tile([2.5, DDM["sv"], DDM["a"], DDM["z"], DDM["sz"], DDM["t"], DDM["st"],
                          P_OUTLIER], (S, 1))
        q, alpha = np.full(S, Q), np.full(S, ALPHA)
        lo = np.arange(S) * per
        for name in a.models:
            model = MODELS[name]
            multi = [m[0] for m in model]

            def groups():
                return ds.wiener_like_rl_reg_groups(model, table, q, alpha, params, **KNOBS)

            def today():
                v = X[:, 0:2] @ COEF[0:2]
                al = X[:, 2:4] @ COEF[2:4] if "alpha" in multi else None
                res = np.empty(S)
                for s in range(S):
                    sl = slice(lo[s], lo[s] + per)
                    res[s] = wfpt.wiener_like_multi_rlddm(
                        rt[sl], response[sl], feedback[sl], split[sl], Q, v[sl], DDM["sv"],
                        DDM["a"], DDM["z"], DDM["sz"], DDM["t"], DDM["st"],
                        ALPHA if al is None else al[sl], KNOBS["err"], multi=multi,
                        n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, p_outlier=P_OUTLIER,
                        w_outlier=KNOBS["w_outlier"])
                return res

            routes = {k: c for k, c in (("a_rl_reg_groups", groups), ("b_numpy_plus_multi_rlddm",
                                                                      today)) if k[0] in a.routes}
            sums = {k: call() for k, call in routes.items()}
            for call in routes.values():  # warm every shape
                for _ in range(5):
                    call()
            ms = {k: [] for k in routes}
            for _ in range(a.rounds):
                for k, call in routes.items():
                    ms[k].append(window(call, a.seconds))
            row = {"subjects": S, "trials_per_subject": per, "model": name, "routes": {}}
            for k, v in ms.items():
                row["routes"][k] = {"median_ms": float(np.median(v)),
                                    "spread_ms": float(max(v) - min(v)), "windows_ms": v}
            if "a" in a.routes:  # device time of the call's launches, HIP events
                ds.ctx.profile(ds.ctx.PROF_EVENTS)
                ds.ctx.profile_read(reset=True)
                for _ in range(50):
                    groups()
                dev_ms, launches, _ = ds.ctx.profile_read(reset=True)
                ds.ctx.profile(0)
                row["a_device_ms_per_call"] = dev_ms / 50
                row["a_profiled_brackets_per_call"] = launches / 50
            if len(sums) == 2:
                sa, sb = sums["a_rl_reg_groups"], sums["b_numpy_plus_multi_rlddm"]
                row["max_rel_diff_a_vs_b"] = float(np.max(np.abs(sa - sb) / np.abs(sb)))
                row["agree"] = row["max_rel_diff_a_vs_b"] < 1e-9
                row["ratio_b_over_a"] = (row["routes"]["b_numpy_plus_multi_rlddm"]["median_ms"]
                                         / row["routes"]["a_rl_reg_groups"]["median_ms"])
            out["rows"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "routes"}), flush=True)
            for k, v in row["routes"].items():
                print(json.dumps({"size": size, "model": name, "route": k,
                                  "median_ms": v["median_ms"], "spread_ms": v["spread_ms"]}),
                      flush=True)
            if row.get("agree") is False:
                raise SystemExit(f"bench_rl_reg: the routes differ by "
                                 f"{row['max_rel_diff_a_vs_b']} (relative) in a subject's sum")
        ds.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": a.out, "build": out["build"]}))


def merge_trace(a):
    with open(a.out) as fh:
        out = json.load(fh)
    for item in a.merge_trace:
        key, path = item.split("=", 1)
        size, name = key.split(":")
        S, per = (int(v) for v in size.split("x"))
        with open(path, newline="") as fh:
            rows = list(csv.DictReader(fh))
        kern = {}
        for k in KERNELS:
            hit = [r for r in rows if k in r["Name"]]
            if hit:
                kern[k] = {"average_us": sum(float(r["AverageNs"]) * int(r["Calls"]) for r in hit)
                           / sum(int(r["Calls"]) for r in hit) / 1e3,
                           "calls": sum(int(r["Calls"]) for r in hit)}
        for row in out["rows"]:
            if (row["subjects"], row["trials_per_subject"], row["model"]) == (S, per, name):
                row["kernels"] = kern
                print(json.dumps({"size": size, "model": name, **kern}))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", default=["40x300", "200x500"])
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--routes", default="ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rl_reg", "rows.json"))
    ap.add_argument("--merge-trace", nargs="+", metavar="SxT:MODEL=CSV")
    a = ap.parse_args()
    if a.merge_trace:
        merge_trace(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
