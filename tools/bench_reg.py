"""Call time of the regression likelihoods on one GPU, against the only route
that existed without them.

Workloads: S subjects x 500 trials (S = 20 and 200), model v ~ 1 + cov +
C(cond) (identity link), full DDM with sv = sz = st = 0.1, HDDM's knobs,
p_outlier 0.05. Routes:

  a. `RegDataset.wiener_like_reg`: one coefficient vector, the sum over all
     trials (the reference's wfpt_reg node);
  b. `RegDataset.wiener_like_reg_groups`: one sum per subject;
  c. the earlier route: `X @ b` in NumPy, then
     `Dataset.wiener_like_multi(multi=['v'])` on a resident input-order data
     set (an n-double upload per call).

Each figure is a host clock around calls that end in the library's wait for
the device's completion word; every shape is warmed up; a window lasts at
least --seconds; the routes alternate in one process for --rounds rounds and
each route's median and spread (max - min) over the rounds are reported. The
per-trial terms of (a) and (c) are compared in the same run (max|dlogp| <
1e-6: `X @ b` is another summation order than the device's).

    python tools/bench_reg.py [--seconds 0.5] [--rounds 5] [--subjects 20 200]
                              [--routes abc] [--out profiles/reg/rows.json]
    python tools/bench_reg.py --merge-trace 20=stats.csv 200=stats.csv --out ...

--merge-trace adds reg_fill_kernel's average time from `rocprofv3
--kernel-trace --stats --output-format csv` runs of their own (one per size,
started with --subjects S --routes a, so that every traced launch is route
(a)'s) to an existing rows file, next to the bytes the kernel moves (n x
columns read + n x arrays written, 8 B each) and the fraction of the HBM peak
that is.
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

MODEL = [("v", 0, 4, "identity")]
COEF = np.array([0.7, 0.45, -0.3, 0.25])
DDM = dict(sv=0.1, a=2.0, z=0.5, sz=0.1, t=0.3, st=0.1)
KNOBS = dict(n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, p_outlier=0.05, w_outlier=0.1)
ERR = 1e-4
PER = 500
HBM_PEAK = 8.0e12  # B/s, MI355X data sheet


def workload(subjects, seed=11):
    rng = np.random.default_rng(seed)
    n = subjects * PER
    subj = np.repeat(np.arange(subjects, dtype=np.int32), PER)
    cov = rng.normal(size=n)
    cond = rng.integers(0, 3, size=n)
    X = np.ascontiguousarray(np.column_stack([np.ones(n), cov, cond == 1, cond == 2]),
                             dtype=np.float64)
    rt = (DDM["t"] + 0.1 + rng.gamma(2.0, 0.3, n)) * rng.choice([-1.0, 1.0], n, p=[0.25, 0.75])
    return rt, X, subj


def window(call, seconds):
    """ms per call over one window of at least `seconds`."""
    reps = 8
    while True:
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        el = time.perf_counter() - t0
        if el >= seconds:
            return el / reps * 1e3
        reps *= 2


def fill_bytes(n):
    cols = sum(m[2] for m in MODEL)
    return n * 8 * (cols + len(MODEL))


def measure(a):
    from hddm_amd import _lib, build as hb, wfpt
    if _lib.device_count() < 1:
        raise SystemExit("bench_reg: no HIP device")
    out = {"build": hb.built_digest(_lib.LIB_PATH), "source": hb.source_digest(),
           "trials_per_subject": PER, "seconds": a.seconds, "rounds": a.rounds, "sizes": []}
    for S in a.subjects:
        rt, X, subj = workload(S)
        n = rt.size
        ds = wfpt.RegDataset(rt, X, group_id=subj, n_groups=S)
        plain = wfpt.Dataset(rt, input_order=True)
        args = (0.0, DDM["sv"], DDM["a"], DDM["z"], DDM["sz"], DDM["t"], DDM["st"], ERR)
        table = np.tile(COEF, (S, 1))
        params = np.tile([0.0, DDM["sv"], DDM["a"], DDM["z"], DDM["sz"], DDM["t"], DDM["st"],
                          KNOBS["p_outlier"]], (S, 1))
        gk = dict(err=ERR, n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, w_outlier=0.1)
        routes = {
            "a_wiener_like_reg": lambda: ds.wiener_like_reg(MODEL, COEF, *args, **KNOBS),
            "b_wiener_like_reg_groups": lambda: ds.wiener_like_reg_groups(MODEL, table, params,
                                                                          **gk),
            "c_numpy_plus_multi": lambda: plain.wiener_like_multi(
                X @ COEF, DDM["sv"], DDM["a"], DDM["z"], DDM["sz"], DDM["t"], DDM["st"], ERR,
                ["v"], **KNOBS),
        }
        total_a, terms_a, _ = ds.wiener_like_reg(MODEL, COEF, *args, **KNOBS, terms=True)
        total_c, terms_c = plain.wiener_like_multi(
            X @ COEF, DDM["sv"], DDM["a"], DDM["z"], DDM["sz"], DDM["t"], DDM["st"], ERR, ["v"],
            **KNOBS, trials=True)
        dmax = float(np.max(np.abs(terms_a - terms_c)))
        sums_b = routes["b_wiener_like_reg_groups"]() if "b" in a.routes else None
        routes = {k: call for k, call in routes.items() if k[0] in a.routes}
        for call in routes.values():  # warm every shape
            for _ in range(20):
                call()
        ms = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, call in routes.items():
                ms[k].append(window(call, a.seconds))
        row = {"subjects": S, "trials": int(n), "logp_a": total_a, "logp_c": total_c,
               "logp_b_sum": None if sums_b is None else float(np.sum(sums_b)),
               "max_abs_dlogp_a_vs_c": dmax,
               "agree": dmax < 1e-6, "fill_bytes": fill_bytes(n), "routes": {}}
        for k, v in ms.items():
            row["routes"][k] = {"median_ms": float(np.median(v)),
                                "spread_ms": float(max(v) - min(v)), "windows_ms": v}
        if "a" in a.routes and "c" in a.routes:
            ra, rc = row["routes"]["a_wiener_like_reg"], row["routes"]["c_numpy_plus_multi"]
            row["a_below_c_by_more_than_c_spread"] = bool(
                ra["median_ms"] < rc["median_ms"] - rc["spread_ms"])
        out["sizes"].append(row)
        print(json.dumps({k: row[k] for k in row if k != "routes"}), flush=True)
        for k, v in row["routes"].items():
            print(json.dumps({"subjects": S, "route": k, "median_ms": v["median_ms"],
                              "spread_ms": v["spread_ms"]}), flush=True)
        if not row["agree"]:
            raise SystemExit(f"bench_reg: routes a and c differ by {dmax} per trial")
        ds.close()
        plain.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": a.out, "build": out["build"]}))


def merge_trace(a):
    with open(a.out) as fh:
        out = json.load(fh)
    for item in a.merge_trace:
        S, path = item.split("=", 1)
        with open(path, newline="") as fh:
            rows = [r for r in csv.DictReader(fh) if "reg_fill_kernel" in r["Name"]]
        if len(rows) != 1:
            raise SystemExit(f"bench_reg: {path} has {len(rows)} reg_fill_kernel rows")
        avg_ns = float(rows[0]["AverageNs"])
        for row in out["sizes"]:
            if row["subjects"] == int(S):
                bw = row["fill_bytes"] / (avg_ns * 1e-9)
                row["reg_fill_kernel"] = {
                    "average_us": avg_ns / 1e3, "min_us": float(rows[0]["MinNs"]) / 1e3,
                    "calls": int(rows[0]["Calls"]), "bytes": row["fill_bytes"],
                    "bytes_per_s": bw, "fraction_of_hbm_peak": bw / HBM_PEAK}
                print(json.dumps({"subjects": int(S), **row["reg_fill_kernel"]}))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--subjects", type=int, nargs="+", default=[20, 200])
    ap.add_argument("--routes", default="abc",
                    help="the routes to time (a trace of reg_fill_kernel alone: --routes a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reg", "rows.json"))
    ap.add_argument("--merge-trace", nargs="+", metavar="S=CSV")
    a = ap.parse_args()
    if a.merge_trace:
        merge_trace(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
