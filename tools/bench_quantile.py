"""Quantile objectives on the GPU: one dmat_cdf_rows launch over R rows against
one dmat_cdf_array call per row (the path before the row kernel), then
HDDM.optimize('gsquare') and its bootstrap end to end.

    python tools/bench_quantile.py [--out profiles/quantile/rows.json] [--bootstraps 200]

Rows: full-DDM parameter rows jittered around (0.5, 0.5, 2.0, 0.5, 0.2, 0.3,
0.15), E = 11 edges from quantile_stats of RTs sampled at each distinct row.
Per R the two paths alternate, repetition by repetition, inside one process;
each figure is the median wall time of a call that ends in a device
synchronise, with the spread (min .. max) next to it. The objective values of
the two paths are compared before anything is timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hddm_amd import _lib, cdfdif_wrapper as cw, wfpt  # noqa: E402
from hddm_amd.hierarchical import HDDM, gen_data  # noqa: E402
from hddm_amd.quantiles import quantile_stats  # noqa: E402

W_OUTLIER = 0.1
BASE = np.array([0.5, 0.5, 2.0, 0.5, 0.2, 0.3, 0.15, 0.05])
DISTINCT = 16


def make_rows(R, seed=1):
    """R rows cycling through DISTINCT sampled (parameters, statistics)."""
    rng = np.random.default_rng(seed)
    np.random.seed(seed)
    P, X, F, N = [], [], [], []
    for _ in range(min(R, DISTINCT)):
        p = BASE.copy()
        p[[0, 2, 5]] *= 1 + 0.1 * rng.uniform(-1, 1, 3)
        rt = wfpt.gen_rts_from_cdf(*p[:7], samples=500, dt=1e-3)
        s = quantile_stats(rt[np.abs(rt) < 4.99])
        P.append(p)
        X.append(s["emp_rt"])
        F.append(s["freq_obs"])
        N.append(float(s["n_samples"]))
    src = np.arange(R) % len(P)
    # the optimiser moves the parameters on every evaluation: a small offset per row
    P = np.array(P)[src]
    P[:, 0] += 1e-3 * rng.standard_normal(R)
    return P, np.array(X)[src], np.array(F)[src], np.array(N)[src]


def per_row(P, X, F, N):
    """One dmat_cdf_array call per row and the reference's NumPy lines on its
    result (likelihoods.py:203-213, 239)."""
    out = 0.0
    for r in range(P.shape[0]):
        cdf = cw.dmat_cdf_array(X[r], *P[r], W_OUTLIER)
        prop = np.diff(np.concatenate((np.array([0.]), cdf, np.array([1.]))))
        prop[prop <= 1e-6] = 1e-6
        out += -2 * np.sum(F[r] * np.log(prop))
    return out


def batched(P, X, F, N):
    return float(np.sum(-cw.dmat_cdf_rows(X, P, W_OUTLIER, F, N)[2]))


def spread(ts):
    ts = np.sort(ts)
    return {"median_ms": float(np.median(ts) * 1e3), "min_ms": float(ts[0] * 1e3),
            "max_ms": float(ts[-1] * 1e3), "reps": int(ts.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile", "rows.json"))
    ap.add_argument("--bootstraps", type=int, default=200)
    ap.add_argument("--sizes", default="1,4,64,2000,20000")
    a = ap.parse_args()
    ctx = _lib.context(0)
    rows = []
    for R in (int(s) for s in a.sizes.split(",")):
        P, X, F, N = make_rows(R)
        base_reps = 3 if R >= 2000 else (20 if R >= 64 else 100)
        rel = abs(batched(P, X, F, N) - per_row(P, X, F, N)) / abs(batched(P, X, F, N))
        assert rel < 1e-12, rel
        batched(P, X, F, N)  # both warm
        tb, tr = [], []
        for _ in range(base_reps):  # interleaved
            t0 = time.perf_counter()
            batched(P, X, F, N)
            t1 = time.perf_counter()
            per_row(P, X, F, N)
            t2 = time.perf_counter()
            tb.append(t1 - t0)
            tr.append(t2 - t1)
        ctx.profile(1)
        ctx.profile_read(reset=True)
        batched(P, X, F, N)
        k_ms, nl, _ = ctx.profile_read(reset=True)
        ctx.profile(0)
        row = {"R": R, "E": 11, "batched": spread(tb), "per_row_calls": spread(tr),
               "batched_kernel_ms": k_ms / max(nl, 1),
               "speedup_median": float(np.median(tr) / np.median(tb)),
               "objective_rel_diff": float(rel)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    # end to end: the single-subject set of tests/test_optimize.py
    data, tr = gen_data(n_subj=1, n_trials=2000, conds={"c0": 0.5, "c1": 1.5}, a=2.0, t=0.3,
                        seed=20261020)
    start = {"a": tr["a"][0], "t": tr["t"][0], "v(c0)": tr["v"]["c0"][0], "v(c1)": tr["v"]["c1"][0]}
    fits = {}
    for label, kw in (("optimize_gsquare", {}),
                      (f"optimize_gsquare_bootstrap_{a.bootstraps}",
                       {"n_bootstraps": a.bootstraps, "seed": 1})):
        m = HDDM(data, depends_on={"v": "cond"}, seed=3, p_outlier=0.0)
        m.set_values(start)
        t0 = time.perf_counter()
        res = m.optimize("gsquare", **kw)
        fits[label] = {"seconds": time.perf_counter() - t0, "result": res}
        if kw:
            fits[label]["bootstrap_std"] = m.bootstrap_stats.loc["std"].to_dict()
        print(json.dumps({label: fits[label]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"rows": rows, "fits": fits, "w_outlier": W_OUTLIER,
                   "base_row": BASE.tolist()}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
