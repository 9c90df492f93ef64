"""The model-comparison pass on one GPU: the device reduction over sweeps
against what a user could do without it.

  device  `Dataset.pointwise_nodes`: the S sweeps scored in tiles, each tile's
          per-trial terms folded into the per-trial state by one kernel; four
          numbers per trial are copied out
  host    `Dataset.wiener_like_nodes_multi(trials=True)` per tile of the same
          size (the S x n terms copied out tile by tile), and the same
          reduction in NumPy: a streaming log-sum-exp and a pairwise merge of
          the tiles' means and sums of squares

Shape: config 4's full DDM, 400 nodes x 250 trials (hierarchical.gen_data),
`--sweeps` kept sweeps of parameters jittered around the generating values (the
traces are made up: only their shape matters here). After a warm-up call of
each at that shape the two paths alternate on the same device, `--rounds` times
each; the figures are host clocks around whole calls that end in a stream wait
(median over the rounds). Kernel times
come from the context's profile events in a pass of their own: the scoring
kernels of every tile, and the accumulate kernel. Writes one row per sweep
count to profiles/pointwise/rows.json with the build digest.

    python tools/bench_pointwise.py [--sweeps 500 2000] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hddm_amd import _lib, build as hb  # noqa: E402
from hddm_amd.hierarchical import HDDM, gen_data  # noqa: E402

WORKSPACE = 1 << 30  # the pass's default tile budget


def model_config4(sweeps, n_subj, n_trials, seed=20261021):
    inter = dict(sv=0.1, sz=0.1, st=0.1)
    data, _ = gen_data(n_subj=n_subj, n_trials=n_trials, **inter)
    m = HDDM(data, depends_on={"v": "cond"}, include=tuple(inter), seed=0)
    rng = np.random.default_rng(seed)
    jit = lambda size, rel: 1 + rel * rng.uniform(-1, 1, size)
    m.trace_subj = {"a": 2.0 * jit((sweeps, m.n_units["a"]), 0.1),
                    "v": 0.75 * jit((sweeps, m.n_units["v"]), 0.4),
                    "t": 0.3 * jit((sweeps, m.n_units["t"]), 0.1)}
    m.trace = {k: v * jit(sweeps, 0.3) for k, v in inter.items()}
    return m


def host_route(ds, tables, wp, tile):
    """The parent commit's route: the terms of every tile on the host, reduced
    there. Returns (sums, lppd, p_waic, mean)."""
    S, n = tables.shape[0], ds.n
    m = np.full(n, -np.inf)
    r = np.zeros(n)
    mean = np.zeros(n)
    M2 = np.zeros(n)
    seen, sums = 0, []
    for s0 in range(0, S, tile):
        out, terms = ds.wiener_like_nodes_multi(tables[s0:s0 + tile], trials=True, **wp)
        sums.append(out)
        T = terms.shape[0]
        m_new = np.maximum(m, terms.max(axis=0))
        r = r * np.exp(m - m_new) + np.exp(terms - m_new).sum(axis=0)
        m = m_new
        t_mean = terms.mean(axis=0)
        t_M2 = ((terms - t_mean) ** 2).sum(axis=0)
        d = t_mean - mean
        M2 = M2 + t_M2 + d * d * (seen * T / (seen + T))
        mean = mean + d * (T / (seen + T))
        seen += T
    return np.concatenate(sums), m + np.log(r) - np.log(S), M2 / max(S - 1, 1), mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, nargs="+", default=[500, 2000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--subjects", type=int, default=200)
    ap.add_argument("--trials", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointwise", "rows.json"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_pointwise: no HIP device")
    ctx = _lib.context()
    m = model_config4(max(a.sweeps), a.subjects, a.trials)
    ds, wp = m.dataset, m.wp
    all_tables = m._pw_ddm_table(np.arange(max(a.sweeps)))
    rows = []
    for S in a.sweeps:
        tables = np.ascontiguousarray(all_tables[:S])
        tile = max(1, min(S, WORKSPACE // (8 * ds.n)))
        # warm-up at this shape: the workspaces grow with the tile
        ds.pointwise_nodes(tables, max_workspace=WORKSPACE, **wp)
        host_route(ds, tables, wp, tile)
        td, th = [], []
        for r in range(a.rounds):  # alternating
            t0 = time.perf_counter()
            pw = ds.pointwise_nodes(tables, max_workspace=WORKSPACE, **wp)
            t1 = time.perf_counter()
            ref = host_route(ds, tables, wp, tile)
            t2 = time.perf_counter()
            td.append((t1 - t0) * 1e3)
            th.append((t2 - t1) * 1e3)
            print(json.dumps({"sweeps": S, "round": r, "device_ms": td[-1], "host_ms": th[-1]}),
                  flush=True)
        rel = lambda got, want: float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
        ctx.profile(1)
        ctx.profile_read(reset=True)
        ctx.pointwise_profile(reset=True)
        ds.pointwise_nodes(tables, max_workspace=WORKSPACE, **wp)
        score_ms, launches, _ = ctx.profile_read(reset=True)
        acc_ms = ctx.pointwise_profile(reset=True)
        ctx.profile(0)
        rows.append({"sweeps": S, "nodes": m.n_nodes, "trials": int(ds.n), "tile_sweeps": tile,
                     "tiles": launches, "rounds": a.rounds,
                     "device_ms": float(np.median(td)), "host_ms": float(np.median(th)),
                     "device_ms_all": td, "host_ms_all": th,
                     "speedup": float(np.median(th) / np.median(td)),
                     "scoring_kernel_ms": score_ms, "accumulate_kernel_ms": acc_ms,
                     "accumulate_share_of_kernel_time": acc_ms / (acc_ms + score_ms),
                     "term_bytes_not_copied": int(8 * S * ds.n),
                     "sums_equal_host_route": bool(np.array_equal(pw["sums"], ref[0])),
                     "lppd_max_diff": rel(pw["lppd"], ref[1]),
                     "p_waic_max_diff": rel(pw["p_waic"], ref[2]),
                     "mean_max_diff": rel(pw["mean"], ref[3]),
                     "n_inf_total": pw["n_inf_total"]})
        print(json.dumps(rows[-1]), flush=True)
    out = {"build": hb.built_digest(_lib.LIB_PATH), "source": hb.source_digest(), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "build": out["build"]}))


if __name__ == "__main__":
    main()
