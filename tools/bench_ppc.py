"""Posterior-predictive data generation on one GPU: the batched sampler
against the loop of single-row calls it replaces.

  batched   one `wfpt.gen_rts_from_cdf_nodes` call over all rows (grid, CDF
            and search on the device, Philox uniforms)
  loop      one `wfpt.gen_rts_from_cdf` call per row (the density grid on the
            device, running sum / search / delays in NumPy): what
            `hierarchical.gen_data` and a per-node random() do

Two shapes, 400 rows x 250 samples of config 4's truth-like parameters
(hierarchical.gen_data's jitter) with sz = 0.1: dt = 1e-3 over (-6, 6), and
the stochastic's default grid dt = 1e-4 over (-5, 5). The two calls alternate
on the same device, `--rounds` times each; the figures are host clocks around
the whole call (median over the rounds). The per-stage kernel times come from
the context's profile events in a pass of its own. Writes profiles/ppc/rows.json
with the build digest.

    python tools/bench_ppc.py [--rounds 3] [--out profiles/ppc/rows.json]
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

SHAPES = [("dt1e-3", -6, 6, 1e-3), ("class_default_dt1e-4", -5, 5, 1e-4)]


def rows_config4(n_subj=200, jitter=0.1, seed=20261017):
    """(2 n_subj, 7) rows like hierarchical.gen_data's subjects (two drift
    conditions each), with sz = 0.1."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_subj):
        a = 2.0 * (1 + jitter * rng.uniform(-1, 1))
        t = 0.3 * (1 + jitter * rng.uniform(-1, 1))
        for v in (0.5, 1.0):
            out.append((v * (1 + jitter * rng.uniform(-1, 1)), 0.0, a, 0.5, 0.1, t, 0.0))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=400)
    ap.add_argument("--samples", type=int, default=250)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppc", "rows.json"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_ppc: no HIP device")
    ctx = _lib.context()
    P = rows_config4(a.rows // 2)
    R, n = P.shape[0], a.samples
    out = {"build": hb.built_digest(_lib.LIB_PATH), "source": hb.source_digest(), "rows": R,
           "samples_per_row": n, "rounds": a.rounds, "shapes": []}
    for name, lb, ub, dt in SHAPES:
        batched = lambda: wfpt.gen_rts_from_cdf_nodes(P, n, lb, ub, dt, seed=1)

        def loop():
            np.random.seed(1)
            return [wfpt.gen_rts_from_cdf(*row, samples=n, cdf_lb=lb, cdf_ub=ub, dt=dt)
                    for row in P]
        batched()  # warm-up: workspaces, code objects
        wfpt.gen_rts_from_cdf(*P[0], samples=n, cdf_lb=lb, cdf_ub=ub, dt=dt)
        tb, tl = [], []
        for _ in range(a.rounds):  # alternating
            t0 = time.perf_counter()
            batched()
            t1 = time.perf_counter()
            loop()
            t2 = time.perf_counter()
            tb.append((t1 - t0) * 1e3)
            tl.append((t2 - t1) * 1e3)
        ctx.profile(1)
        ctx.profile_stages(reset=True)
        batched()
        stages = ctx.profile_stages(reset=True)
        # the same densities on the path pdf_array / wiener_like take (lean
        # level-0 pass): a resident dataset of 16 rows' grid points, one row's
        # parameters, kernel time from the same events
        x = np.arange(lb, ub, dt)
        G = x.shape[0]
        ds = wfpt.Dataset(np.tile(x[1:], 16))
        v, sv, aa, z, sz = P[0][:5]
        lean = lambda: ds.wiener_like(v, sv, aa, z, sz, 0.0, 0.0, 1e-4, 2, 2, 1, 1e-3, 0.0, 0.0)
        lean()
        lean()
        ctx.profile_read(reset=True)
        lean()
        lean_ms = ctx.profile_read(reset=True)[0]
        ds.close()
        ctx.profile(0)
        row = {"shape": name, "grid_points": G, "batched_ms": float(np.median(tb)),
               "loop_ms": float(np.median(tl)), "batched_ms_all": tb, "loop_ms_all": tl,
               "speedup": float(np.median(tl) / np.median(tb)), "stage_kernel_ms": stages,
               "density_ns_per_point": stages["density"] * 1e6 / (R * (G - 1)),
               "lean_path_ns_per_point": lean_ms * 1e6 / (16 * (G - 1))}
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "build": out["build"]}))


if __name__ == "__main__":
    main()
