"""Call time of the RL likelihoods on one GPU, against the only route that
existed without them.

  1. resident `RLDataset.wiener_like_rlddm`: one node, 4 conditions x 75
     trials, full DDM, HDDM's knobs;
  2. `RLDataset.wiener_like_rlddm_nodes`: 40 copies of that node in one call;
     twice in a row, and `wiener_like_rlddm_nodes_multi` with T = 2 tables on
     the same data set (both stepping-out probes of a slice step in one call);
  3. emulation: the Q recurrence as a Python loop, then
     `Dataset.wiener_like_multi(multi=['v'])` on a resident input-order dataset
     of the scored trials (a Python loop plus an n-double upload per call).

Each figure is a host clock around calls that end in the library's wait for the
device's completion word, over enough repeats to fill --seconds; the kernel
time comes from the context's profile events in a pass of its own. Writes
profiles/rl/rows.json with the build digest.

    python tools/bench_rl.py [--seconds 0.5] [--out profiles/rl/rows.json]
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

E = 2.718281828459
ROW = (0.5, -1.2, 0.4)  # q, alpha, pos_alpha
DDM = dict(v=2.4, sv=0.1, a=2.0, z=0.5, sz=0.1, t=0.3, st=0.1)
KNOBS = dict(n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, p_outlier=0.05, w_outlier=0.1)
ERR = 1e-4


def node_data(seed, conditions=4, per=75):
    rng = np.random.default_rng(seed)
    n = conditions * per
    split_by = np.repeat(np.arange(conditions, dtype=np.int64), per)
    rng.shuffle(split_by)
    x = np.sign(rng.uniform(-0.4, 0.6, n)) * (0.35 + rng.gamma(2.0, 0.4, n))
    response = (x > 0).astype(np.int64)
    feedback = (rng.uniform(size=n) < np.where(response == 1, 0.7, 0.35)).astype(np.float64)
    return x, response, feedback, split_by


def python_drift(response, feedback, split_by, q, alpha, pos_alpha, v):
    """The recurrence of wfpt.pyx:111-153 on the host: (drift, scored mask)."""
    n = len(response)
    drift = np.zeros(n)
    scored = np.zeros(n, dtype=bool)
    pos_alfa = alpha if pos_alpha == 100.0 else pos_alpha
    a_neg = (E ** alpha) / (1 + E ** alpha)
    a_pos = (E ** pos_alfa) / (1 + E ** pos_alfa)
    for s in np.unique(split_by):
        qs = [q, q]
        for k, i in enumerate(np.nonzero(split_by == s)[0]):
            drift[i] = (qs[1] - qs[0]) * v
            scored[i] = k > 0
            r, f = int(response[i]), float(feedback[i])
            qs[r] = qs[r] + (a_pos if f > qs[r] else a_neg) * (f - qs[r])
    return drift, scored


def timed(call, seconds):
    """(ms per call, repeats): repeats doubled until the window fills `seconds`."""
    call()
    call()
    reps = 8
    while True:
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        el = time.perf_counter() - t0
        if el >= seconds:
            return el / reps * 1e3, reps
        reps *= 2


def kernel_ms(ctx, call, reps=50):
    ctx.profile(1)
    ctx.profile_read(reset=True)
    for _ in range(reps):
        call()
    ms, launches, _ = ctx.profile_read(reset=True)
    ctx.profile(0)
    return ms / max(launches, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--nodes", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rl", "rows.json"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_rl: no HIP device")
    ctx = _lib.context()
    x, response, feedback, split_by = node_data(7)
    args = (*ROW, DDM["v"], DDM["sv"], DDM["a"], DDM["z"], DDM["sz"], DDM["t"], DDM["st"], ERR)

    one = wfpt.RLDataset(x, response, feedback, split_by)
    call1 = lambda: one.wiener_like_rlddm(*args, **KNOBS)

    m = a.nodes
    node = np.repeat(np.arange(m, dtype=np.int32), x.size)
    batch = wfpt.RLDataset(np.tile(x, m), np.tile(response, m), np.tile(feedback, m),
                           np.tile(split_by, m), node_id=node, n_nodes=m)
    rows = np.tile(np.array(ROW), (m, 1))
    params = np.tile(np.array([DDM[k] for k in ("v", "sv", "a", "z", "sz", "t", "st")] +
                              [KNOBS["p_outlier"]]), (m, 1))
    nk = dict(err=ERR, n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3, w_outlier=0.1)
    call2 = lambda: batch.wiener_like_rlddm_nodes(rows, params, **nk)
    # two probes of a slice step: two one-table calls, or one two-table call
    rows2 = np.stack([rows, rows + np.array([0.0, 0.3, 0.0])])
    params2 = np.stack([params, params])

    def call2_twice():
        return np.stack([batch.wiener_like_rlddm_nodes(rows2[0], params2[0], **nk),
                         batch.wiener_like_rlddm_nodes(rows2[1], params2[1], **nk)])

    call2_multi = lambda: batch.wiener_like_rlddm_nodes_multi(rows2, params2, **nk)

    _, scored = python_drift(response, feedback, split_by, *ROW, DDM["v"])
    emu = wfpt.Dataset(x[scored], input_order=True)

    def call3():
        drift, sc = python_drift(response, feedback, split_by, *ROW, DDM["v"])
        return emu.wiener_like_multi(drift[sc], DDM["sv"], DDM["a"], DDM["z"], DDM["sz"],
                                     DDM["t"], DDM["st"], ERR, ["v"], **KNOBS)

    v1, v2, v3 = call1(), call2(), call3()
    same = bool(np.all(v2 == v1))
    multi_same = bool(np.array_equal(call2_multi(), call2_twice()))
    out = {"build": hb.built_digest(_lib.LIB_PATH), "source": hb.source_digest(),
           "trials_per_node": int(x.size), "nodes": m, "seconds": a.seconds,
           "logp": {"resident": v1, "emulated": v3, "batch_equals_resident": same,
                    "multi_equals_two_calls": multi_same}, "rows": []}
    for name, call in (("resident_rlddm_1_node", call1), (f"node_batch_{m}_nodes", call2),
                       (f"node_batch_{m}_nodes_two_calls", call2_twice),
                       (f"node_batch_multi_{m}_nodes_T2", call2_multi),
                       ("python_scan_plus_multi", call3)):
        ms, reps = timed(call, a.seconds)
        out["rows"].append({"call": name, "call_ms": ms, "repeats": reps,
                            "kernel_ms": kernel_ms(ctx, call)})
        print(json.dumps(out["rows"][-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "build": out["build"]}))


if __name__ == "__main__":
    main()
