"""Generate tests/golden/drift.npz (run once, where the reference tree is).

hddm.generate._gen_rts_from_simulated_drift (hddm/generate.py:208-319) cannot
be imported (generate.py imports hddm -> PyMC / kabuki), so its definition is
taken out of the reference's generate.py with `ast` at run time and executed
in a namespace whose random sources record what they hand out:

  uniform.rvs(loc, scale, size)  loc + scale * u      (scipy's own arithmetic)
  norm.rvs(loc, scale)           loc + scale * n
  numpy.random.rand(nn)          the walk's uniforms

One call per trial (samples = 1). Per trial the fixture holds the parameters,
the uniforms and normals drawn, the start delay, start point and drift
rate(s) they give, the step outcomes rand < prob_up of every block the call
generated (packed bits; the crossing lies inside them) and the returned RT.

Usage: python tests/golden/make_golden_drift.py --reference <reference tree>
"""
import argparse
import ast
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DT, INTRA_SV, SEED = 1e-3, 1.0, 20261019
NAN = float("nan")
# (v, sv, a, z, sz, t, st), (v_switch, V_switch, t_switch) or None, trials
CASES = [
    ((0.5, 0.0, 2.0, 0.5, 0.0, 0.3, 0.0), None, 10),                  # plain
    ((0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1), None, 10),                  # sv, sz, st
    ((-1.2, 0.8, 1.4, 0.45, 0.25, 0.25, 0.1), None, 6),
    ((1.0, 0.0, 2.0, 0.5, 0.0, 0.3, 0.0), (-3.0, 0.0, 0.2), 6),       # switch at step 200
    ((0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1), (-1.0, 0.5, 0.005), 6),     # switch at step 5, V_switch
    ((0.5, 0.0, 0.1, 0.5, 0.8, 0.3, 0.0), None, 10),                  # a = 0.1: crossings from step 0 on
]


class Recorder:
    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.reset()

    def reset(self):
        self.uniforms, self.values, self.normals, self.drifts, self.walk = [], [], [], [], []

    # scipy.stats.uniform / norm stand-ins
    def uniform_rvs(self, loc=0, scale=1, size=1):
        u = self.rs.random_sample(size)
        self.uniforms.append(u)
        self.values.append(loc + scale * u)
        return self.values[-1]

    def norm_rvs(self, loc=0, scale=1):
        n = self.rs.standard_normal()
        self.normals.append(n)
        self.drifts.append(loc + scale * n)
        return self.drifts[-1]

    def rand(self, n):
        u = self.rs.random_sample(n)
        self.walk.append(u)
        return u


def load_reference_function(reference):
    path = os.path.join(reference, "hddm", "generate.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    fn = [n for n in tree.body
          if isinstance(n, ast.FunctionDef) and n.name == "_gen_rts_from_simulated_drift"]
    assert len(fn) == 1
    return compile(ast.Module(body=fn, type_ignores=[]), path, "exec")


def main(reference):
    rec = Recorder(SEED)
    ns = {"np": np,
          "uniform": type("uniform", (), {"rvs": staticmethod(rec.uniform_rvs)}),
          "norm": type("norm", (), {"rvs": staticmethod(rec.norm_rvs)})}
    exec(load_reference_function(reference), ns)
    simulate = ns["_gen_rts_from_simulated_drift"]
    cols = {k: [] for k in ("params", "switch", "u_t", "u_z", "n", "n_switch", "delay", "y0",
                            "drift", "drift_switch", "rt", "n_bits")}
    bits = []
    saved = np.random.rand
    np.random.rand = rec.rand  # generate.py:227 imports it inside the function
    try:
        for p, sw, trials in CASES:
            params = dict(zip(("v", "sv", "a", "z", "sz", "t", "st"), p))
            if sw is not None:
                params.update(zip(("v_switch", "V_switch", "t_switch"), sw))
            for _ in range(trials):
                rec.reset()
                rts, _ = simulate(params, 1, DT, INTRA_SV)
                v, sv, a, z, sz, t, st = p
                normals, drifts = list(rec.normals), list(rec.drifts)
                n = normals.pop(0) if sv != 0 else NAN
                drift = drifts.pop(0) if sv != 0 else v
                n_sw, drift_sw = NAN, NAN
                if sw is not None:
                    n_sw = normals.pop(0) if sw[1] != 0 else NAN
                    drift_sw = drifts.pop(0) if sw[1] != 0 else sw[0]
                assert not normals and len(rec.uniforms) == 2
                # generate.py:279, 284-287: the outcome of every uniform the call drew
                nn = int(round(sw[2] / DT)) if sw is not None else 1000
                ups = []
                for block, u in enumerate(rec.walk):
                    assert u.shape == (nn,)
                    d = drift_sw if (sw is not None and block >= 1) else drift
                    ups.append(u < 0.5 * (1 + np.sqrt(DT) / INTRA_SV * d))
                ups = np.concatenate(ups)
                cols["params"].append(p)
                cols["switch"].append(sw if sw is not None else (NAN, NAN, NAN))
                cols["u_t"].append(rec.uniforms[0][0])
                cols["u_z"].append(rec.uniforms[1][0])
                cols["n"].append(n)
                cols["n_switch"].append(n_sw)
                cols["delay"].append(rec.values[0][0] - st / 2.)      # generate.py:245-246
                cols["y0"].append((rec.values[1][0] - sz / 2.) * a)   # generate.py:252-253
                cols["drift"].append(drift)
                cols["drift_switch"].append(drift_sw)
                cols["rt"].append(rts[0])
                cols["n_bits"].append(ups.size)
                bits.append(ups)
    finally:
        np.random.rand = saved
    out = {k: np.array(v, dtype=np.int64 if k == "n_bits" else np.float64)
           for k, v in cols.items()}
    out["ups"] = np.packbits(np.concatenate(bits))
    out["dt"] = np.array(DT)
    out["intra_sv"] = np.array(INTRA_SV)
    path = os.path.join(HERE, "drift.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out["rt"]), "trials", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    main(ap.parse_args().reference)
