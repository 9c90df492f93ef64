"""Digest of short seeded chains of every sampler, on the CPU.

    python tools/chain_digest.py > before.jsonl    # on the parent commit
    python tools/chain_digest.py > after.jsonl     # on the branch
    cmp before.jsonl after.jsonl

Each model's chain is a function of its seed. This tool runs HDDM, HDDMChains,
HDDMRegressor and HDDMrl over the oracle-backed stand-ins of the resident data
sets that the tests define (tests/test_hierarchical.py::_OracleDataset,
tests/test_regressor.py::_OracleRegDataset, tests/test_hddmrl.py::_OracleRLDataset),
so it needs no GPU, and prints one
JSON line per model: the trace keys in order, the number of likelihood calls
and a SHA-256 over the traces, the subject traces, the generator's state after
sampling, the call_stats keys with their counts and logp() at the final state
(`sha256`; `sha256_chain` is the same without logp(), which no sampler reads,
and `logp` its value, so a change to logp() alone shows as such).
A change to the samplers that is meant to leave the chains alone gives
byte-identical output before and after, on one machine: the digests depend on
the machine's libm, so they are compared, never stored.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def digest(m):
    """(sha256 of the chain alone, sha256 of the chain and logp(), logp())."""
    h = hashlib.sha256()
    for part in (m.trace, m.trace_subj):
        for k, v in part.items():
            h.update(k.encode())
            h.update(str((v.dtype, v.shape)).encode())
            h.update(np.ascontiguousarray(v).tobytes())
    h.update(repr(m.rng.bit_generator.state).encode())
    h.update(repr([(k, c) for k, (c, _) in m.call_stats.items()]).encode())
    chain = h.hexdigest()
    logp = np.asarray(m.logp(), dtype=np.float64)
    h.update(logp.tobytes())
    return chain, h.hexdigest(), logp.tolist()


def main():
    import oracle
    oracle.build()
    import test_hierarchical as th
    import test_regressor as tr
    from hddm_amd import hierarchical as h, regression as r
    h._wfpt.Dataset = th._OracleDataset
    r._wfpt.RegDataset = tr._OracleRegDataset
    data = th._cpu_data(n=40)
    runs = []
    for include in ((), ("sv", "sz", "st")):
        for paired in (True, False):
            runs.append((f"HDDM include={list(include)} paired_probes={paired}",
                         lambda include=include, paired=paired: h.HDDM(
                             data, depends_on={"v": "cond"}, include=include, seed=0,
                             paired_probes=paired),
                         dict(iter=6, burn=1, thin=2)))
    runs.append(("HDDMChains chains=3 include=['sz', 'st']",
                 lambda: h.HDDMChains(data, chains=3, include=("sz", "st"), seed=0),
                 dict(iter=6, burn=1, thin=2)))
    runs.append(("HDDMChains chains=1 depends_on v,a paired_probes=False",
                 lambda: h.HDDMChains(data, chains=1, depends_on={"v": "cond", "a": "cond"},
                                      paired_probes=False, seed=0),
                 dict(iter=4)))
    reg_data = tr._cpu_data()
    for group_only in (True, False):
        runs.append((f"HDDMRegressor group_only_regressors={group_only}",
                     lambda group_only=group_only: r.HDDMRegressor(
                         reg_data, tr.MODELS, include=("st",), group_only_regressors=group_only,
                         seed=0),
                     dict(iter=5, burn=1)))
    import test_hddmrl as trl
    from hddm_amd import rl
    rl._wfpt.RLDataset = trl._OracleRLDataset
    rl_data, _ = trl._cpu_data()
    rl_runs = [dict(dual=dual, paired_probes=paired) for dual in (False, True)
               for paired in (True, False)] + [dict(include=("sz", "st"))]
    for kw in rl_runs:
        runs.append(("HDDMrl " + " ".join(f"{k}={list(v) if k == 'include' else v}"
                                          for k, v in kw.items()),
                     lambda kw=kw: rl.HDDMrl(rl_data, seed=0, **kw), dict(iter=5, burn=1)))
    for name, make, how in runs:
        m = make()
        m.sample(**how)
        calls = m.likelihood_calls
        chain, full, logp = digest(m)
        print(json.dumps({"model": name, "trace_keys": list(m.trace), "likelihood_calls": calls,
                          "sha256": full, "sha256_chain": chain, "logp": logp}), flush=True)


if __name__ == "__main__":
    main()
