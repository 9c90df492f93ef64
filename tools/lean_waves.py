"""Per-wave clocks of lean_kernel on bench.py's C3 call (diagnostic build with
WFPT_PHASE_TIMING: `python tools/ab_variants.py build --names phase`, run with
WFPT_AMD_LIB=hddm_amd/lib/variants/libwfpt_phase.so).

Prints the launch's span, the wave-duration distribution by position in the
dataset (deciles of the chunk id: |rt| ascending within each boundary), the
number of waves in flight over time (the dispatch rounds and the tail), the
per-XCD end times, and the end of the launch: the time of the last dispatch
(the latest wave start), the 32 last-ending waves (chunk id, the wave of the
grid that took it = its position in dispatch order, the site each took: 0 uniform by the table, 1 uniform by the
vote, 2 generic) and the end of the last uniform wave. `--out FILE` also
writes the record to FILE.

    WFPT_AMD_LIB=hddm_amd/lib/variants/libwfpt_phase.so python tools/lean_waves.py
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_PHASE = 16384  # wfpt_internal.h kPhaseWaves


def main():
    import bench
    from hddm_amd import _lib, wfpt
    ctx = _lib.context(0)
    x = bench.make_rts(1_000_000, 20261015)
    ds = wfpt.Dataset(x)
    args, kn = bench.args_tuple(), bench.knobs_tuple()
    for _ in range(3):
        ds.wiener_like(*args, *kn)
    ctx.synchronize()
    assert ctx.last_path() & _lib.PATH_LEAN
    buf = (ctypes.c_uint64 * (K_PHASE * 8))()
    _lib.check(_lib.wfpt_debug_waves(ctx.handle, buf, K_PHASE))
    r = np.frombuffer(buf, dtype=np.uint64).reshape(K_PHASE, 8).astype(np.int64)
    nw = (len(ds) + 63) // 64
    r = r[:nw]
    t0 = r[:, 0].min()
    st = (r[:, 0] - t0) / 100.0  # us (100 MHz)
    en = (r[:, 1] - t0) / 100.0
    du = en - st
    xcc = r[:, 3] & 0xf
    out = {"waves": int(nw), "span_us": float(en.max()),
           "dur_median_us": float(np.median(du)), "dur_p90_us": float(np.quantile(du, 0.9)),
           "dur_max_us": float(du.max())}
    dec = np.array_split(np.arange(nw), 10)
    out["dur_median_by_decile_us"] = [round(float(np.median(du[d])), 1) for d in dec]
    out["start_median_by_decile_us"] = [round(float(np.median(st[d])), 1) for d in dec]
    # waves in flight over time
    grid = np.arange(0.0, en.max() + 1.0, 1.0)
    live = np.array([int(((st <= t) & (en > t)).sum()) for t in grid])
    peak = int(live.max())
    out["in_flight_peak"] = peak
    out["in_flight_every_5us"] = [int(v) for v in live[::5]]
    half = np.flatnonzero(live >= peak / 2)
    out["time_below_half_peak_at_end_us"] = float(en.max() - grid[half[-1]]) if half.size else None
    out["mean_in_flight_over_span"] = float(live.mean())
    out["xcc_last_end_us"] = {int(k): round(float(en[xcc == k].max()), 1) for k in np.unique(xcc)}
    out["xcc_waves"] = {int(k): int((xcc == k).sum()) for k in np.unique(xcc)}
    # the end of the launch: which waves set it
    site = r[:, 4]
    out["site_waves"] = {int(k): int((site == k).sum()) for k in np.unique(site)}
    out["site_dur_median_us"] = {int(k): round(float(np.median(du[site == k])), 2)
                                 for k in np.unique(site)}
    out["last_dispatch_us"] = float(st.max())
    uni = site != 2
    out["last_uniform_end_us"] = float(en[uni].max()) if uni.any() else None
    out["end_minus_last_uniform_end_us"] = (round(float(en.max() - en[uni].max()), 2)
                                            if uni.any() else None)
    gen = np.flatnonzero(site == 2)
    out["generic_chunks"] = [int(c) for c in gen]
    out["generic_start_us"] = [round(float(st[c]), 2) for c in gen]
    out["generic_dur_us"] = [round(float(du[c]), 2) for c in gen]
    wave = r[:, 5]  # the wave of the grid that took the chunk (listed chunks: the first waves)
    if wave.max() == 0:  # a launch without a list: wave w takes chunk w
        wave = np.arange(nw)
    out["grid_waves"] = int(wave.max()) + 1
    out["chunks_taken_out_of_order"] = int((wave != np.arange(nw)).sum())
    out["first_waves_chunks"] = [int(c) for c in np.argsort(wave)[:int(wave.max()) + 1 - nw]]
    last = np.argsort(en)[::-1][:32]
    out["last_ending"] = [{"chunk": int(c), "wave": int(wave[c]),
                           "pos": round(float(wave[c]) / (int(wave.max()) + 1), 4),
                           "site": int(site[c]),
                           "start_us": round(float(st[c]), 2), "dur_us": round(float(du[c]), 2),
                           "end_us": round(float(en[c]), 2)} for c in last]
    out["generic_among_last_16"] = int((site[last[:16]] == 2).sum())
    text = json.dumps(out)
    print(text, flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
