"""Drop-in for the reference's `wfpt` extension module (src/wfpt.pyx), on MI355X.

Same names, positional order, defaults and return conventions as the Cython
module that `hddm/__init__.py:16` imports as `hddm.wfpt`:

    pdf_array   src/wfpt.pyx:32-48    (defaults err=1e-4, n_st=n_sz=2, simps_err=1e-3, w_outlier=0)
    wiener_like src/wfpt.pyx:54-76    (defaults n_st=n_sz=10, simps_err=1e-8, w_outlier=0.1)
    full_pdf    src/pdf.pxi:104-146   (cpdef; defaults n_st=n_sz=2, simps_err=1e-3)
    wiener_like_multi  src/wfpt.pyx:244-274
    wiener_like_rlddm        src/wfpt.pyx:79-154   (Q-learning drift; RLDataset: resident data)
    wiener_like_rl           src/wfpt.pyx:157-241  (choice probability only)
    wiener_like_multi_rlddm  src/wfpt.pyx:277-320  (per-trial parameters, adjacent-change reset)
    gen_rts_from_cdf   src/wfpt.pyx:323-354 (density grid on the GPU, sampling in NumPy)

Every density is computed by the HIP kernels of libwfpt_amd.so; there is no
CPU path. Argument checking mirrors Cython's buffer protocol: `x` must be a
1-D float64 ndarray (TypeError otherwise; ValueError for dtype / ndim).

Additions for resident data (the reference re-reads host memory every call):
`Dataset(rt)` uploads RTs once; `Dataset.wiener_like(...)` has wiener_like's
signature minus `x`. `Dataset(rt, node_id=...)` + `wiener_like_nodes` scores
many PyMC nodes in one launch. `gen_rts_from_cdf_nodes` draws RTs for many
parameter rows in one call, grid, CDF and search on the device (posterior
predictive data sets: HDDM.post_pred_gen). `gen_rts_from_drift_nodes` /
`gen_rts_from_drift` are the reference's 'drift' sampling method
(hddm/generate.py:208-319: every RT a simulated diffusion path, with the
in-trial drift switch) on the device. `rt_stats_rows` reduces many rows of
signed RTs to the posterior predictive check's statistics (gen_ppc_stats,
hddm/utils.py:241-265) on the device, and `gen_rts_stats_nodes` does so for
the draws of either sampler without copying them out. `gen_rlddm_rows` simulates
RLDDM sequences in closed loop on the device (hddm/generate.py:430-516: every
trial's drift comes from the Q values the earlier simulated trials left), and
`gen_rlddm_stats_rows` reduces its draws likewise. `RegDataset(rt, design)` keeps a
design matrix resident and forms HDDMRegressor's trial-wise parameters
link(design . coefficients) on the device (hddm_regression.py:26-36);
`RegDataset.gen_rts_drift` / `gen_rts_drift_stats` simulate one diffusion path
per (sweep, trial) at those trial-wise parameters, formed on the device as the
walk picks the trial up (the regression node's random(), hddm_regression.py:39-56).

Shared pieces, each stated once: the samplers' argument rules (`_sampler_table`,
`_cdf_prep`, `_drift_prep` / `_drift_seed`, `_check_drawn`, `_check_finished`)
serve the plain samplers and `gen_rts_stats_nodes` alike; `_multi_args` builds
the per-trial arguments of the 7- and 8-parameter forms, with `_like_multi` and
`_like_multi_rlddm` behind every wiener_like_multi[_rlddm] spelling; the three
resident classes share `_Resident` (close / __del__ / __len__) and `_id_array`;
the module-level RL functions run a method over a transient `RLDataset`
(`_on_rl_dataset`).
"""
import ctypes

import numpy as np

from . import _lib

__all__ = ["pdf_array", "wiener_like", "full_pdf", "wiener_like_multi", "wiener_like_multi_terms",
           "gen_rts_from_cdf", "gen_rts_from_cdf_nodes", "gen_rts_from_drift_nodes",
           "gen_rts_from_drift", "rt_stats_rows", "rt_stats_names", "gen_rts_stats_nodes",
           "gen_rlddm_rows", "gen_rlddm_stats_rows",
           "Dataset", "prob_ub", "wiener_like_rlddm", "wiener_like_rl", "wiener_like_multi_rlddm",
           "RLDataset", "wiener_like_rlddm_nodes", "wiener_like_rlddm_nodes_multi",
           "wiener_like_rlddm_terms",
           "wiener_like_rl_terms", "wiener_like_multi_rlddm_terms", "RegDataset",
           "RLRegDataset"]


def _check_x(x, name="x"):
    """Cython `np.ndarray[double, ndim=1]` argument semantics."""
    if not isinstance(x, np.ndarray):
        raise TypeError(f"Argument '{name}' has incorrect type (expected numpy.ndarray, got "
                        f"{type(x).__name__})")
    if x.dtype != np.float64:
        raise ValueError(f"Buffer dtype mismatch, expected 'double' but got {x.dtype}")
    if x.ndim != 1:
        raise ValueError(f"Buffer has wrong number of dimensions (expected 1, got {x.ndim})")
    return np.ascontiguousarray(x)


def _i64ptr(a):
    return a.ctypes.data_as(_lib._PI64)


def _optr(a):
    """double* of an optional array (None: NULL)."""
    return _lib.dptr(a) if a is not None else None


def pdf_array(x, v, sv, a, z, sz, t, st, err=1e-4, logp=0, n_st=2, n_sz=2, use_adaptive=1,
              simps_err=1e-3, p_outlier=0, w_outlier=0):
    x = _check_x(x)
    out = np.empty(x.shape[0], dtype=np.float64)
    c = _lib.context()
    P = _lib.make_params(v, sv, a, z, sz, t, st, p_outlier)
    K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
    _lib.check(_lib.wfpt_pdf_array(c.handle, _lib.dptr(x), x.shape[0], ctypes.byref(P),
                                   ctypes.byref(K), 1 if logp else 0, _lib.dptr(out)))
    return out


def wiener_like(x, v, sv, a, z, sz, t, st, err, n_st=10, n_sz=10, use_adaptive=1,
                simps_err=1e-8, p_outlier=0, w_outlier=0.1):
    x = _check_x(x)
    c = _lib.context()
    P = _lib.make_params(v, sv, a, z, sz, t, st, p_outlier)
    K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
    out = ctypes.c_double()
    _lib.check(_lib.wfpt_wiener_like_host(c.handle, _lib.dptr(x), x.shape[0], ctypes.byref(P),
                                          ctypes.byref(K), ctypes.byref(out)))
    return out.value


def full_pdf(x, v, sv, a, z, sz, t, st, err, n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3):
    x = float(x)
    c = _lib.context()
    P = _lib.make_params(v, sv, a, z, sz, t, st, 0.0)
    K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, 0.0)
    out = ctypes.c_double()
    _lib.check(_lib.wfpt_full_pdf(c.handle, x, ctypes.byref(P), ctypes.byref(K),
                                  ctypes.byref(out)))
    return out.value


def prob_ub(v, a, z):
    """P(upper boundary), pdf.pxi:67-72 (host scalar helper, as in likelihoods.py:64-67)."""
    if v == 0:
        return z
    return (np.exp(-2 * a * z * v) - 1) / (np.exp(-2 * a * v) - 1)


_MULTI_NAMES = ("v", "sv", "a", "z", "sz", "t", "st")


def _multi_args(n, names, vals, multi):
    """Per-trial arrays (pointer table, kept alive) and scalars of a
    wiener_like_multi[_rlddm] call (wfpt.pyx:257-260, 296: names in `multi`
    are indexed per trial, the others are scalars)."""
    multi = set(multi)
    keep = []
    ptrs = (_lib._PD * len(names))()
    scal = np.zeros(len(names))
    for j, (nm, val) in enumerate(zip(names, vals)):
        if nm in multi:
            arr = np.ascontiguousarray(np.asarray(val, dtype=np.float64))
            if arr.shape != (n,):
                raise ValueError(f"parameter {nm} must have one value per trial")
            keep.append(arr)
            ptrs[j] = _lib.dptr(arr)
        else:
            ptrs[j] = _lib._PD()
            scal[j] = float(val)
    return ptrs, scal, keep


def _like_multi(ds, x, n, vals, err, multi, n_st, n_sz, use_adaptive, simps_err, p_outlier,
                w_outlier, trials):
    """wiener_like_multi over the resident Dataset `ds` or, with ds None, the
    host RTs `x`; trials: (sum, per-trial terms)."""
    ptrs, scal, keep = _multi_args(n, _MULTI_NAMES, vals, multi)
    c = (ds.ctx if ds is not None else _lib.context()).handle
    K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
    out = ctypes.c_double()
    terms = np.empty(n, dtype=np.float64) if trials else None
    args = (ptrs, _lib.dptr(scal), ctypes.byref(K), float(p_outlier), ctypes.byref(out))
    if ds is not None:
        rc = _lib.wfpt_wiener_like_multi_resident_ex(c, ds.handle, *args,
                                                     _lib.dptr(terms) if trials else None)
    elif trials:
        rc = _lib.wfpt_wiener_like_multi_ex(c, _lib.dptr(x), n, *args, _lib.dptr(terms))
    else:
        rc = _lib.wfpt_wiener_like_multi(c, _lib.dptr(x), n, *args)
    _lib.check(rc)
    del keep
    return (out.value, terms) if trials else out.value


def wiener_like_multi(x, v, sv, a, z, sz, t, st, err, multi=None, n_st=10, n_sz=10,
                      use_adaptive=1, simps_err=1e-3, p_outlier=0, w_outlier=0):
    x = _check_x(x)
    if multi is None:
        return full_pdf(x, v, sv, a, z, sz, t, st, err)  # wfpt.pyx:255-256 (TypeError for arrays)
    return _like_multi(None, x, x.shape[0], (v, sv, a, z, sz, t, st), err, multi, n_st, n_sz,
                       use_adaptive, simps_err, p_outlier, w_outlier, False)


def wiener_like_multi_terms(x, v, sv, a, z, sz, t, st, err, multi, n_st=10, n_sz=10,
                            use_adaptive=1, simps_err=1e-3, p_outlier=0, w_outlier=0):
    """wiener_like_multi (wfpt.pyx:244-274) returning (sum, per-trial terms):
    terms[i] is trial i's addend log p_i (wfpt.pyx:261-272)."""
    x = _check_x(x)
    return _like_multi(None, x, x.shape[0], (v, sv, a, z, sz, t, st), err, multi, n_st, n_sz,
                       use_adaptive, simps_err, p_outlier, w_outlier, True)


def gen_rts_from_cdf(v, sv, a, z, sz, t, st, samples=1000, cdf_lb=-6, cdf_ub=6, dt=1e-2):
    """wfpt.pyx:323-354: inverse-CDF sampling from the density on a dt grid.

    The grid density (full_pdf with t = st = 0, err = 1e-4) runs on the GPU;
    the running sum, normalisation, searchsorted and the non-decision-time
    delays follow the reference step for step and draw from NumPy's global
    RNG in the same order.
    """
    x = np.arange(cdf_lb, cdf_ub, dt)
    pdf = pdf_array(x[1:].copy(), v, sv, a, z, sz, 0, 0, 1e-4)
    l_cdf = np.empty(x.shape[0], dtype=np.float64)
    l_cdf[0] = 0
    l_cdf[1:] = np.cumsum(pdf)
    l_cdf /= l_cdf[x.shape[0] - 1]
    f = np.random.rand(samples)
    if st != 0:
        delay = np.random.rand(samples) * st + (t - st / 2.)
    idx = np.searchsorted(l_cdf, f)
    rt = x[idx]
    if st == 0:
        return rt + np.sign(rt) * t
    return rt + np.sign(rt) * delay


# The samplers' argument rules, shared by gen_rts_from_cdf_nodes /
# gen_rts_from_drift_nodes and the fused gen_rts_stats_nodes: each check, RNG
# rule and error mapping is stated here and nowhere else.

def _sampler_table(params, samples):
    """The samplers' (R, 8) table, per-row counts and offsets."""
    pm = np.asarray(params, dtype=np.float64)
    if pm.ndim != 2 or pm.shape[1] not in (7, 8) or pm.shape[0] < 1:
        raise ValueError("params must have shape (R, 7) or (R, 8), R >= 1")
    R = pm.shape[0]
    table = np.zeros((R, 8))
    table[:, :pm.shape[1]] = pm
    cnt = np.asarray(samples)
    if cnt.ndim == 0:
        cnt = np.full(R, int(cnt))
    if cnt.shape != (R,) or not np.issubdtype(cnt.dtype, np.integer):
        raise ValueError(f"samples must be an int or {R} ints")
    cnt = np.ascontiguousarray(cnt, dtype=np.int64)
    if np.any(cnt < 0):
        raise ValueError("samples must be non-negative")
    offsets = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(cnt, out=offsets[1:])
    return table, cnt, offsets


def _cdf_prep(table, cnt, offsets, cdf_lb, cdf_ub, dt, u, u_delay, seed, max_workspace):
    """The CDF sampler's checked arguments: (grid, u, u_delay, seed, workspace
    bytes). Without `u` and `seed` the uniforms are drawn here, from NumPy's
    global RNG in the reference's order."""
    R, total = table.shape[0], int(offsets[-1])
    has_st = table[:, 6] != 0
    if u is None and u_delay is not None:
        raise ValueError("u_delay needs u")
    if u is not None:
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.shape != (total,):
            raise ValueError(f"u must hold sum(samples) = {total} uniforms")
        if has_st.any() and u_delay is None:
            raise ValueError("u_delay is needed: a row has st != 0")
        if u_delay is not None:
            u_delay = np.ascontiguousarray(u_delay, dtype=np.float64)
            if u_delay.shape != (total,):
                raise ValueError(f"u_delay must hold sum(samples) = {total} uniforms")
        for nm, arr in (("u", u), ("u_delay", u_delay)):
            if arr is not None and arr.size and not (arr.min() >= 0 and arr.max() < 1):
                raise ValueError(f"{nm} must lie in [0, 1)")
    elif seed is None:
        # the reference's order of draws from the global RNG (wfpt.pyx:340-345)
        u = np.empty(total)
        u_delay = np.zeros(total) if has_st.any() else None
        for r in range(R):
            lo, hi = offsets[r], offsets[r + 1]
            u[lo:hi] = np.random.rand(int(cnt[r]))
            if has_st[r]:
                u_delay[lo:hi] = np.random.rand(int(cnt[r]))
    x = np.arange(cdf_lb, cdf_ub, dt)
    if x.shape[0] < 2:
        raise ValueError("the grid np.arange(cdf_lb, cdf_ub, dt) needs at least two points")
    ws = 0 if max_workspace is None else int(max_workspace)
    if ws < 0:
        raise ValueError("max_workspace must be positive")
    return x, u, u_delay, 0 if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF, ws


def _drift_prep(R, dt, intra_sv, switch, max_t, unfinished):
    """The drift sampler's checked arguments: (dt, intra_sv, max_steps, switch
    table or None). The seed is _drift_seed's: the plain sampler checks its own
    arguments between the two, before anything is taken from the global RNG."""
    dt, intra_sv = float(dt), float(intra_sv)
    if not (dt > 0 and np.isfinite(dt)):
        raise ValueError("dt must be positive")
    if not (intra_sv > 0 and np.isfinite(intra_sv)):
        raise ValueError("intra_sv must be positive")
    if not max_t > 0:
        raise ValueError("max_t must be positive")
    max_steps = int(np.ceil(float(max_t) / dt))
    if not 1 <= max_steps <= 2 ** 31:
        raise ValueError("ceil(max_t / dt) must lie in [1, 2^31]")
    if unfinished not in ("raise", "nan"):
        raise ValueError("unfinished must be 'raise' or 'nan'")
    sw = None
    if switch is not None:
        sw = np.ascontiguousarray(switch, dtype=np.float64)
        if sw.shape != (R, 3):
            raise ValueError(f"switch must have shape ({R}, 3): v_switch, V_switch, t_switch")
        if not np.all(np.round(sw[:, 2] / dt) >= 1):  # generate.py:237-239
            raise ValueError("t_switch / dt must round to at least one step")
    return dt, intra_sv, max_steps, sw


def _drift_seed(seed):
    """The drift sampler's 64-bit seed; None takes two 32-bit words from
    NumPy's global RNG."""
    if seed is None:
        lo, hi = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint64)
        seed = int(lo) | (int(hi) << 32)
    return int(seed) & 0xFFFFFFFFFFFFFFFF


_NO_DRAW = {"cdf": b"has no CDF", "drift": b"cannot be simulated"}


def _check_drawn(rc, method):
    """_lib.check for a sampler's status: a parameter row it cannot draw from
    is a RuntimeError that names the row, not check's NotImplementedError."""
    if rc == 4 and _NO_DRAW[method] in _lib.wfpt_last_error():
        raise RuntimeError("wfpt_amd: " + _lib.wfpt_last_error().decode(errors="replace"))
    _lib.check(rc)


def _check_finished(n_unfinished, total, max_steps, max_t, unfinished):
    if n_unfinished and unfinished == "raise":
        raise RuntimeError(f"wfpt_amd: {n_unfinished} of {total} draws had not crossed a boundary "
                           f"after {max_steps} steps (max_t = {max_t})")


def gen_rts_from_cdf_nodes(params, samples, cdf_lb=-6, cdf_ub=6, dt=1e-2, u=None, u_delay=None,
                           seed=None, max_workspace=None, return_debug=False):
    """gen_rts_from_cdf (wfpt.pyx:323-354) for R parameter rows in one call:
    grid densities, running sums, normalisation, search and delays all run on
    the GPU (wfpt_gen_rts_nodes); only the draws come back.

    params: (R, 7) or (R, 8) rows of v, sv, a, z, sz, t, st[, p_outlier]
    (node_table's column order; p_outlier is ignored). samples: draws per row,
    an int or R ints. Returns (rts, offsets): row r's draws are
    rts[offsets[r]:offsets[r + 1]].

    Uniforms, in this order of precedence: `u` (and `u_delay` when a row has
    st != 0), sum(samples) values in [0, 1) each, row after row; `seed`, the
    device's Philox4x32-10 streams (the draws depend on the seed, the row index
    and the draw index only); else NumPy's global RNG in the reference's order,
    rand(n_r) and, when the row's st != 0, rand(n_r), row after row: under one
    np.random.seed the call reproduces a loop of gen_rts_from_cdf calls.

    max_workspace: device bytes for the rows' grids (default 1 GiB); more rows
    than fit are processed in tiles, with the same result. return_debug: also
    a dict of the grid `x`, the densities `pdf` and normalised CDF `cdf`
    (R, len(x) - 1), each draw's grid index `idx` and the uniforms `u`,
    `u_delay` used.
    """
    table, cnt, offsets = _sampler_table(params, samples)
    x, u, u_delay, seed, ws = _cdf_prep(table, cnt, offsets, cdf_lb, cdf_ub, dt, u, u_delay, seed,
                                        max_workspace)
    R, G, total = table.shape[0], x.shape[0], int(offsets[-1])
    out = np.empty(total, dtype=np.float64)
    head = (_lib.context().handle, _lib.dptr(x), G, table.ctypes.data_as(_lib._PP), R,
            _i64ptr(cnt), _optr(u), _optr(u_delay), seed, ws, _lib.dptr(out))
    if return_debug:
        dbg = {"x": x, "pdf": np.empty((R, G - 1)), "cdf": np.empty((R, G - 1)),
               "idx": np.empty(total, dtype=np.int64), "u": np.empty(total),
               "u_delay": np.empty(total)}
        rc = _lib.wfpt_gen_rts_nodes_ex(*head, _lib.dptr(dbg["pdf"]), _lib.dptr(dbg["cdf"]),
                                        _i64ptr(dbg["idx"]), _lib.dptr(dbg["u"]),
                                        _lib.dptr(dbg["u_delay"]))
    else:
        rc = _lib.wfpt_gen_rts_nodes(*head)
    _check_drawn(rc, "cdf")
    return (out, offsets, dbg) if return_debug else (out, offsets)


def gen_rts_from_drift_nodes(params, samples, dt=1e-4, intra_sv=1., seed=None, switch=None,
                             max_t=20., unfinished='raise', return_debug=False, row0=0,
                             wave_draws=None):
    """_gen_rts_from_simulated_drift (hddm/generate.py:208-319), the 'drift'
    sampling method, for R parameter rows in one call on the GPU
    (wfpt_gen_rts_drift_nodes): every draw is one +-sqrt(dt) * intra_sv random
    walk between the boundaries with the crossing time interpolated, in the
    reference's arithmetic.

    params: (R, 7) or (R, 8) rows of v, sv, a, z, sz, t, st[, p_outlier]
    (p_outlier is ignored). samples: draws per row, an int or R ints. switch:
    None, or (R, 3) rows of v_switch, V_switch, t_switch: from step
    round(t_switch / dt) on the walk uses the drift v_switch (+ V_switch times a
    normal draw when V_switch != 0). Returns (rts, offsets): row r's draws are
    rts[offsets[r]:offsets[r + 1]].

    seed: the device's Philox4x32-10 streams; a draw depends on the seed, its
    row's index and its index in the row only. None takes a seed from NumPy's
    global RNG, so np.random.seed makes the call reproducible. A walk is cut
    after ceil(max_t / dt) steps: unfinished='raise' raises RuntimeError with
    the number of such draws, 'nan' returns them as NaN.

    return_debug: also a dict of each draw's start point `y0`, `delay`,
    `drift`, `drift_switch` and steps taken `n_steps`. row0 is added to the
    row index of the random streams (a slice of a larger table draws what it
    draws there). wave_draws: draws handed to one wave (a multiple of 64; a
    measurement knob that changes no value); with return_debug the dict then
    also holds `wave_steps`, the steps each wave's loop ran.
    """
    table, cnt, offsets = _sampler_table(params, samples)
    R, total = table.shape[0], int(offsets[-1])
    dt, intra_sv, max_steps, sw = _drift_prep(R, dt, intra_sv, switch, max_t, unfinished)
    row0 = int(row0)
    if not 0 <= row0 < 2 ** 31:
        raise ValueError("row0 must lie in [0, 2^31)")
    wd = 0 if wave_draws is None else int(wave_draws)
    if wd < 0 or wd % 64:
        raise ValueError("wave_draws must be a positive multiple of 64")
    seed = _drift_seed(seed)
    out = np.empty(total, dtype=np.float64)
    nun = ctypes.c_int64()
    head = (_lib.context().handle, table.ctypes.data_as(_lib._PP), R, _optr(sw), _i64ptr(cnt), dt,
            intra_sv, max_steps, seed)
    if return_debug or row0 or wd:
        dbg = {k: np.empty(total) for k in ("y0", "delay", "drift", "drift_switch")}
        dbg["n_steps"] = np.empty(total, dtype=np.int64)
        if wd:
            dbg["wave_steps"] = np.empty(-(-total // wd), dtype=np.int64)
        rc = _lib.wfpt_gen_rts_drift_nodes_ex(
            *head, row0, wd, _lib.dptr(out), ctypes.byref(nun), _lib.dptr(dbg["y0"]),
            _lib.dptr(dbg["delay"]), _lib.dptr(dbg["drift"]), _lib.dptr(dbg["drift_switch"]),
            _i64ptr(dbg["n_steps"]), _i64ptr(dbg["wave_steps"]) if wd else None)
    else:
        rc = _lib.wfpt_gen_rts_drift_nodes(*head, _lib.dptr(out), ctypes.byref(nun))
    _check_drawn(rc, "drift")
    _check_finished(nun.value, total, max_steps, max_t, unfinished)
    return (out, offsets, dbg) if return_debug else (out, offsets)


def gen_rts_from_drift(v, sv, a, z, sz, t, st, samples=1000, dt=1e-4, intra_sv=1., seed=None,
                       **switch):
    """generate.py:208-319 for one parameter set: `samples` signed RTs of the
    simulated diffusion path. switch: v_switch, t_switch and optionally
    V_switch, the reference's in-trial change of the drift rate."""
    unknown = set(switch) - {"v_switch", "V_switch", "t_switch"}
    if unknown:
        raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
    sw = None
    if "v_switch" in switch:
        if "t_switch" not in switch:
            raise ValueError("v_switch needs t_switch")
        sw = [[switch["v_switch"], switch.get("V_switch", 0.0), switch["t_switch"]]]
    return gen_rts_from_drift_nodes([[v, sv, a, z, sz, t, st]], int(samples), dt, intra_sv, seed,
                                    switch=sw)[0]


PPC_QUANTILES = (10, 30, 50, 70, 90)  # gen_ppc_stats' default (hddm/utils.py:241)


def _check_quantiles(quantiles):
    q = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
    if q.size > 16:
        raise ValueError("at most 16 quantiles")
    if not np.all((q >= 0) & (q <= 100)):  # NaN fails both comparisons
        raise ValueError("quantiles must lie in [0, 100]")
    return q


def rt_stats_names(quantiles=PPC_QUANTILES):
    """The columns of rt_stats_rows: n, n_ub, n_lb, then gen_ppc_stats' own
    names in its order (hddm/utils.py:250-265): accuracy, mean_ub, std_ub,
    '10q_ub', ..., mean_lb, std_lb, '10q_lb', ..."""
    keys = [str(q) + "q" for q in quantiles]
    return (["n", "n_ub", "n_lb", "accuracy", "mean_ub", "std_ub"] + [k + "_ub" for k in keys]
            + ["mean_lb", "std_lb"] + [k + "_lb" for k in keys])


def rt_stats_rows(rts, offsets, quantiles=PPC_QUANTILES, tier=0):
    """gen_ppc_stats (hddm/utils.py:241-265) for R rows of signed RTs in one
    call on the GPU (wfpt_rt_stats_rows): row r is rts[offsets[r]:offsets[r + 1]].

    Returns an (R, 8 + 2 len(quantiles)) array with rt_stats_names' columns.
    The upper boundary's draws are those > 0, the lower boundary's those < 0
    (mean_lb is the mean of the signed values, the lower quantiles are taken
    over |x|); a draw that is 0 or NaN counts in n only. std is np.std
    (ddof=0); each quantile equals scipy.stats.scoreatpercentile bit for bit;
    an empty boundary gives NaN. tier: 0 picks the kernel by row length, 1 / 2 /
    3 force the wave / block / global one (ValueError when a row does not fit).
    """
    q = _check_quantiles(quantiles)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    if off.ndim != 1 or off.size < 2:
        raise ValueError("offsets must hold R + 1 >= 2 entries")
    if off[0] != 0 or np.any(np.diff(off) < 0):
        raise ValueError("offsets must rise from 0")
    x = np.ascontiguousarray(rts, dtype=np.float64)
    if x.ndim != 1 or x.size != off[-1]:
        raise ValueError(f"rts must hold offsets[-1] = {int(off[-1])} values")
    if tier not in (0, 1, 2, 3):
        raise ValueError("tier must be 0, 1, 2 or 3")
    R = off.size - 1
    out = np.empty((R, 8 + 2 * q.size))
    c = _lib.context()
    _lib.check(_lib.wfpt_rt_stats_rows_ex(c.handle, _lib.dptr(x), _i64ptr(off), R, _lib.dptr(q),
                                          q.size, int(tier), _lib.dptr(out)))
    return out


def _cdf_stats(table, cnt, offsets, q, out, stats, seed=None, cdf_lb=-6, cdf_ub=6, dt=1e-2, u=None,
               u_delay=None, max_workspace=None):
    x, u, u_delay, seed, ws = _cdf_prep(table, cnt, offsets, cdf_lb, cdf_ub, dt, u, u_delay, seed,
                                        max_workspace)
    rc = _lib.wfpt_gen_rts_nodes_stats(
        _lib.context().handle, _lib.dptr(x), x.shape[0], table.ctypes.data_as(_lib._PP),
        table.shape[0], _i64ptr(cnt), _optr(u), _optr(u_delay), seed, ws, _optr(out), _lib.dptr(q),
        q.size, _lib.dptr(stats))
    _check_drawn(rc, "cdf")


def _drift_stats(table, cnt, offsets, q, out, stats, seed=None, dt=1e-4, intra_sv=1., switch=None,
                 max_t=20., unfinished="raise"):
    R = table.shape[0]
    dt, intra_sv, max_steps, sw = _drift_prep(R, dt, intra_sv, switch, max_t, unfinished)
    seed = _drift_seed(seed)
    nun = ctypes.c_int64()
    rc = _lib.wfpt_gen_rts_drift_nodes_stats(
        _lib.context().handle, table.ctypes.data_as(_lib._PP), R, _optr(sw), _i64ptr(cnt), dt,
        intra_sv, max_steps, seed, _optr(out), ctypes.byref(nun), _lib.dptr(q), q.size,
        _lib.dptr(stats))
    _check_drawn(rc, "drift")
    _check_finished(nun.value, int(offsets[-1]), max_steps, max_t, unfinished)


def gen_rts_stats_nodes(params, samples, method="cdf", quantiles=PPC_QUANTILES, seed=None,
                        return_draws=False, **sampler_kw):
    """The draws of gen_rts_from_cdf_nodes (method='cdf') or
    gen_rts_from_drift_nodes (method='drift') for R parameter rows, reduced to
    rt_stats_rows' statistics while they are still in device memory
    (wfpt_gen_rts_nodes_stats / wfpt_gen_rts_drift_nodes_stats): with
    return_draws=False no draw is copied to the host.

    params, samples, seed and sampler_kw (cdf: cdf_lb, cdf_ub, dt, u, u_delay,
    max_workspace; drift: dt, intra_sv, switch, max_t, unfinished) are the
    sampler's own, with its seed, uniform and RNG rules: the draws are the ones
    that sampler returns for the same arguments. Returns (stats, offsets), and
    the draws as a third element with return_draws=True; stats is (R, 8 + 2
    len(quantiles)) in rt_stats_names' order."""
    if method not in ("cdf", "drift"):
        raise ValueError("method must be 'cdf' or 'drift'")
    q = _check_quantiles(quantiles)
    table, cnt, offsets = _sampler_table(params, samples)
    stats = np.empty((table.shape[0], 8 + 2 * q.size))
    out = np.empty(int(offsets[-1])) if return_draws else None
    run = _cdf_stats if method == "cdf" else _drift_stats
    run(table, cnt, offsets, q, out, stats, seed=seed, **sampler_kw)
    return (stats, offsets, out) if return_draws else (stats, offsets)


# The closed-loop RLDDM simulator (wfpt_gen_rlddm_rows).

_RL_DEBUG = ("feedback", "q_up", "q_low", "sim_drift", "drift", "y0", "delay")


def _rl_source(R, cnt, offsets, rewards, reward_arrays, observed):
    """The checked reward source of a closed-loop call: (_lib.RlSource, the
    arrays it points into). Exactly one of the three is given."""
    if sum(x is not None for x in (rewards, reward_arrays, observed)) != 1:
        raise ValueError("exactly one of rewards, reward_arrays and observed must be given")
    src, keep = _lib.RlSource(), []

    def addr(a):
        keep.append(a)
        return a.ctypes.data

    if rewards is not None:
        p = np.asarray(rewards, dtype=np.float64)
        if p.shape == (2,):
            p = np.tile(p, (R, 1))
        if p.shape != (R, 2):
            raise ValueError(f"rewards must have shape (2,) or ({R}, 2): p_upper, p_lower")
        if not np.all((p >= 0) & (p <= 1)):  # NaN fails both comparisons
            raise ValueError("reward probabilities must lie in [0, 1]")
        src.p = addr(np.ascontiguousarray(p))
        return src, keep
    name = "reward_arrays" if reward_arrays is not None else "observed"
    parts = tuple(reward_arrays if reward_arrays is not None else observed)
    if len(parts) not in (2, 3):
        raise ValueError(f"{name} must be (first, second) or (first, second, start)")
    first = np.ascontiguousarray(parts[0], dtype=np.float64 if observed is None else np.int64)
    second = np.ascontiguousarray(parts[1], dtype=np.float64)
    if first.ndim != 1 or first.shape != second.shape:
        raise ValueError(f"the two arrays of {name} must be 1-D and of one length")
    if len(parts) == 3:
        start = np.ascontiguousarray(parts[2], dtype=np.int64)
        if start.shape != (R,):
            raise ValueError(f"the start offsets of {name} must hold {R} entries")
    else:
        start = offsets[:-1]
    if np.any(start < 0) or np.any(start + cnt > first.size):
        raise ValueError(f"a row reads outside the {first.size} elements of {name}")
    if len(parts) == 3:
        src.start = addr(start)
    src.n = first.size
    if observed is None:
        src.rew_up, src.rew_low = addr(first), addr(second)
    else:
        src.obs_response, src.obs_feedback = addr(first), addr(second)
    return src, keep


def _rlddm_prep(params, rl_rows, n_trials, rewards, reward_arrays, observed, dt, intra_sv, max_t,
                unfinished, row0):
    """The closed-loop simulator's checked arguments, before the seed is taken
    and before any context is loaded."""
    table, cnt, offsets = _sampler_table(params, n_trials)
    R = table.shape[0]
    rl = np.ascontiguousarray(rl_rows, dtype=np.float64)
    if rl.shape != (R, 3):
        raise ValueError(f"rl_rows must have shape ({R}, 3): q, alpha, pos_alpha")
    if np.isnan(rl).any():
        raise ValueError("rl_rows must not hold NaN")
    dt, intra_sv, max_steps, _ = _drift_prep(R, dt, intra_sv, None, max_t, unfinished)
    row0 = int(row0)
    if not 0 <= row0 <= 2 ** 31 - R:
        raise ValueError("row0 + R must lie in [1, 2^31]")
    src, keep = _rl_source(R, cnt, offsets, rewards, reward_arrays, observed)
    return table, rl, cnt, offsets, dt, intra_sv, max_steps, row0, src, keep


def gen_rlddm_rows(params, rl_rows, n_trials, rewards=None, reward_arrays=None, observed=None,
                   dt=1e-4, intra_sv=1., seed=None, max_t=20., unfinished='raise',
                   return_debug=False, row0=0, wave_rows=None):
    """gen_rand_rlddm_data (hddm/generate.py:430-516) for R sequences in ONE
    launch on the GPU (wfpt_gen_rlddm_rows): a lane owns a sequence and closes
    the loop itself -- simulate the trial as a diffusion path (the arithmetic
    and random streams of gen_rts_from_drift_nodes with the draw index set to
    the trial index), take the chosen option's reward, move its Q value
    exactly as the likelihood does, form the next drift (q_up - q_low) * v.

    params: (R, 7) or (R, 8) rows of v (the drift scaling), sv, a, z, sz, t,
    st[, p_outlier]. rl_rows: (R, 3) rows of q, alpha, pos_alpha (alpha on the
    unbounded scale, pos_alpha == 100.0: use alpha). n_trials: trials per row,
    an int or R ints. Exactly one reward source:
      rewards        (2,) or (R, 2) probabilities p_upper, p_lower: binary
                     rewards drawn on the device;
      reward_arrays  (rew_up, rew_low[, start]): the two options' rewards per
                     trial; trial k of row r reads element start[r] + k
                     (default: the row's own offset), so replicate rows can
                     share one copy;
      observed       (response, feedback[, start]): the reference's
                     one-step-ahead simulator (generate.py:608-661): Q follows
                     the observed pair, the simulated RT is only recorded.
    Returns (rts, offsets): row r's trials are rts[offsets[r]:offsets[r + 1]].

    seed, max_t and unfinished are gen_rts_from_drift_nodes' (a cut walk makes
    its trial and every later trial of the row NaN). return_debug: also a dict
    of the per-trial `feedback`, `q_up`, `q_low` (before the update),
    `sim_drift`, the walk's `drift`, `y0`, `delay` and `n_steps`. row0 is added
    to the row index of the random streams; wave_rows (a multiple of 64) is a
    measurement knob that changes no value and adds `wave_steps` to the dict.
    """
    table, rl, cnt, offsets, dt, intra_sv, max_steps, row0, src, keep = _rlddm_prep(
        params, rl_rows, n_trials, rewards, reward_arrays, observed, dt, intra_sv, max_t,
        unfinished, row0)
    R, total = table.shape[0], int(offsets[-1])
    wd = 0 if wave_rows is None else int(wave_rows)
    if wd < 0 or wd % 64:
        raise ValueError("wave_rows must be a positive multiple of 64")
    seed = _drift_seed(seed)
    out = np.empty(total, dtype=np.float64)
    nun = ctypes.c_int64()
    head = (_lib.context().handle, table.ctypes.data_as(_lib._PP), _lib.dptr(rl), R, _i64ptr(cnt),
            ctypes.byref(src), dt, intra_sv, max_steps, seed)
    if return_debug or row0 or wd:
        dbg = {k: np.empty(total) for k in _RL_DEBUG}
        dbg["n_steps"] = np.empty(total, dtype=np.int64)
        if wd:
            dbg["wave_steps"] = np.empty(-(-R // wd), dtype=np.int64)
        rc = _lib.wfpt_gen_rlddm_rows_ex(
            *head, row0, wd, _lib.dptr(out), ctypes.byref(nun),
            *[_lib.dptr(dbg[k]) for k in _RL_DEBUG], _i64ptr(dbg["n_steps"]),
            _i64ptr(dbg["wave_steps"]) if wd else None)
    else:
        rc = _lib.wfpt_gen_rlddm_rows(*head, _lib.dptr(out), ctypes.byref(nun))
    _check_drawn(rc, "drift")
    _check_finished(nun.value, total, max_steps, max_t, unfinished)
    return (out, offsets, dbg) if return_debug else (out, offsets)


def gen_rlddm_stats_rows(params, rl_rows, n_trials, groups, rewards=None, reward_arrays=None,
                         observed=None, quantiles=PPC_QUANTILES, dt=1e-4, intra_sv=1., seed=None,
                         max_t=20., unfinished='raise', return_draws=False):
    """gen_rlddm_rows' draws (same arguments, same seed: the same draws)
    reduced to rt_stats_rows' statistics while they are still in device memory
    (wfpt_gen_rlddm_rows_stats). groups: G + 1 rising offsets from 0 to R over
    the rows; statistics row g covers the trials of rows groups[g] ..
    groups[g + 1], a node made of its condition sequences. Returns (stats,
    trial offsets of the groups), and the draws as a third element with
    return_draws=True; stats is (G, 8 + 2 len(quantiles)) in rt_stats_names'
    order."""
    q = _check_quantiles(quantiles)
    table, rl, cnt, offsets, dt, intra_sv, max_steps, _, src, keep = _rlddm_prep(
        params, rl_rows, n_trials, rewards, reward_arrays, observed, dt, intra_sv, max_t,
        unfinished, 0)
    R, total = table.shape[0], int(offsets[-1])
    goff = np.ascontiguousarray(groups, dtype=np.int64)
    if goff.ndim != 1 or goff.size < 2 or goff[0] != 0 or goff[-1] != R \
            or np.any(np.diff(goff) < 0):
        raise ValueError(f"groups must hold G + 1 >= 2 offsets rising from 0 to {R}")
    seed = _drift_seed(seed)
    G = goff.size - 1
    stats = np.empty((G, 8 + 2 * q.size))
    out = np.empty(total) if return_draws else None
    nun = ctypes.c_int64()
    rc = _lib.wfpt_gen_rlddm_rows_stats(
        _lib.context().handle, table.ctypes.data_as(_lib._PP), _lib.dptr(rl), R, _i64ptr(cnt),
        ctypes.byref(src), dt, intra_sv, max_steps, seed, _optr(out), ctypes.byref(nun),
        _i64ptr(goff), G, _lib.dptr(q), q.size, _lib.dptr(stats))
    _check_drawn(rc, "drift")
    _check_finished(nun.value, total, max_steps, max_t, unfinished)
    return (stats, offsets[goff], out) if return_draws else (stats, offsets[goff])


class _Resident:
    """Data resident in HBM behind `handle`: n trials, freed by the class's
    `_destroy` entry point."""

    def close(self):
        if getattr(self, "handle", None):
            self._destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.n


def _id_array(ids, count):
    """The optional per-trial ids (node_id, group_id) of a resident data set:
    (int32 array, `count` or one more than the largest id, int32 pointer)."""
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).ravel())
    count = int(count if count is not None else (ids.max() + 1 if ids.size else 0))
    return ids, count, ids.ctypes.data_as(_lib._PI32)


def _pointwise_result(sums, stats, trial, ninf_total):
    """The dict every pointwise_* method returns."""
    return {"sums": sums, "lppd": stats[0], "p_waic": stats[1], "mean": stats[2],
            "n_inf": stats[3].astype(np.int64), "trial": trial, "n_inf_total": int(ninf_total)}


class Dataset(_Resident):
    """RTs resident in HBM for repeated likelihood calls (MCMC: data fixed,
    parameters change per proposal). Optional `node_id` groups trials into
    `n_nodes` likelihood nodes scored together by `wiener_like_nodes`."""
    _destroy = staticmethod(_lib.wfpt_dataset_destroy)

    def __init__(self, rt, node_id=None, n_nodes=None, device=None, ctx=None, input_order=False):
        rt = np.ascontiguousarray(np.asarray(rt, dtype=np.float64).ravel())
        self.ctx = ctx if ctx is not None else _lib.context(device)
        self.n = rt.shape[0]
        self.input_order = bool(input_order)
        flags = _lib.WFPT_DS_INPUT_ORDER if input_order else 0
        node, self.n_nodes, nptr = None, 0, None
        if node_id is not None:
            node, self.n_nodes, nptr = _id_array(node_id, n_nodes)
            if node.shape != rt.shape:
                raise ValueError("node_id must have one entry per trial")
        h = _lib._VP()
        _lib.check(_lib.wfpt_dataset_create_ex(self.ctx.handle, _lib.dptr(rt), self.n, nptr,
                                               self.n_nodes, flags, ctypes.byref(h)))
        self.handle = h

    def _knobs(self, err, n_st, n_sz, use_adaptive, simps_err, w_outlier):
        """The knobs struct, rebuilt only when the knobs change (they are fixed
        across an MCMC run; per-call Python work sits in front of the kernel)."""
        key = (err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        kc = getattr(self, "_kc", None)
        if kc is None or kc[0] != key:
            K = _lib.make_knobs(*key)
            kc = self._kc = (key, K, ctypes.addressof(K))
        return kc[1]

    def _knobs_addr(self, err, n_st, n_sz, use_adaptive, simps_err, w_outlier):
        """(knobs struct, its address). The caller keeps the struct in a local
        until the raw call returns: another thread may replace self._kc (other
        knobs) meanwhile, and the address must not outlive its struct."""
        self._knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        kc = self._kc
        return kc[1], kc[2]

    def wiener_like(self, v, sv, a, z, sz, t, st, err, n_st=10, n_sz=10, use_adaptive=1,
                    simps_err=1e-8, p_outlier=0, w_outlier=0.1):
        P = _lib.make_params(v, sv, a, z, sz, t, st, p_outlier)
        K, kaddr = self._knobs_addr(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = ctypes.c_double()
        c, h = self.ctx.handle, self.handle
        if not c or not h:  # closed: the C ABI's own argument error
            _lib.check(_lib.wfpt_wiener_like(c, h, ctypes.byref(P), ctypes.byref(K),
                                             ctypes.byref(out)))
        rc = _lib.raw_wiener_like(c.value, h.value, ctypes.addressof(P), kaddr,
                                  ctypes.addressof(out))
        if rc:
            _lib.check(rc)
        return out.value

    def wiener_like_trials(self, v, sv, a, z, sz, t, st, err, n_st=10, n_sz=10, use_adaptive=1,
                           simps_err=1e-8, p_outlier=0, w_outlier=0.1):
        """wiener_like plus each trial's addend (wfpt.pyx:66-74), in the order the
        trials were given: (total, terms). Same call sequence and kernels as
        wiener_like (with one more store per trial): the per-trial check of the
        summing path."""
        P = _lib.make_params(v, sv, a, z, sz, t, st, p_outlier)
        K = self._knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = ctypes.c_double()
        terms = np.empty(self.n, dtype=np.float64)
        _lib.check(_lib.wfpt_wiener_like_trials(self.ctx.handle, self.handle, ctypes.byref(P),
                                                ctypes.byref(K), ctypes.byref(out),
                                                _lib.dptr(terms)))
        return out.value, terms

    def order(self):
        """order()[i] = the caller's index of stored trial i (chunk c holds
        stored trials 64c .. 64c + 63)."""
        perm = np.empty(self.n, dtype=np.int64)
        _lib.check(_lib.wfpt_dataset_order(self.handle, _i64ptr(perm)))
        return perm

    def local_triple(self, v, sv, a, z, sz, t, st, err, n_st=10, n_sz=10, use_adaptive=1,
                     simps_err=1e-8, p_outlier=0, w_outlier=0.1):
        """This shard's {sum log p, #zero trials, encoded errors}: what
        wiener_like_allreduce contributes to its all-reduce."""
        P = _lib.make_params(v, sv, a, z, sz, t, st, p_outlier)
        K = self._knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        r = (ctypes.c_double * 3)()
        _lib.check(_lib.wfpt_wiener_like_local(self.ctx.handle, self.handle, ctypes.byref(P),
                                               ctypes.byref(K), r))
        return [r[0], r[1], r[2]]

    def wiener_like_allreduce(self, v, sv, a, z, sz, t, st, err, n_st=10, n_sz=10,
                              use_adaptive=1, simps_err=1e-8, p_outlier=0, w_outlier=0.1):
        """Global sum over every rank's shard (requires hddm_amd.dist.init_comm; torch-free)."""
        P = _lib.make_params(v, sv, a, z, sz, t, st, p_outlier)
        K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = ctypes.c_double()
        _lib.check(_lib.wfpt_wiener_like_allreduce(self.ctx.handle, self.handle,
                                                   ctypes.byref(P), ctypes.byref(K),
                                                   ctypes.byref(out)))
        return out.value

    def wiener_like_multi(self, v, sv, a, z, sz, t, st, err, multi, n_st=10, n_sz=10,
                          use_adaptive=1, simps_err=1e-3, p_outlier=0, w_outlier=0,
                          trials=False):
        """wiener_like_multi (wfpt.pyx:244-274) over this resident dataset
        (created with input_order=True): only the per-trial parameter arrays
        go to the device per call. trials=True: (sum, per-trial terms)."""
        return _like_multi(self, None, self.n, (v, sv, a, z, sz, t, st), err, multi, n_st, n_sz,
                           use_adaptive, simps_err, p_outlier, w_outlier, trials)

    def _node_table(self, params):
        """The (n_nodes, 8) parameter table as a wfpt_params pointer, zero-copy
        (wfpt_params is 8 doubles, the row layout of a C-contiguous float64
        array); returns (pointer, the array that owns the memory)."""
        if self.n_nodes == 0:
            raise ValueError("dataset was created without node ids")
        pm = np.ascontiguousarray(params, dtype=np.float64)
        if pm.shape != (self.n_nodes, 8):
            raise ValueError(f"params must have shape ({self.n_nodes}, 8)")
        return pm.ctypes.data_as(_lib._PP), pm

    def wiener_like_nodes_local(self, params, err=1e-4, n_st=2, n_sz=2, use_adaptive=1,
                                simps_err=1e-3, w_outlier=0.1):
        """This shard's per-node partial sums and its encoded error count
        (n_nodes + 1 values): what wiener_like_nodes_allreduce sums over ranks."""
        table, keep = self._node_table(params)
        K = self._knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = np.empty(self.n_nodes + 1, dtype=np.float64)
        _lib.check(_lib.wfpt_wiener_like_nodes_local(self.ctx.handle, self.handle, table,
                                                     ctypes.byref(K), _lib.dptr(out)))
        del keep
        return out

    def wiener_like_nodes_allreduce(self, params, err=1e-4, n_st=2, n_sz=2, use_adaptive=1,
                                    simps_err=1e-3, w_outlier=0.1):
        """Per-node sums over every rank's shard (hddm_amd.dist.init_comm):
        one all-reduce of n_nodes + 1 doubles per call.

        The exchange's count is the table's row count, which every rank
        shares; whether this rank's dataset matches it (node ids present,
        n_nodes rows) is checked by the library *inside* the collective, so a
        rank with a bad dataset enters the all-reduce poisoned instead of
        leaving its peers blocked in it."""
        pm = np.ascontiguousarray(params, dtype=np.float64)
        if pm.ndim != 2 or pm.shape[1] != 8:  # the table itself: the same on every rank
            raise ValueError("params must have shape (n_nodes, 8)")
        K = self._knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        m = pm.shape[0]
        out = np.empty(m, dtype=np.float64)
        _lib.check(_lib.wfpt_wiener_like_nodes_allreduce(self.ctx.handle, self.handle,
                                                         pm.ctypes.data_as(_lib._PP), m,
                                                         ctypes.byref(K), _lib.dptr(out)))
        return out

    def wiener_like_nodes_multi(self, tables, err=1e-4, n_st=2, n_sz=2, use_adaptive=1,
                                simps_err=1e-3, w_outlier=0.1, trials=False):
        """T parameter tables in ONE launch: tables (T, n_nodes, 8) -> per-node
        sums (T, n_nodes); row t equals wiener_like_nodes(tables[t]) bit for bit
        (several MCMC chains in lockstep, or both stepping-out probes of a slice
        step). trials=True: (sums, per-trial terms (T, n) in the caller's trial
        order)."""
        tb = np.ascontiguousarray(tables, dtype=np.float64)
        if self.n_nodes == 0:
            raise ValueError("dataset was created without node ids")
        if tb.ndim != 3 or tb.shape[1:] != (self.n_nodes, 8) or tb.shape[0] < 1:
            raise ValueError(f"tables must have shape (T, {self.n_nodes}, 8), T >= 1")
        T = tb.shape[0]
        K, kaddr = self._knobs_addr(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = np.empty((T, self.n_nodes), dtype=np.float64)
        c, h = self.ctx.handle, self.handle
        if trials:
            terms = np.empty((T, self.n), dtype=np.float64)
            _lib.check(_lib.wfpt_wiener_like_nodes_multi_ex(
                c, h, tb.ctypes.data_as(_lib._PP), T, ctypes.byref(K), _lib.dptr(out),
                _lib.dptr(terms)))
            return out, terms
        if not c or not h:  # closed: the C ABI's own argument error
            _lib.check(_lib.wfpt_wiener_like_nodes_multi(c, h, tb.ctypes.data_as(_lib._PP), T,
                                                         ctypes.byref(K), _lib.dptr(out)))
            return out
        # the per-step MCMC call: plain addresses through the raw prototype
        rc = _lib.raw_wiener_like_nodes_multi(c.value, h.value, tb.ctypes.data, T, kaddr,
                                              out.ctypes.data)
        if rc:
            _lib.check(rc)
        return out

    def pointwise_nodes(self, tables, err=1e-4, n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3,
                        w_outlier=0.1, max_workspace=None):
        """The model-comparison pass over S kept sweeps: tables (S, n_nodes, 8)
        -> a dict of `sums` (S, n_nodes), row s bit for bit
        wiener_like_nodes(tables[s]), and per trial, reduced over the sweeps on
        the device, `lppd` (log mean density), `p_waic` (sample variance of the
        log terms), `mean` (mean log term) and `n_inf` (sweeps with a zero
        density), in the caller's trial order (`trial` = arange(n)). The S x n
        terms stay in device memory, scored in tiles of max_workspace bytes
        (default 1 GiB)."""
        tb = np.ascontiguousarray(tables, dtype=np.float64)
        if self.n_nodes == 0:
            raise ValueError("dataset was created without node ids")
        if tb.ndim != 3 or tb.shape[1:] != (self.n_nodes, 8) or tb.shape[0] < 1:
            raise ValueError(f"tables must have shape (S, {self.n_nodes}, 8), S >= 1")
        S = tb.shape[0]
        K = self._knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        sums = np.empty((S, self.n_nodes), dtype=np.float64)
        stats = np.empty((4, self.n), dtype=np.float64)
        ninf = ctypes.c_int64()
        _lib.check(_lib.wfpt_pointwise_nodes(
            self.ctx.handle, self.handle, tb.ctypes.data_as(_lib._PP), S, ctypes.byref(K),
            int(max_workspace or 0), _lib.dptr(sums), _lib.dptr(stats), ctypes.byref(ninf)))
        return _pointwise_result(sums, stats, np.arange(self.n, dtype=np.int64), ninf.value)

    def wiener_like_nodes(self, params, err=1e-4, n_st=2, n_sz=2, use_adaptive=1,
                          simps_err=1e-3, w_outlier=0.1, trials=False):
        """params: array (n_nodes, 8) of v, sv, a, z, sz, t, st, p_outlier.
        Returns the per-node summed log-likelihoods (float64[n_nodes]);
        trials=True: (per-node sums, per-trial log terms in the order the
        trials were given to the Dataset)."""
        pm = np.ascontiguousarray(params, dtype=np.float64)
        if self.n_nodes == 0:
            raise ValueError("dataset was created without node ids")
        if pm.shape != (self.n_nodes, 8):
            raise ValueError(f"params must have shape ({self.n_nodes}, 8)")
        K, kaddr = self._knobs_addr(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = np.empty(self.n_nodes, dtype=np.float64)
        c, h = self.ctx.handle, self.handle
        if trials:
            terms = np.empty(self.n, dtype=np.float64)
            _lib.check(_lib.wfpt_wiener_like_nodes_ex(c, h, pm.ctypes.data_as(_lib._PP),
                                                      ctypes.byref(K), _lib.dptr(out),
                                                      _lib.dptr(terms)))
            return out, terms
        if not c or not h:  # closed: the C ABI's own argument error
            _lib.check(_lib.wfpt_wiener_like_nodes(c, h, pm.ctypes.data_as(_lib._PP),
                                                   ctypes.byref(K), _lib.dptr(out)))
            return out
        # the per-step MCMC call: plain addresses through the raw prototype
        rc = _lib.raw_wiener_like_nodes(c.value, h.value, pm.ctypes.data, kaddr, out.ctypes.data)
        if rc:
            _lib.check(rc)
        return out


# ---------------------------------------------------------------------------
# Reinforcement-learning family (src/wfpt.pyx:79-241, 277-320)

def _check_long(a, name):
    """Cython `np.ndarray[long, ndim=1]` argument semantics."""
    if not isinstance(a, np.ndarray):
        raise TypeError(f"Argument '{name}' has incorrect type (expected numpy.ndarray, got "
                        f"{type(a).__name__})")
    if a.dtype != np.int64:
        raise ValueError(f"Buffer dtype mismatch, expected 'long' but got {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"Buffer has wrong number of dimensions (expected 1, got {a.ndim})")
    return np.ascontiguousarray(a)


def _same_length(n, **arrays):
    for nm, arr in arrays.items():
        if arr.shape[0] != n:
            raise ValueError(f"{nm} must have one entry per trial ({n}), got {arr.shape[0]}")


def _rl_outputs(n, terms):
    """The optional per-trial terms and drifts of an RL call, and their pointers."""
    if not terms:
        return None, None, None, None
    tr = np.empty(n, dtype=np.float64)
    dr = np.empty(n, dtype=np.float64)
    return tr, dr, _lib.dptr(tr), _lib.dptr(dr)


def _like_multi_rlddm(ctx, rt, response, feedback, split_by, q, vals, err, multi, n_st, n_sz,
                      use_adaptive, simps_err, p_outlier, w_outlier, terms):
    """wiener_like_multi_rlddm (wfpt.pyx:277-320) from host arrays, on `ctx`
    or, with ctx None, the process-wide context; vals: v, sv, a, z, sz, t, st,
    alpha. terms: (sum, per-trial terms, per-trial drifts)."""
    if multi is None:
        return full_pdf(rt, *vals[:7], err)  # wfpt.pyx:293-294 (TypeError for arrays)
    n = rt.shape[0]
    _same_length(n, response=response, feedback=feedback, split_by=split_by)
    ptrs, scal, keep = _multi_args(n, _MULTI_NAMES + ("alpha",), vals, multi)  # wfpt.pyx:296
    c = ctx if ctx is not None else _lib.context()
    K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
    out = ctypes.c_double()
    tr, dr, ptr, pdr = _rl_outputs(n, terms)
    _lib.check(_lib.wfpt_wiener_like_multi_rlddm_ex(
        c.handle, _lib.dptr(rt), _i64ptr(response), _lib.dptr(feedback), _i64ptr(split_by), n,
        float(q), ptrs, _lib.dptr(scal), ctypes.byref(K), float(p_outlier), ctypes.byref(out),
        ptr, pdr))
    del keep
    return (out.value, tr, dr) if terms else out.value


class RLDataset(_Resident):
    """The fixed inputs of the RL likelihoods (RT, response, feedback,
    condition) resident in HBM: per call only the scalars go to the device.
    `rt` may be None for the choice-only model (wiener_like_rl). Optional
    `node_id` groups trials into `n_nodes` likelihood nodes scored together by
    `wiener_like_rlddm_nodes`. |rt| == 999 is rejected (ValueError): the RL
    likelihoods have no missing-response code."""
    _destroy = staticmethod(_lib.wfpt_rl_dataset_destroy)

    def __init__(self, rt, response, feedback, split_by, node_id=None, n_nodes=None, device=None,
                 ctx=None):
        response = np.ascontiguousarray(np.asarray(response, dtype=np.int64).ravel())
        n = response.shape[0]
        feedback = np.ascontiguousarray(np.asarray(feedback, dtype=np.float64).ravel())
        split_by = np.ascontiguousarray(np.asarray(split_by, dtype=np.int64).ravel())
        _same_length(n, feedback=feedback, split_by=split_by)
        if rt is not None:
            rt = np.ascontiguousarray(np.asarray(rt, dtype=np.float64).ravel())
            _same_length(n, rt=rt)
        self.ctx = ctx if ctx is not None else _lib.context(device)
        self.n = n
        self._host = (rt, response, feedback, split_by)
        node, self.n_nodes, nptr = None, 0, None
        if node_id is not None:
            node, self.n_nodes, nptr = _id_array(node_id, n_nodes)
            _same_length(n, node_id=node)
        # the scored trials: all but the first of each (node, condition) segment
        key = np.stack([node if node is not None else np.zeros(n, dtype=np.int64), split_by])
        self.n_scored = n - (np.unique(key, axis=1).shape[1] if n else 0)
        h = _lib._VP()
        _lib.check(_lib.wfpt_rl_dataset_create(
            self.ctx.handle, _optr(rt), _i64ptr(response), _lib.dptr(feedback), _i64ptr(split_by),
            n, nptr, self.n_nodes, ctypes.byref(h)))
        self.handle = h

    def wiener_like_rlddm(self, q, alpha, pos_alpha, v, sv, a, z, sz, t, st, err, n_st=10,
                          n_sz=10, use_adaptive=1, simps_err=1e-8, p_outlier=0, w_outlier=0,
                          terms=False):
        """wiener_like_rlddm (wfpt.pyx:79-154) over the resident trials.
        terms=True: (sum, per-trial terms, per-trial drifts), caller order."""
        P = _lib.make_params(v, sv, a, z, sz, t, st, p_outlier)
        K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = ctypes.c_double()
        tr, dr, ptr, pdr = _rl_outputs(self.n, terms)
        _lib.check(_lib.wfpt_wiener_like_rlddm_ex(
            self.ctx.handle, self.handle, float(q), float(alpha), float(pos_alpha),
            ctypes.byref(P), ctypes.byref(K), ctypes.byref(out), ptr, pdr))
        return (out.value, tr, dr) if terms else out.value

    def wiener_like_rl(self, q, alpha, pos_alpha, v, z, err=1e-4, n_st=10, n_sz=10,
                       use_adaptive=1, simps_err=1e-8, p_outlier=0, w_outlier=0, terms=False):
        """wiener_like_rl (wfpt.pyx:157-241): err, n_st, n_sz, use_adaptive and
        simps_err are accepted and ignored, as in the reference."""
        out = ctypes.c_double()
        tr, dr, ptr, pdr = _rl_outputs(self.n, terms)
        _lib.check(_lib.wfpt_wiener_like_rl_ex(
            self.ctx.handle, self.handle, float(q), float(alpha), float(pos_alpha), float(v),
            float(z), float(p_outlier), float(w_outlier), ctypes.byref(out), ptr, pdr))
        return (out.value, tr, dr) if terms else out.value

    def wiener_like_multi_rlddm(self, q, v, sv, a, z, sz, t, st, alpha, err, multi=None, n_st=10,
                                n_sz=10, use_adaptive=1, simps_err=1e-3, p_outlier=0,
                                w_outlier=0, terms=False):
        """wiener_like_multi_rlddm (wfpt.pyx:277-320). Its segments (runs of
        equal adjacent split_by) and per-trial arrays differ per model, so this
        call works from the host copies, not the resident layout."""
        rt, response, feedback, split_by = self._host
        if rt is None:
            raise ValueError("wiener_like_multi_rlddm needs RTs")
        return _like_multi_rlddm(self.ctx, rt, response, feedback, split_by, q,
                                 (v, sv, a, z, sz, t, st, alpha), err, multi, n_st, n_sz,
                                 use_adaptive, simps_err, p_outlier, w_outlier, terms)

    def wiener_like_rlddm_nodes(self, rl_rows, params, err=1e-4, n_st=2, n_sz=2, use_adaptive=1,
                                simps_err=1e-3, w_outlier=0.1, terms=False):
        """One wiener_like_rlddm per node in one scan + one scoring pass:
        rl_rows (n_nodes, 3) of q, alpha, pos_alpha; params (n_nodes, 8) of v,
        sv, a, z, sz, t, st, p_outlier (one p_outlier for all nodes). Returns
        the per-node sums; terms=True: (sums, per-trial terms, drifts)."""
        if self.n_nodes == 0:
            raise ValueError("dataset was created without node ids")
        rr = np.ascontiguousarray(rl_rows, dtype=np.float64)
        pm = np.ascontiguousarray(params, dtype=np.float64)
        if rr.shape != (self.n_nodes, 3):
            raise ValueError(f"rl_rows must have shape ({self.n_nodes}, 3)")
        if pm.shape != (self.n_nodes, 8):
            raise ValueError(f"params must have shape ({self.n_nodes}, 8)")
        K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = np.empty(self.n_nodes, dtype=np.float64)
        tr, dr, ptr, pdr = _rl_outputs(self.n, terms)
        _lib.check(_lib.wfpt_wiener_like_rlddm_nodes_ex(
            self.ctx.handle, self.handle, _lib.dptr(rr), pm.ctypes.data_as(_lib._PP),
            ctypes.byref(K), _lib.dptr(out), ptr, pdr))
        return (out, tr, dr) if terms else out

    def wiener_like_rlddm_nodes_multi(self, rl_tables, params, err=1e-4, n_st=2, n_sz=2,
                                      use_adaptive=1, simps_err=1e-3, w_outlier=0.1, terms=False):
        """wiener_like_rlddm_nodes for T row tables in ONE call (both probes of
        a slice step): rl_tables (T, n_nodes, 3), params (T, n_nodes, 8), one
        p_outlier throughout. Returns the (T, n_nodes) sums, row t bit for bit
        the one-table call's on table t; terms=True: (sums, (T, n) per-trial
        terms, (T, n) drifts)."""
        if self.n_nodes == 0:
            raise ValueError("dataset was created without node ids")
        rr = np.ascontiguousarray(rl_tables, dtype=np.float64)
        pm = np.ascontiguousarray(params, dtype=np.float64)
        if rr.ndim != 3 or rr.shape[0] < 1 or rr.shape[1:] != (self.n_nodes, 3):
            raise ValueError(f"rl_tables must have shape (T, {self.n_nodes}, 3) with T >= 1")
        T = rr.shape[0]
        if pm.shape != (T, self.n_nodes, 8):
            raise ValueError(f"params must have shape ({T}, {self.n_nodes}, 8)")
        K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = np.empty((T, self.n_nodes), dtype=np.float64)
        tr, dr, ptr, pdr = _rl_outputs((T, self.n), terms)
        _lib.check(_lib.wfpt_wiener_like_rlddm_nodes_multi_ex(
            self.ctx.handle, self.handle, _lib.dptr(rr), pm.ctypes.data_as(_lib._PP), T,
            ctypes.byref(K), _lib.dptr(out), ptr, pdr))
        return (out, tr, dr) if terms else out

    def pointwise_rlddm_nodes(self, rl_tables, params, err=1e-4, n_st=2, n_sz=2, use_adaptive=1,
                              simps_err=1e-3, w_outlier=0.1, max_workspace=None):
        """Dataset.pointwise_nodes over the multi-table RL node batch: rl_tables
        (S, n_nodes, 3), params (S, n_nodes, 8), one p_outlier throughout. The
        per-trial entries cover the scored trials only (all but each segment's
        first); `trial` is the caller's index of each entry."""
        if self.n_nodes == 0:
            raise ValueError("dataset was created without node ids")
        rr = np.ascontiguousarray(rl_tables, dtype=np.float64)
        pm = np.ascontiguousarray(params, dtype=np.float64)
        if rr.ndim != 3 or rr.shape[0] < 1 or rr.shape[1:] != (self.n_nodes, 3):
            raise ValueError(f"rl_tables must have shape (S, {self.n_nodes}, 3) with S >= 1")
        S = rr.shape[0]
        if pm.shape != (S, self.n_nodes, 8):
            raise ValueError(f"params must have shape ({S}, {self.n_nodes}, 8)")
        K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        sums = np.empty((S, self.n_nodes), dtype=np.float64)
        m = self.n_scored
        stats = np.empty((4, m), dtype=np.float64)
        index = np.empty(m, dtype=np.int64)
        ninf = ctypes.c_int64()
        _lib.check(_lib.wfpt_pointwise_rlddm_nodes(
            self.ctx.handle, self.handle, _lib.dptr(rr), pm.ctypes.data_as(_lib._PP), S,
            ctypes.byref(K), int(max_workspace or 0), _lib.dptr(sums), _lib.dptr(stats),
            _i64ptr(index), ctypes.byref(ninf)))
        return _pointwise_result(sums, stats, index, ninf.value)


# ---------------------------------------------------------------------------
# Regression likelihoods (hddm/models/hddm_regression.py:26-36)

REG_PARAMS = ("v", "sv", "a", "z", "sz", "t", "st")
REG_LINKS = {"identity": _lib.LINK_IDENTITY, "exp": _lib.LINK_EXP,
             "invlogit": _lib.LINK_INVLOGIT}


def _reg_terms(model, n_cols, params=REG_PARAMS):
    """[(param_name, col0, ncol, link_name), ...] -> a wfpt_reg_term array.
    Checks that need no device: known names, one term per parameter, column
    ranges inside the design matrix. params: the names a term may predict, in
    wfpt_reg_term.param order (RLRegDataset adds alpha)."""
    model = list(model)
    arr = (_lib.RegTerm * max(len(model), 1))()
    seen = set()
    for k, term in enumerate(model):
        try:
            name, col0, ncol, link = term
        except (TypeError, ValueError):
            raise ValueError("a model term is (param_name, col0, ncol, link_name)")
        if name not in params:
            raise ValueError(f"unknown parameter {name!r}; expected one of {params}")
        if name in seen:
            raise ValueError(f"parameter {name!r} is named twice")
        seen.add(name)
        if link not in REG_LINKS:
            raise ValueError(f"unknown link {link!r}; the link runs on the device and is one "
                             f"of {tuple(REG_LINKS)}")
        col0, ncol = int(col0), int(ncol)
        if ncol < 1 or col0 < 0 or col0 + ncol > n_cols:
            raise ValueError(f"columns [{col0}, {col0 + ncol}) of term {name!r} lie outside "
                             f"the design matrix's {n_cols} columns")
        arr[k] = _lib.RegTerm(params.index(name), REG_LINKS[link], col0, ncol)
    return arr, len(model)


class RegDataset(_Resident):
    """The fixed inputs of a regression likelihood (signed RTs and the design
    matrix) resident in HBM: per call only the coefficients go to the device,
    and the trial-wise parameters link(design . coefficients) are formed there.
    `design` is an (n, C) array or DataFrame. Optional `group_id` groups the
    trials into `n_groups` groups (subjects) scored together by
    `wiener_like_reg_groups`. |rt| == 999 is a missing response, as in
    wiener_like_multi (wfpt.pyx:261-270)."""
    _destroy = staticmethod(_lib.wfpt_reg_dataset_destroy)

    def __init__(self, rt, design, group_id=None, n_groups=None, device=None, ctx=None):
        rt = np.ascontiguousarray(np.asarray(rt, dtype=np.float64).ravel())
        n = rt.shape[0]
        self.columns = list(getattr(design, "columns", ()))
        X = np.ascontiguousarray(np.asarray(design, dtype=np.float64))
        if X.ndim != 2 or X.shape[0] != n or X.shape[1] < 1:
            raise ValueError(f"design must have shape ({n}, C) with C >= 1, got {X.shape}")
        node, self.n_groups, nptr = None, 1, None
        if group_id is not None:
            node, self.n_groups, nptr = _id_array(group_id, n_groups)
            _same_length(n, group_id=node)
            if self.n_groups < 1:
                raise ValueError("group ids need n_groups >= 1")
            if node.size and (node.min() < 0 or node.max() >= self.n_groups):
                raise ValueError(f"group ids must lie in [0, {self.n_groups})")
        self.n = n
        self.n_cols = int(X.shape[1])
        self.grouped = group_id is not None
        self.ctx = ctx if ctx is not None else _lib.context(device)
        h = _lib._VP()
        _lib.check(_lib.wfpt_reg_dataset_create(
            self.ctx.handle, _lib.dptr(rt), n, _lib.dptr(X), self.n_cols, nptr, self.n_groups,
            ctypes.byref(h)))
        self.handle = h

    def _outputs(self, terms, n_terms):
        if not terms:
            return None, None, None, None
        tr = np.empty(self.n, dtype=np.float64)
        pr = np.empty((max(n_terms, 1), self.n), dtype=np.float64)
        return tr, pr, _lib.dptr(tr), _lib.dptr(pr)

    def wiener_like_reg(self, model, coef, v, sv, a, z, sz, t, st, err, n_st=10, n_sz=10,
                        use_adaptive=1, simps_err=1e-3, p_outlier=0, w_outlier=0, terms=False):
        """The reference's regression node (hddm_regression.py:26-36 into
        wiener_like_multi, wfpt.pyx:244-274) over the resident trials: `model`
        is a list of (param_name, col0, ncol, link_name), `coef` one
        coefficient per design column; a regressed parameter's scalar argument
        is ignored. terms=True: (sum, per-trial terms, {param: predicted
        array}), caller order."""
        model = list(model)
        T, nt = _reg_terms(model, self.n_cols)
        b = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).ravel())
        if b.shape != (self.n_cols,):
            raise ValueError(f"coef must have one entry per design column ({self.n_cols})")
        P = _lib.make_params(v, sv, a, z, sz, t, st, p_outlier)
        K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = ctypes.c_double()
        tr, pr, ptr, ppr = self._outputs(terms, nt)
        _lib.check(_lib.wfpt_wiener_like_reg_ex(
            self.ctx.handle, self.handle, T, nt, _lib.dptr(b), ctypes.byref(P), ctypes.byref(K),
            ctypes.byref(out), ptr, ppr))
        if not terms:
            return out.value
        return out.value, tr, {m[0]: pr[k] for k, m in enumerate(model)}

    def wiener_like_reg_groups(self, model, coef_table, params, err=1e-4, n_st=2, n_sz=2,
                               use_adaptive=1, simps_err=1e-3, w_outlier=0.1, terms=False):
        """One regression node per group in one fill launch and one scoring
        pass: coef_table (G, C) one coefficient row per group, params (G, 8) of
        v, sv, a, z, sz, t, st, p_outlier (one p_outlier for all groups).
        Returns the (G,) per-group sums; terms=True: (sums, per-trial terms,
        {param: predicted array})."""
        model = list(model)
        T, nt = _reg_terms(model, self.n_cols)
        G = self.n_groups
        bt = np.ascontiguousarray(coef_table, dtype=np.float64)
        pm = np.ascontiguousarray(params, dtype=np.float64)
        if bt.shape != (G, self.n_cols):
            raise ValueError(f"coef_table must have shape ({G}, {self.n_cols})")
        if pm.shape != (G, 8):
            raise ValueError(f"params must have shape ({G}, 8)")
        K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = np.empty(G, dtype=np.float64)
        tr, pr, ptr, ppr = self._outputs(terms, nt)
        _lib.check(_lib.wfpt_wiener_like_reg_groups_ex(
            self.ctx.handle, self.handle, T, nt, _lib.dptr(bt), pm.ctypes.data_as(_lib._PP),
            ctypes.byref(K), _lib.dptr(out), ptr, ppr))
        if not terms:
            return out
        return out, tr, {m[0]: pr[k] for k, m in enumerate(model)}

    def pointwise_reg_groups(self, model, coef_tables, params, err=1e-4, n_st=2, n_sz=2,
                             use_adaptive=1, simps_err=1e-3, w_outlier=0.1, max_workspace=None):
        """Dataset.pointwise_nodes over the regression groups call: coef_tables
        (S, G, C), params (S, G, 8), one p_outlier per sweep. `sums` is (S, G);
        the per-trial entries are in the caller's trial order. The groups call
        scores one table, so a tile is one sweep; the accumulator state stays
        on the device between sweeps."""
        model = list(model)
        T, nt = _reg_terms(model, self.n_cols)
        G = self.n_groups
        bt = np.ascontiguousarray(coef_tables, dtype=np.float64)
        pm = np.ascontiguousarray(params, dtype=np.float64)
        if bt.ndim != 3 or bt.shape[0] < 1 or bt.shape[1:] != (G, self.n_cols):
            raise ValueError(f"coef_tables must have shape (S, {G}, {self.n_cols}) with S >= 1")
        S = bt.shape[0]
        if pm.shape != (S, G, 8):
            raise ValueError(f"params must have shape ({S}, {G}, 8)")
        K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        sums = np.empty((S, G), dtype=np.float64)
        stats = np.empty((4, self.n), dtype=np.float64)
        ninf = ctypes.c_int64()
        _lib.check(_lib.wfpt_pointwise_reg_groups(
            self.ctx.handle, self.handle, T, nt, _lib.dptr(bt), pm.ctypes.data_as(_lib._PP), S,
            ctypes.byref(K), int(max_workspace or 0), _lib.dptr(sums), _lib.dptr(stats),
            ctypes.byref(ninf)))
        return _pointwise_result(sums, stats, np.arange(self.n, dtype=np.int64), ninf.value)

    # The posterior predictive's trial-wise drift sampler
    # (wfpt_gen_rts_reg_drift).

    def _sim_prep(self, model, coef_tables, params, dt, intra_sv, seed, max_t, unfinished,
                  invalid, wave_draws, max_workspace):
        """The checked arguments of gen_rts_drift[_stats], none of which needs
        the device: (terms, n_terms, coef (S, G, C), params (S, G, 8), S, dt,
        intra_sv, max_steps, seed, wave_draws, workspace bytes)."""
        T, nt = _reg_terms(model, self.n_cols)
        G, C = self.n_groups, self.n_cols
        bt = np.ascontiguousarray(coef_tables, dtype=np.float64)
        pm = np.ascontiguousarray(params, dtype=np.float64)
        bt = bt[None] if bt.ndim == 2 else bt
        pm = pm[None] if pm.ndim == 2 else pm
        if bt.ndim != 3 or bt.shape[0] < 1 or bt.shape[1:] != (G, C):
            raise ValueError(f"coef_tables must have shape (S, {G}, {C}) with S >= 1, or "
                             f"({G}, {C})")
        S = bt.shape[0]
        if pm.shape != (S, G, 8):
            raise ValueError(f"params must have shape ({S}, {G}, 8)")
        dt, intra_sv, max_steps, _ = _drift_prep(S * G, dt, intra_sv, None, max_t, unfinished)
        if invalid not in ("raise", "nan"):
            raise ValueError("invalid must be 'raise' or 'nan'")
        wd = 0 if wave_draws is None else int(wave_draws)
        if wd < 0 or wd % 64:
            raise ValueError("wave_draws must be a positive multiple of 64")
        ws = 0 if max_workspace is None else int(max_workspace)
        if ws < 0:
            raise ValueError("max_workspace must be positive")
        return T, nt, bt, pm, S, dt, intra_sv, max_steps, _drift_seed(seed), wd, ws

    def _sim_done(self, rc, nun, ninv, S, max_steps, max_t, unfinished, invalid):
        _lib.check(rc)
        if ninv.value and invalid == "raise":
            raise RuntimeError(f"wfpt_amd: {ninv.value} of {S * self.n} (sweep, trial) pairs have "
                               "parameters that cannot be simulated (a non-finite parameter, "
                               "a <= 0, or a start point outside [0, 1])")
        _check_finished(nun.value, S * self.n, max_steps, max_t, unfinished)

    def gen_rts_drift(self, model, coef_tables, params, dt=1e-4, intra_sv=1., seed=None,
                      max_t=20., unfinished='raise', invalid='raise', return_debug=False,
                      wave_draws=None, max_workspace=None):
        """The regression node's random() (hddm_regression.py:39-56: one
        simulated diffusion path per trial at the trial's own parameters,
        generate.py:208-319) for S sweeps in one call (wfpt_gen_rts_reg_drift):
        the trial-wise parameters are formed on the device from the resident
        design matrix at the moment a lane walks the (sweep, trial).

        model: wiener_like_reg_groups' term list. coef_tables (S, G, C) and
        params (S, G, 8): sweep s's coefficient and parameter row of each
        group (2-D: one sweep; a regressed parameter's column and p_outlier
        are ignored). Returns the (S, n) signed RTs in the caller's order.

        seed: the device's Philox4x32-10 streams (None: from NumPy's global
        RNG). Trial i of sweep s is bit for bit draw s of row i of
        gen_rts_from_drift_nodes over the trials' parameters: it depends on
        (seed, s, i) only, not on the grouping. A walk cut after
        ceil(max_t / dt) steps is NaN (unfinished='raise': RuntimeError with
        the count); so is a trial whose parameters cannot be walked, e.g. a
        predicted a <= 0 (invalid='raise': RuntimeError with the count).

        return_debug: also a dict of `params` (S, n, 7) the formed v, sv, a,
        z, sz, t, st, and `y0`, `delay`, `drift`, `n_steps` (S, n).
        wave_draws (elements handed to one wave, a multiple of 64; with
        return_debug then also `wave_steps`) and max_workspace (device bytes
        for the draws, default 1 GiB: more sweeps run in tiles) change no
        value."""
        T, nt, bt, pm, S, dt, intra_sv, max_steps, seed, wd, ws = self._sim_prep(
            model, coef_tables, params, dt, intra_sv, seed, max_t, unfinished, invalid,
            wave_draws, max_workspace)
        n = self.n
        out = np.empty((S, n), dtype=np.float64)
        nun, ninv = ctypes.c_int64(), ctypes.c_int64()
        head = (self.ctx.handle, self.handle, T, nt, _lib.dptr(bt), pm.ctypes.data_as(_lib._PP), S,
                dt, intra_sv, max_steps, seed)
        if return_debug or wd or ws:
            dbg = {}
            if return_debug:
                dbg["params"] = np.empty((S, n, 7))
                dbg.update((k, np.empty((S, n))) for k in ("y0", "delay", "drift"))
                dbg["n_steps"] = np.empty((S, n), dtype=np.int64)
                if wd:
                    dbg["wave_steps"] = np.empty(-(-S * n // wd), dtype=np.int64)
            i64 = {k: _i64ptr(dbg[k]) if k in dbg else None for k in ("n_steps", "wave_steps")}
            rc = _lib.wfpt_gen_rts_reg_drift_ex(
                *head, wd, ws, _lib.dptr(out), ctypes.byref(nun), ctypes.byref(ninv),
                _optr(dbg.get("params")), _optr(dbg.get("y0")), _optr(dbg.get("delay")),
                _optr(dbg.get("drift")), i64["n_steps"], i64["wave_steps"])
        else:
            rc = _lib.wfpt_gen_rts_reg_drift(*head, _lib.dptr(out), ctypes.byref(nun),
                                             ctypes.byref(ninv))
        self._sim_done(rc, nun, ninv, S, max_steps, max_t, unfinished, invalid)
        return (out, dbg) if return_debug else out

    def gen_rts_drift_stats(self, model, coef_tables, params, dt=1e-4, intra_sv=1., seed=None,
                            max_t=20., unfinished='raise', invalid='raise',
                            quantiles=PPC_QUANTILES, return_draws=False, max_workspace=None):
        """gen_rts_drift's draws (same arguments, same seed: the same draws)
        reduced to rt_stats_rows' statistics per (sweep, group) while they are
        still in device memory (wfpt_gen_rts_reg_drift_stats): returns (S, G,
        8 + 2 len(quantiles)) in rt_stats_names' order, and with
        return_draws=True also the (S, n) draws."""
        q = _check_quantiles(quantiles)
        T, nt, bt, pm, S, dt, intra_sv, max_steps, seed, _, ws = self._sim_prep(
            model, coef_tables, params, dt, intra_sv, seed, max_t, unfinished, invalid, None,
            max_workspace)
        stats = np.empty((S, self.n_groups, 8 + 2 * q.size))
        out = np.empty((S, self.n), dtype=np.float64) if return_draws else None
        nun, ninv = ctypes.c_int64(), ctypes.c_int64()
        rc = _lib.wfpt_gen_rts_reg_drift_stats(
            self.ctx.handle, self.handle, T, nt, _lib.dptr(bt), pm.ctypes.data_as(_lib._PP), S, dt,
            intra_sv, max_steps, seed, ws, _optr(out), ctypes.byref(nun), ctypes.byref(ninv),
            _lib.dptr(q), q.size, _lib.dptr(stats))
        self._sim_done(rc, nun, ninv, S, max_steps, max_t, unfinished, invalid)
        return (stats, out) if return_draws else stats


# ---------------------------------------------------------------------------
# RL regression likelihood (hddm/models/hddm_rl_regression.py:25-38)

RL_REG_PARAMS = REG_PARAMS + ("alpha",)


class RLRegDataset(_Resident):
    """The fixed inputs of the RL regression likelihood resident in HBM: signed
    RTs, responses, feedback, conditions and the design matrix. Per call only
    the coefficients and a few rows per group go to the device; the trial-wise
    parameters link(design . coefficients), the learning rate's `alpha` among
    them, are formed there. Optional `group_id` groups the trials into
    `n_groups` groups (subjects), each scored as one wiener_like_multi_rlddm
    call (wfpt.pyx:277-320) would score its trials: Q restarts at every
    adjacent change of split_by inside a group and at every group boundary.
    |rt| == 999 and a response outside {0, 1} are rejected (ValueError)."""
    _destroy = staticmethod(_lib.wfpt_rl_reg_dataset_destroy)

    def __init__(self, rt, response, feedback, split_by, design, group_id=None, n_groups=None,
                 device=None, ctx=None):
        rt = np.ascontiguousarray(np.asarray(rt, dtype=np.float64).ravel())
        n = rt.shape[0]
        response = np.ascontiguousarray(np.asarray(response, dtype=np.int64).ravel())
        feedback = np.ascontiguousarray(np.asarray(feedback, dtype=np.float64).ravel())
        split_by = np.ascontiguousarray(np.asarray(split_by, dtype=np.int64).ravel())
        _same_length(n, response=response, feedback=feedback, split_by=split_by)
        self.columns = list(getattr(design, "columns", ()))
        X = np.ascontiguousarray(np.asarray(design, dtype=np.float64))
        if X.ndim != 2 or X.shape[0] != n or X.shape[1] < 1:
            raise ValueError(f"design must have shape ({n}, C) with C >= 1, got {X.shape}")
        if np.any((response != 0) & (response != 1)):
            raise ValueError("response must be 0 or 1")
        if np.any(np.abs(rt) == 999.):
            raise ValueError("|rt| == 999: the RL likelihoods have no missing-response code")
        node, self.n_groups, nptr = None, 1, None
        if group_id is not None:
            node, self.n_groups, nptr = _id_array(group_id, n_groups)
            _same_length(n, group_id=node)
            if self.n_groups < 1:
                raise ValueError("group ids need n_groups >= 1")
            if node.size and (node.min() < 0 or node.max() >= self.n_groups):
                raise ValueError(f"group ids must lie in [0, {self.n_groups})")
        self.n = n
        self.n_cols = int(X.shape[1])
        self.grouped = group_id is not None
        self.ctx = ctx if ctx is not None else _lib.context(device)
        h = _lib._VP()
        _lib.check(_lib.wfpt_rl_reg_dataset_create(
            self.ctx.handle, _lib.dptr(rt), _i64ptr(response), _lib.dptr(feedback),
            _i64ptr(split_by), n, _lib.dptr(X), self.n_cols, nptr, self.n_groups,
            ctypes.byref(h)))
        self.handle = h

    def _check_groups(self, model, coef_table, q, alpha, params):
        """The arguments of a groups call as contiguous arrays, every shape
        checked before any device work."""
        T, nt = _reg_terms(model, self.n_cols, RL_REG_PARAMS)
        G = self.n_groups
        bt = np.ascontiguousarray(coef_table, dtype=np.float64)
        pm = np.ascontiguousarray(params, dtype=np.float64)
        if bt.shape != (G, self.n_cols):
            raise ValueError(f"coef_table must have shape ({G}, {self.n_cols})")
        if pm.shape != (G, 8):
            raise ValueError(f"params must have shape ({G}, 8)")
        rows = []
        for name, val in (("q", q), ("alpha", alpha)):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(val, dtype=np.float64), (G,))
                                     if np.ndim(val) == 0 else np.asarray(val, dtype=np.float64))
            if a.shape != (G,):
                raise ValueError(f"{name} must have one entry per group ({G})")
            rows.append(a)
        return T, nt, bt, rows[0], rows[1], pm

    def wiener_like_rl_reg_groups(self, model, coef_table, q, alpha, params, err=1e-4, n_st=2,
                                  n_sz=2, use_adaptive=1, simps_err=1e-3, w_outlier=0.1,
                                  terms=False):
        """One RL regression node per group in one fill launch, one Q scan and
        one scoring pass: `model` is a list of (param_name, col0, ncol,
        link_name) with param_name one of v, sv, a, z, sz, t, st, alpha;
        coef_table (G, C) one coefficient row per group; q (G,) the start of
        both Q values; alpha (G,) the unbounded learning-rate parameter,
        ignored when alpha is regressed; params (G, 8) of v, sv, a, z, sz, t,
        st, p_outlier (one p_outlier for all groups), v the drift scaling
        unless regressed. Returns the (G,) per-group sums; terms=True: (sums,
        per-trial terms, {param: predicted array}, drifts, learning rates) in
        the caller's order, the alpha prediction after the link and before
        squashing. A regressed alpha's rate is correctly rounded and can
        differ from the reference's libm value by an ulp of the power
        (DESIGN.md §25)."""
        model = list(model)
        T, nt, bt, qa, al, pm = self._check_groups(model, coef_table, q, alpha, params)
        K = _lib.make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier)
        out = np.empty(self.n_groups, dtype=np.float64)
        tr = pr = dr = ra = None
        if terms:
            tr, dr, ra = (np.empty(self.n, dtype=np.float64) for _ in range(3))
            pr = np.empty((max(nt, 1), self.n), dtype=np.float64)
        _lib.check(_lib.wfpt_wiener_like_rl_reg_groups_ex(
            self.ctx.handle, self.handle, T, nt, _lib.dptr(bt), _lib.dptr(qa), _lib.dptr(al),
            pm.ctypes.data_as(_lib._PP), ctypes.byref(K), _lib.dptr(out), _optr(tr), _optr(pr),
            _optr(dr), _optr(ra)))
        if not terms:
            return out
        return out, tr, {m[0]: pr[k] for k, m in enumerate(model)}, dr, ra

    def wiener_like_rl_reg(self, model, coef, q, alpha, v, sv, a, z, sz, t, st, err, n_st=10,
                           n_sz=10, use_adaptive=1, simps_err=1e-3, p_outlier=0, w_outlier=0,
                           terms=False):
        """The reference's node (hddm_rl_regression.py:25-38) over all resident
        trials of a data set made without group ids: one coefficient vector,
        scalar q, alpha and parameters. Returns the sum; terms=True as
        wiener_like_rl_reg_groups."""
        if self.grouped:
            raise ValueError("wiener_like_rl_reg needs a data set made without group ids")
        b = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).ravel())
        if b.shape != (self.n_cols,):
            raise ValueError(f"coef must have one entry per design column ({self.n_cols})")
        P = np.array([[v, sv, a, z, sz, t, st, p_outlier]], dtype=np.float64)
        r = self.wiener_like_rl_reg_groups(model, b[None, :], [float(q)], [float(alpha)], P, err,
                                           n_st, n_sz, use_adaptive, simps_err, w_outlier, terms)
        return (float(r[0][0]),) + r[1:] if terms else float(r[0])


def _rl_host(x, response, feedback, split_by, x_optional=False):
    """The RL functions' arrays, checked as Cython checks them, in the
    reference's argument order."""
    if not (x_optional and x is None):
        x = _check_x(x)
    return (x, _check_long(response, "response"), _check_x(feedback, "feedback"),
            _check_long(split_by, "split_by"))


def _on_rl_dataset(method, x, response, feedback, split_by, *args, **kw):
    """An RLDataset method over a transient dataset of the checked arrays."""
    ds = RLDataset(*_rl_host(x, response, feedback, split_by, x_optional=True))
    try:
        return method(ds, *args, **kw)
    finally:
        ds.close()


def wiener_like_rlddm(x, response, feedback, split_by, q, alpha, pos_alpha, v, sv, a, z, sz, t,
                      st, err, n_st=10, n_sz=10, use_adaptive=1, simps_err=1e-8, p_outlier=0,
                      w_outlier=0):
    return _on_rl_dataset(RLDataset.wiener_like_rlddm, x, response, feedback, split_by, q, alpha,
                          pos_alpha, v, sv, a, z, sz, t, st, err, n_st, n_sz, use_adaptive,
                          simps_err, p_outlier, w_outlier)


def wiener_like_rlddm_terms(x, response, feedback, split_by, q, alpha, pos_alpha, v, sv, a, z,
                            sz, t, st, err, n_st=10, n_sz=10, use_adaptive=1, simps_err=1e-8,
                            p_outlier=0, w_outlier=0):
    """wiener_like_rlddm returning (sum, terms, drift): terms[i] is trial i's
    log term (0.0 for the unscored first trial of a condition), drift[i] the
    drift the recurrence holds when it reaches trial i."""
    return _on_rl_dataset(RLDataset.wiener_like_rlddm, x, response, feedback, split_by, q, alpha,
                          pos_alpha, v, sv, a, z, sz, t, st, err, n_st, n_sz, use_adaptive,
                          simps_err, p_outlier, w_outlier, terms=True)


def wiener_like_rl(response, feedback, split_by, q, alpha, pos_alpha, v, z, err=1e-4, n_st=10,
                   n_sz=10, use_adaptive=1, simps_err=1e-8, p_outlier=0, w_outlier=0):
    return _on_rl_dataset(RLDataset.wiener_like_rl, None, response, feedback, split_by, q, alpha,
                          pos_alpha, v, z, err, n_st, n_sz, use_adaptive, simps_err, p_outlier,
                          w_outlier)


def wiener_like_rl_terms(response, feedback, split_by, q, alpha, pos_alpha, v, z, err=1e-4,
                         n_st=10, n_sz=10, use_adaptive=1, simps_err=1e-8, p_outlier=0,
                         w_outlier=0):
    """wiener_like_rl returning (sum, terms, drift), as wiener_like_rlddm_terms."""
    return _on_rl_dataset(RLDataset.wiener_like_rl, None, response, feedback, split_by, q, alpha,
                          pos_alpha, v, z, err, n_st, n_sz, use_adaptive, simps_err, p_outlier,
                          w_outlier, terms=True)


def wiener_like_multi_rlddm(x, response, feedback, split_by, q, v, sv, a, z, sz, t, st, alpha,
                            err, multi=None, n_st=10, n_sz=10, use_adaptive=1, simps_err=1e-3,
                            p_outlier=0, w_outlier=0):
    return _like_multi_rlddm(None, *_rl_host(x, response, feedback, split_by), q,
                             (v, sv, a, z, sz, t, st, alpha), err, multi, n_st, n_sz, use_adaptive,
                             simps_err, p_outlier, w_outlier, False)


def wiener_like_multi_rlddm_terms(x, response, feedback, split_by, q, v, sv, a, z, sz, t, st,
                                  alpha, err, multi, n_st=10, n_sz=10, use_adaptive=1,
                                  simps_err=1e-3, p_outlier=0, w_outlier=0):
    """wiener_like_multi_rlddm returning (sum, terms, drift); every trial is
    scored here, the first of a run at drift 0."""
    return _like_multi_rlddm(None, *_rl_host(x, response, feedback, split_by), q,
                             (v, sv, a, z, sz, t, st, alpha), err, multi, n_st, n_sz, use_adaptive,
                             simps_err, p_outlier, w_outlier, True)


def wiener_like_rlddm_nodes(ds, rl_rows, params, err=1e-4, n_st=2, n_sz=2, use_adaptive=1,
                            simps_err=1e-3, w_outlier=0.1, terms=False):
    """RLDataset.wiener_like_rlddm_nodes as a module function."""
    return ds.wiener_like_rlddm_nodes(rl_rows, params, err, n_st, n_sz, use_adaptive, simps_err,
                                      w_outlier, terms)


def wiener_like_rlddm_nodes_multi(ds, rl_tables, params, err=1e-4, n_st=2, n_sz=2, use_adaptive=1,
                                  simps_err=1e-3, w_outlier=0.1, terms=False):
    """RLDataset.wiener_like_rlddm_nodes_multi as a module function."""
    return ds.wiener_like_rlddm_nodes_multi(rl_tables, params, err, n_st, n_sz, use_adaptive,
                                            simps_err, w_outlier, terms)
