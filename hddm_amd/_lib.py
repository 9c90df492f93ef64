"""ctypes binding to libwfpt_amd.so (include/wfpt_amd.h).

There is no CPU fallback: if the HIP library is missing this module raises
ImportError, and every device/driver failure raises RuntimeError with the
library's message (never a numeric stand-in).
"""
import ctypes
import os
import threading

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WFPT_AMD_LIB", os.path.join(_PKG, "lib", "libwfpt_amd.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"hddm_amd: HIP library not found at {LIB_PATH}; build it with "
        "`python -m hddm_amd.build` (hipcc --offload-arch=gfx950)")

# Kernel arguments in device memory: every wave of the likelihood kernels
# reads its ~150-byte argument block with scalar loads at start; from the
# default host-side kernarg pool those are PCIe round trips (measured on
# MI355X: 2.5% of the full-DDM kernel time). Read by the HIP runtime when it
# initialises, i.e. at the first call into the library; an explicit setting
# wins.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

_lib = ctypes.CDLL(LIB_PATH)

WFPT_OK = 0
WFPT_MAX_DEPTH = 24
WFPT_DS_INPUT_ORDER = 1
# WFPT_PATH_* (include/wfpt_amd.h): kernels the last likelihood call launched
PATH_LEAN, PATH_ENGINE, PATH_SMALL, PATH_REDO = 1, 2, 4, 8
PATH_FOLD, PATH_DIRECT, PATH_FIXED, PATH_SPLIT = 16, 32, 64, 128
PATH_SMALL_SPLIT, PATH_NODE_SPLIT, PATH_NODE_RARE = 256, 512, 1024
# regression links (include/wfpt_amd.h)
LINK_IDENTITY, LINK_EXP, LINK_INVLOGIT = 0, 1, 2

_D = ctypes.c_double
_I = ctypes.c_int
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64
_U64 = ctypes.c_uint64
_VP = ctypes.c_void_p
_CP = ctypes.c_char_p


class Params(ctypes.Structure):
    _fields_ = [(n, _D) for n in ("v", "sv", "a", "z", "sz", "t", "st", "p_outlier")]


class Knobs(ctypes.Structure):
    _fields_ = [("err", _D), ("n_st", _I32), ("n_sz", _I32), ("use_adaptive", _I32),
                ("simps_err", _D), ("w_outlier", _D)]


class RlSource(ctypes.Structure):
    """wfpt_rl_source: the closed-loop simulator's reward source (addresses)."""
    _fields_ = [(n, _VP) for n in ("p", "rew_up", "rew_low", "obs_response", "obs_feedback",
                                   "start")] + [("n", _I64)]


class RegTerm(ctypes.Structure):
    _fields_ = [(n, _I32) for n in ("param", "link", "col0", "ncol")]


_PD = ctypes.POINTER(_D)
_PPD = ctypes.POINTER(_PD)
_PI = ctypes.POINTER(_I)
_PI32 = ctypes.POINTER(_I32)
_PI64 = ctypes.POINTER(_I64)
_PU64 = ctypes.POINTER(_U64)
_PVP = ctypes.POINTER(_VP)
_PP = ctypes.POINTER(Params)
_PK = ctypes.POINTER(Knobs)
_PT = ctypes.POINTER(RegTerm)
_PS = ctypes.POINTER(RlSource)

# Every entry point of include/wfpt_amd.h: name -> (restype, argtypes). Each
# becomes a module attribute below, and EXPORTED is this table's names.
_LIKE = [_VP, _VP, _PP, _PK, _PD]  # ctx, dataset, params | table, knobs, out
_MULTI = [_PPD, _PD, _PK, _D, _PD]  # per-trial arrays, scalars, knobs, p_outlier, out
_RL_HOST = [_VP, _PD, _PI64, _PD, _PI64, _I64, _D]  # ctx, rt, response, feedback, split_by, n, q
_REG = [_VP, _VP, _PT, _I32, _PD, _PP, _PK, _PD]  # ctx, ds, terms, n_terms, coef, params, ...
_RL_REG = [_VP, _VP, _PT, _I32, _PD, _PD, _PD, _PP, _PK, _PD]
_GEN_CDF = [_VP, _PD, _I64, _PP, _I64, _PI64, _PD, _PD, _U64, _I64, _PD]
_GEN_DRIFT = [_VP, _PP, _I64, _PD, _PI64, _D, _D, _I64, _U64]
_GEN_RLDDM = [_VP, _PP, _PD, _I64, _PI64, _PS, _D, _D, _I64, _U64]
# ctx, ds, terms, n_terms, coef, params, S, dt, intra_sv, max_steps, seed
_GEN_REG = [_VP, _VP, _PT, _I32, _PD, _PP, _I64, _D, _D, _I64, _U64]
_SIGNATURES = {
    "wfpt_last_error": (_CP, []),
    "wfpt_device_count": (_I, [_PI]),
    "wfpt_open": (_I, [_I, _PVP]),
    "wfpt_close": (None, [_VP]),
    "wfpt_synchronize": (_I, [_VP]),
    "wfpt_shard_range": (None, [_I64, _I, _I, _PI64, _PI64]),
    # resident data sets and their likelihoods
    "wfpt_dataset_create": (_I, [_VP, _PD, _I64, _PI32, _I32, _PVP]),
    "wfpt_dataset_create_ex": (_I, [_VP, _PD, _I64, _PI32, _I32, _I, _PVP]),
    "wfpt_dataset_destroy": (None, [_VP]),
    "wfpt_dataset_size": (_I64, [_VP]),
    "wfpt_dataset_order": (_I, [_VP, _PI64]),
    "wfpt_wiener_like": (_I, _LIKE),
    "wfpt_wiener_like_trials": (_I, _LIKE + [_PD]),
    "wfpt_wiener_like_local": (_I, _LIKE),
    "wfpt_wiener_like_nodes": (_I, _LIKE),
    "wfpt_wiener_like_nodes_ex": (_I, _LIKE + [_PD]),
    "wfpt_wiener_like_nodes_local": (_I, _LIKE),
    "wfpt_wiener_like_nodes_multi": (_I, [_VP, _VP, _PP, _I32, _PK, _PD]),
    "wfpt_wiener_like_nodes_multi_ex": (_I, [_VP, _VP, _PP, _I32, _PK, _PD, _PD]),
    "wfpt_wiener_like_multi_resident": (_I, [_VP, _VP] + _MULTI),
    "wfpt_wiener_like_multi_resident_ex": (_I, [_VP, _VP] + _MULTI + [_PD]),
    # host arrays
    "wfpt_wiener_like_host": (_I, [_VP, _PD, _I64, _PP, _PK, _PD]),
    "wfpt_pdf_array": (_I, [_VP, _PD, _I64, _PP, _PK, _I, _PD]),
    "wfpt_full_pdf": (_I, [_VP, _D, _PP, _PK, _PD]),
    "wfpt_wiener_like_multi": (_I, [_VP, _PD, _I64] + _MULTI),
    "wfpt_wiener_like_multi_ex": (_I, [_VP, _PD, _I64] + _MULTI + [_PD]),
    "wfpt_dmat_cdf_array": (_I, [_VP, _PD, _I64, _PP, _D, _PD]),
    "wfpt_dmat_cdf_rows": (_I, [_VP, _PP, _PD, _PD, _PD, _I64, _I32, _D, _PD, _PD, _PD]),
    # multi-GPU
    "wfpt_comm_unique_id": (_I, [_CP]),
    "wfpt_comm_init": (_I, [_VP, _I, _I, _CP]),
    "wfpt_comm_exchange_id": (_I, [_I, _I, _CP, _I, _I, _CP]),
    "wfpt_comm_init_tcp": (_I, [_VP, _I, _I, _CP, _I, _I]),
    "wfpt_comm_init_all": (_I, [_PVP, _I]),
    "wfpt_wiener_like_allreduce": (_I, _LIKE),
    "wfpt_wiener_like_allreduce_group": (_I, [_PVP, _PVP, _I, _PP, _PK, _PD]),
    "wfpt_wiener_like_nodes_allreduce": (_I, [_VP, _VP, _PP, _I32, _PK, _PD]),
    "wfpt_result_poison": (_I, [_PD]),
    "wfpt_decode_result": (_I, [_PD, _PD]),
    # diagnostics
    "wfpt_profile_enable": (_I, [_VP, _I]),
    "wfpt_profile_read": (_I, [_VP, _PD, _PI64, _PI64, _I]),
    "wfpt_profile_stages": (_I, [_VP, _PD, _I]),
    "wfpt_profile_lists": (_I, [_VP, _PI64, _I]),
    "wfpt_debug_waves": (_I, [_VP, _PU64, _I64]),
    "wfpt_debug_partials": (_I, [_VP, _PD, _PI32, _I64]),
    "wfpt_debug_lean_first": (_I, [_VP, _PI32, _I32, _PI32]),
    "wfpt_last_path": (_I, [_VP, _PI]),
    # reinforcement-learning family
    "wfpt_rl_dataset_create": (_I, [_VP, _PD, _PI64, _PD, _PI64, _I64, _PI32, _I32, _PVP]),
    "wfpt_rl_dataset_destroy": (None, [_VP]),
    "wfpt_wiener_like_rlddm": (_I, [_VP, _VP, _D, _D, _D, _PP, _PK, _PD]),
    "wfpt_wiener_like_rlddm_ex": (_I, [_VP, _VP, _D, _D, _D, _PP, _PK, _PD, _PD, _PD]),
    "wfpt_wiener_like_rl": (_I, [_VP, _VP] + [_D] * 7 + [_PD]),
    "wfpt_wiener_like_rl_ex": (_I, [_VP, _VP] + [_D] * 7 + [_PD, _PD, _PD]),
    "wfpt_wiener_like_multi_rlddm": (_I, _RL_HOST + _MULTI),
    "wfpt_wiener_like_multi_rlddm_ex": (_I, _RL_HOST + _MULTI + [_PD, _PD]),
    "wfpt_wiener_like_rlddm_nodes": (_I, [_VP, _VP, _PD, _PP, _PK, _PD]),
    "wfpt_wiener_like_rlddm_nodes_ex": (_I, [_VP, _VP, _PD, _PP, _PK, _PD, _PD, _PD]),
    "wfpt_wiener_like_rlddm_nodes_multi": (_I, [_VP, _VP, _PD, _PP, _I32, _PK, _PD]),
    "wfpt_wiener_like_rlddm_nodes_multi_ex": (_I, [_VP, _VP, _PD, _PP, _I32, _PK, _PD, _PD, _PD]),
    # regression likelihoods
    "wfpt_reg_dataset_create": (_I, [_VP, _PD, _I64, _PD, _I32, _PI32, _I32, _PVP]),
    "wfpt_reg_dataset_destroy": (None, [_VP]),
    "wfpt_wiener_like_reg": (_I, _REG),
    "wfpt_wiener_like_reg_ex": (_I, _REG + [_PD, _PD]),
    "wfpt_wiener_like_reg_groups": (_I, _REG),
    "wfpt_wiener_like_reg_groups_ex": (_I, _REG + [_PD, _PD]),
    # RL regression likelihood: ctx, ds, terms, n_terms, coef, q, alpha, params, knobs, out
    "wfpt_rl_reg_dataset_create": (_I, [_VP, _PD, _PI64, _PD, _PI64, _I64, _PD, _I32, _PI32, _I32,
                                        _PVP]),
    "wfpt_rl_reg_dataset_destroy": (None, [_VP]),
    "wfpt_wiener_like_rl_reg_groups": (_I, _RL_REG),
    "wfpt_wiener_like_rl_reg_groups_ex": (_I, _RL_REG + [_PD, _PD, _PD, _PD]),
    "wfpt_gen_rts_reg_drift": (_I, _GEN_REG + [_PD, _PI64, _PI64]),
    "wfpt_gen_rts_reg_drift_ex": (_I, _GEN_REG + [_I32, _I64, _PD, _PI64, _PI64, _PD, _PD, _PD,
                                                  _PD, _PI64, _PI64]),
    "wfpt_gen_rts_reg_drift_stats": (_I, _GEN_REG + [_I64, _PD, _PI64, _PI64, _PD, _I32, _PD]),
    # RT samplers and per-row RT statistics
    "wfpt_gen_rts_nodes": (_I, _GEN_CDF),
    "wfpt_gen_rts_nodes_ex": (_I, _GEN_CDF + [_PD, _PD, _PI64, _PD, _PD]),
    "wfpt_gen_rts_nodes_stats": (_I, _GEN_CDF + [_PD, _I32, _PD]),
    "wfpt_gen_rts_drift_nodes": (_I, _GEN_DRIFT + [_PD, _PI64]),
    "wfpt_gen_rts_drift_nodes_ex": (_I, _GEN_DRIFT + [_I64, _I32, _PD, _PI64, _PD, _PD, _PD, _PD,
                                                      _PI64, _PI64]),
    "wfpt_gen_rts_drift_nodes_stats": (_I, _GEN_DRIFT + [_PD, _PI64, _PD, _I32, _PD]),
    "wfpt_gen_rlddm_rows": (_I, _GEN_RLDDM + [_PD, _PI64]),
    "wfpt_gen_rlddm_rows_ex": (_I, _GEN_RLDDM + [_I64, _I32, _PD, _PI64] + [_PD] * 7
                               + [_PI64, _PI64]),
    "wfpt_gen_rlddm_rows_stats": (_I, _GEN_RLDDM + [_PD, _PI64, _PI64, _I64, _PD, _I32, _PD]),
    "wfpt_rt_stats_rows": (_I, [_VP, _PD, _PI64, _I64, _PD, _I32, _PD]),
    "wfpt_rt_stats_rows_ex": (_I, [_VP, _PD, _PI64, _I64, _PD, _I32, _I32, _PD]),
    # model comparison: per-sweep sums + per-trial statistics over S sweeps
    "wfpt_pointwise_nodes": (_I, [_VP, _VP, _PP, _I64, _PK, _I64, _PD, _PD, _PI64]),
    "wfpt_pointwise_rlddm_nodes": (_I, [_VP, _VP, _PD, _PP, _I64, _PK, _I64, _PD, _PD, _PI64,
                                        _PI64]),
    "wfpt_pointwise_reg_groups": (_I, [_VP, _VP, _PT, _I32, _PD, _PP, _I64, _PK, _I64, _PD, _PD,
                                       _PI64]),
    "wfpt_pointwise_profile": (_I, [_VP, _PD, _I]),
}
# diagnostics only: A/B runs may load an older library build without them
_OPTIONAL = ("wfpt_profile_lists", "wfpt_debug_waves")
EXPORTED = list(_SIGNATURES)


def _sig(name, res, args):
    f = getattr(_lib, name, None) if name in _OPTIONAL else getattr(_lib, name)
    if f is not None:
        f.restype = res
        f.argtypes = args
    return f


globals().update({name: _sig(name, *sig) for name, sig in _SIGNATURES.items()})


def _raw(name, nargs, i32=()):
    """The same entry point through a prototype of plain addresses (ints): the
    per-call paths (one likelihood per MCMC step) skip the per-argument ctypes
    object conversions (~1 us per call through byref / data_as). The argument
    positions in `i32` are int32 values, not addresses."""
    proto = ctypes.CFUNCTYPE(_I, *[_I32 if j in i32 else _VP for j in range(nargs)])
    return proto(ctypes.cast(getattr(_lib, name), _VP).value)


raw_wiener_like = _raw("wfpt_wiener_like", 5)
raw_wiener_like_nodes = _raw("wfpt_wiener_like_nodes", 5)
raw_wiener_like_nodes_multi = _raw("wfpt_wiener_like_nodes_multi", 6, i32=(3,))

# error encoding of a result triple (include/wfpt_amd.h: wfpt_decode_result)
DEPTH_ERROR = 1.0
BUDGET_ERROR = 1048576.0
PEER_FAILED = 1099511627776.0  # 2^40: a rank that failed before the exchange


def poisoned_result():
    """The triple a rank that failed before the exchange contributes
    (wfpt_result_poison)."""
    r = (ctypes.c_double * 3)()
    check(wfpt_result_poison(r))
    return [r[0], r[1], r[2]]


def decode_result(triple):
    """The library's decode of a (rank-summed) {sum, zeros, errors} triple."""
    r = (ctypes.c_double * 3)(*[float(v) for v in triple])
    out = _D()
    check(wfpt_decode_result(r, ctypes.byref(out)))
    return out.value


class CommError(RuntimeError):
    """A multi-GPU exchange failed (WFPT_ERR_COMM), e.g. another rank's local
    pass failed before the all-reduce."""


def check(rc):
    if rc != WFPT_OK:
        msg = wfpt_last_error().decode(errors="replace")
        if rc == 4:
            raise NotImplementedError(f"wfpt_amd: {msg}")
        if rc == 2:
            raise ValueError(f"wfpt_amd: {msg}")
        if rc == 3:
            raise CommError(f"wfpt_amd error {rc}: {msg}")
        raise RuntimeError(f"wfpt_amd error {rc}: {msg}")


def dptr(a):
    return a.ctypes.data_as(_PD)


class Context:
    """One HIP device + stream + workspaces (wfpt_ctx)."""

    def __init__(self, device=0):
        h = _VP()
        check(wfpt_open(int(device), ctypes.byref(h)))
        self.handle = h
        self.device = int(device)

    def close(self):
        if self.handle:
            wfpt_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    PROF_EVENTS = 1
    PROF_EVALS = 2

    def profile(self, flags=1):
        """flags: PROF_EVENTS (per-launch HIP-event time) | PROF_EVALS (count pdf_sv evals)."""
        check(wfpt_profile_enable(self.handle, int(flags)))

    def profile_read(self, reset=False):
        ms, nl, ne = _D(), _I64(), _I64()
        check(wfpt_profile_read(self.handle, ctypes.byref(ms), ctypes.byref(nl),
                                ctypes.byref(ne), 1 if reset else 0))
        return ms.value, nl.value, ne.value

    def profile_stages(self, reset=False):
        """Device ms of the RT sampler's stages since the last reset
        (wfpt_profile_stages): density, scan, normalise, draws."""
        a = (_D * 4)()
        check(wfpt_profile_stages(self.handle, a, 1 if reset else 0))
        return dict(zip(("density", "scan", "normalise", "draws"), a))

    def pointwise_profile(self, reset=False):
        """Device ms of the model-comparison pass's accumulate kernel since the
        last reset (wfpt_pointwise_profile; profiled passes only)."""
        ms = _D()
        check(wfpt_pointwise_profile(self.handle, ctypes.byref(ms), 1 if reset else 0))
        return ms.value

    def profile_lists(self, reset=False):
        """Deferred-pass list sizes (include/wfpt_amd.h: wfpt_profile_lists)."""
        a = (_I64 * 16)()
        if wfpt_profile_lists is None:
            return {}
        check(wfpt_profile_lists(self.handle, a, 1 if reset else 0))
        v = list(a)
        return {"segments": v[0], "lean_table": v[0], "node_deferred": v[3], "lean_generic": v[3],
                "tasks1": v[1], "tasks2": v[2], "records": v[4], "exact": v[5],
                "walk": v[6], "zwalks": v[7], "zwalks0": v[8], "zwalks1": v[9],
                "zwalks2": v[10], "phase_kcycles": v[11:16]}

    def debug_waves(self, n):
        """Per-wave engine records of diagnostic builds (wfpt_debug_waves): (n, 8) uint64."""
        out = np.zeros((n, 8), dtype=np.uint64)
        check(wfpt_debug_waves(self.handle, out.ctypes.data_as(_PU64), n))
        return out

    def synchronize(self):
        check(wfpt_synchronize(self.handle))

    def last_path(self):
        """WFPT_PATH_* bits of the kernels the last likelihood call launched."""
        v = _I()
        check(wfpt_last_path(self.handle, ctypes.byref(v)))
        return v.value

    def lean_first(self):
        """The chunks the last call's lean pass dispatched first (wfpt_debug_lean_first)."""
        out = np.zeros(64, dtype=np.int32)
        n = _I32()
        check(wfpt_debug_lean_first(self.handle, out.ctypes.data_as(_PI32), 64, ctypes.byref(n)))
        return [int(v) for v in out[:n.value]]

    def partials(self, n):
        """The first n chunk partials {sum, zero word} of the last summing call."""
        part = np.empty(n, dtype=np.float64)
        zero = np.empty(n, dtype=np.int32)
        check(wfpt_debug_partials(self.handle, dptr(part), zero.ctypes.data_as(_PI32), n))
        return part, zero


_ctx_lock = threading.Lock()
_contexts = {}


def default_device():
    env = os.environ.get("WFPT_DEVICE")
    if env is not None:
        return int(env)
    return 0


def context(device=None):
    """Process-wide context for `device` (default: $WFPT_DEVICE or 0)."""
    dev = default_device() if device is None else int(device)
    with _ctx_lock:
        c = _contexts.get(dev)
        if c is None:
            c = Context(dev)
            _contexts[dev] = c
        return c


def device_count():
    n = _I()
    check(wfpt_device_count(ctypes.byref(n)))
    return n.value


def shard_range(n, nranks, rank):
    lo, hi = _I64(), _I64()
    wfpt_shard_range(int(n), int(nranks), int(rank), ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def make_params(v, sv, a, z, sz, t, st, p_outlier=0.0):
    return Params(float(v), float(sv), float(a), float(z), float(sz), float(t), float(st),
                  float(p_outlier))


def make_knobs(err, n_st, n_sz, use_adaptive, simps_err, w_outlier):
    return Knobs(float(err), int(n_st), int(n_sz), 1 if use_adaptive else 0, float(simps_err),
                 float(w_outlier))
