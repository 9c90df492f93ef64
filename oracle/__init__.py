"""ORACLE — TEST INFRASTRUCTURE ONLY.

ctypes bindings to oracle/wfpt_oracle.c, the plain-C CPU restatement of the
reference WFPT path (src/pdf.pxi, src/integrate.pxi, src/wfpt.pyx:32-76,244-274).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import
this package, and only as the checker or the timed CPU baseline. The product
package (hddm_amd) never imports it; it fails loudly without its HIP library.

Parity pins (tests/test_oracle.py): bit-exact vs oracle/_ref (the reference's
own kernels compiled by oracle/build_ref.py) on branch-covering vectors, and the
20 Navarro-Fuss MATLAB tuples of hddm/tests/matlab_values.py to 1e-9.

The DMAT CDF (oracle/cdfdif_oracle.c) also comes as a probe, `cdf_probe` (the
series cap as a parameter; per trial the branch, each series' stop index and
the scale S of the output), and in long double, `dmat_cdf_array_ld` (the same
source, summing the terms the double run summed): tests/test_cdfdif_tiers.py.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "liboracle_wfpt.so")
SRC = os.path.join(HERE, "wfpt_oracle.c")
SRC_CDF = os.path.join(HERE, "cdfdif_oracle.c")
SRC_CDF_LD = os.path.join(HERE, "cdfdif_oracle_ld.c")  # the same source in long double

_D = ctypes.c_double
_I = ctypes.c_int
_I64 = ctypes.c_int64
_PD = ctypes.POINTER(ctypes.c_double)

CDF_NSTOP = 43        # cd_record.stop slots (oracle/cdfdif_oracle.c)
CDF_SLOT_ZERO = 36    # zero-drift series of node m at 36 + m; (m, i) at m * 6 + i
CDF_SLOT_BEYOND = 42  # the series beyond the Ter window
CDF_VMAX = 5000       # the reference's series cap; as a stop index: never converged


class _CdfRecord(ctypes.Structure):
    _fields_ = [("branch", _I), ("stop", _I * CDF_NSTOP)]


class _CdfProbe(ctypes.Structure):
    _fields_ = [("S", _D), ("prob", _D), ("rec", _CdfRecord)]


def build(force=False):
    """gcc -O2 -ffp-contract=off (the reference's setup.py:4-7 uses -O2, no FMA)."""
    os.makedirs(LIBDIR, exist_ok=True)
    hdr = os.path.join(HERE, "wfpt_oracle.h")
    if (not force and os.path.exists(LIB)
            and all(os.path.getmtime(LIB) > os.path.getmtime(f)
                    for f in (SRC, SRC_CDF, SRC_CDF_LD, hdr))):
        return LIB
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC",
                    "-shared", "-o", LIB, SRC, SRC_CDF, SRC_CDF_LD, "-lm"], check=True)
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            build()
        L = ctypes.CDLL(LIB)
        L.oracle_ftt_01w.restype = _D
        L.oracle_ftt_01w.argtypes = [_D, _D, _D]
        L.oracle_prob_ub.restype = _D
        L.oracle_prob_ub.argtypes = [_D, _D, _D]
        L.oracle_pdf_sv.restype = _D
        L.oracle_pdf_sv.argtypes = [_D] * 6
        L.oracle_full_pdf.restype = _D
        L.oracle_full_pdf.argtypes = [_D] * 9 + [_I, _I, _I, _D, ctypes.POINTER(_I64)]
        L.oracle_wiener_like.restype = _D
        L.oracle_wiener_like.argtypes = [_PD, _I64] + [_D] * 8 + [_I, _I, _I, _D, _D, _D]
        L.oracle_pdf_array.restype = None
        L.oracle_pdf_array.argtypes = [_PD, _I64] + [_D] * 8 + [_I, _I, _I, _I, _D, _D, _D, _PD]
        L.oracle_pdf_array_omp.restype = _I
        L.oracle_pdf_array_omp.argtypes = [_PD, _I64] + [_D] * 8 + [_I, _I, _I, _I, _D, _D, _D,
                                                                    _PD, _I]
        L.oracle_wiener_like_multi.restype = _D
        L.oracle_wiener_like_multi.argtypes = [_PD, _I64, ctypes.POINTER(_PD), _PD, _D, _I, _I,
                                               _I, _D, _D, _D]
        L.oracle_count_evals.restype = _I64
        L.oracle_wiener_like_multi_terms.restype = _D
        L.oracle_wiener_like_multi_terms.argtypes = [_PD, _I64, ctypes.POINTER(_PD), _PD, _D, _I,
                                                     _I, _I, _D, _D, _D, _PD]
        L.oracle_count_evals.argtypes = [_PD, _I64] + [_D] * 8 + [_I, _I, _I, _D]
        L.oracle_dmat_cdf_array.restype = _I
        L.oracle_dmat_cdf_array.argtypes = [_PD, _I64] + [_D] * 9 + [_PD]
        L.oracle_dmat_cdf_array_omp.restype = _I
        L.oracle_dmat_cdf_array_omp.argtypes = [_PD, _I64] + [_D] * 9 + [_PD, _I]
        L.oracle_cdfdif_probe.restype = _D
        L.oracle_cdfdif_probe.argtypes = [_D, _I, _PD, _I, ctypes.POINTER(_CdfProbe)]
        L.oracle_cdfdif_replay.restype = _D
        L.oracle_cdfdif_replay.argtypes = [_D, _I, _PD, _I, ctypes.POINTER(_CdfProbe)]
        L.oracle_dmat_cdf_probe_array.restype = _I
        L.oracle_dmat_cdf_probe_array.argtypes = [_PD, _I64] + [_D] * 9 + [_I, _PD, _PD, _PD,
                                                                           ctypes.c_void_p]
        L.oracle_dmat_cdf_array_ld.restype = _I
        L.oracle_dmat_cdf_array_ld.argtypes = [_PD, _I64] + [_D] * 9 + [_I, ctypes.c_void_p,
                                                                        ctypes.c_void_p]
        _lib = L
    return _lib


def _arr(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return x, x.ctypes.data_as(_PD)


def ftt_01w(tt, w, err):
    return lib().oracle_ftt_01w(tt, w, err)


def prob_ub(v, a, z):
    return lib().oracle_prob_ub(v, a, z)


def pdf_sv(x, v, sv, a, z, err):
    return lib().oracle_pdf_sv(x, v, sv, a, z, err)


def full_pdf(x, v, sv, a, z, sz, t, st, err, n_st=2, n_sz=2, use_adaptive=1, simps_err=1e-3):
    return lib().oracle_full_pdf(x, v, sv, a, z, sz, t, st, err, n_st, n_sz, int(use_adaptive),
                                 simps_err, None)


def wiener_like(x, v, sv, a, z, sz, t, st, err, n_st=10, n_sz=10, use_adaptive=1,
                simps_err=1e-8, p_outlier=0, w_outlier=0.1):
    x, px = _arr(x)
    return lib().oracle_wiener_like(px, x.size, v, sv, a, z, sz, t, st, err, n_st, n_sz,
                                    int(use_adaptive), simps_err, p_outlier, w_outlier)


def pdf_array(x, v, sv, a, z, sz, t, st, err=1e-4, logp=0, n_st=2, n_sz=2, use_adaptive=1,
              simps_err=1e-3, p_outlier=0, w_outlier=0, n_threads=None):
    x, px = _arr(x)
    out = np.empty_like(x)
    if n_threads is None:
        # the reference applies np.log to the mixture array (wfpt.pyx:45-46); NumPy's log
        # differs from libm's by <= 1 ulp, so the log is taken here, in NumPy, too.
        lib().oracle_pdf_array(px, x.size, v, sv, a, z, sz, t, st, err, 0, n_st, n_sz,
                               int(use_adaptive), simps_err, p_outlier, w_outlier,
                               out.ctypes.data_as(_PD))
        if logp == 1:
            with np.errstate(divide="ignore", invalid="ignore"):
                out = np.log(out)
    else:
        lib().oracle_pdf_array_omp(px, x.size, v, sv, a, z, sz, t, st, err, int(logp), n_st,
                                   n_sz, int(use_adaptive), simps_err, p_outlier, w_outlier,
                                   out.ctypes.data_as(_PD), int(n_threads))
    return out


def wiener_like_multi(x, v, sv, a, z, sz, t, st, err, multi=None, n_st=10, n_sz=10,
                      use_adaptive=1, simps_err=1e-3, p_outlier=0, w_outlier=0, terms=False):
    """The reference's wiener_like_multi (wfpt.pyx:244-274); terms=True:
    (sum, per-trial terms)."""
    x, px = _arr(x)
    vals = [v, sv, a, z, sz, t, st]
    names = ["v", "sv", "a", "z", "sz", "t", "st"]
    multi = set(multi or ())
    keep = []
    ptrs = (_PD * 7)()
    scal = (_D * 7)()
    for j, (nm, val) in enumerate(zip(names, vals)):
        if nm in multi:
            arr, p = _arr(val)
            keep.append(arr)
            ptrs[j] = p
            scal[j] = 0.0
        else:
            ptrs[j] = _PD()
            scal[j] = float(val)
    out = np.empty(x.size) if terms else None
    tot = lib().oracle_wiener_like_multi_terms(px, x.size, ptrs, scal, err, n_st, n_sz,
                                               int(use_adaptive), simps_err, p_outlier,
                                               w_outlier,
                                               out.ctypes.data_as(_PD) if terms else None)
    return (tot, out) if terms else tot


def dmat_cdf_array(x, v, sv, a, z, sz, t, st, p_outlier, w_outlier, n_threads=None):
    """The reference's cdfdif_wrapper.dmat_cdf_array (cdfdif_wrapper.pyx:16-53
    over cdfdif.c:59-221) restated in C (oracle/cdfdif_oracle.c)."""
    x, px = _arr(x)
    out = np.empty_like(x)
    if n_threads is None:
        rc = lib().oracle_dmat_cdf_array(px, x.size, v, sv, a, z, sz, t, st, p_outlier,
                                         w_outlier, out.ctypes.data_as(_PD))
    else:
        rc = lib().oracle_dmat_cdf_array_omp(px, x.size, v, sv, a, z, sz, t, st, p_outlier,
                                             w_outlier, out.ctypes.data_as(_PD), int(n_threads))
    if rc < 0:
        raise ValueError("at least one of the parameters is out of the support")
    return out


class CdfProbe:
    """What oracle_dmat_cdf_probe_array returns for x[n]: `out` the wrapper's
    outputs, `F` cdfdif's values, `S` the scale of each output (the sum of the
    absolute values of every addend that enters it, after its multipliers),
    `branch` (0 below the Ter window, 1 beyond it, 2 inside it) and `stop`
    [n, 43]: the index of the last term each series added (window series
    (m, i) at m * 6 + i, zero-drift series of node m at 36 + m, the series
    beyond the window at 42; 5000 = never converged, -1 = did not run)."""

    def __init__(self, vcap, out, F, S, rec):
        self.vcap, self.out, self.F, self.S, self.rec = vcap, out, F, S, rec
        self.branch = rec["branch"]
        self.stop = rec["stop"]

    @property
    def longest(self):
        """The largest stop index of each trial (-1 where no series ran)."""
        return self.stop.max(axis=1)


_CDF_REC = np.dtype([("branch", np.int32), ("stop", np.int32, (CDF_NSTOP,))])
assert _CDF_REC.itemsize == ctypes.sizeof(_CdfRecord)


def cdf_probe(x, v, sv, a, z, sz, t, st, p_outlier, w_outlier, vcap=CDF_VMAX):
    """dmat_cdf_array with the series cap as a parameter (vcap = 5000: the
    reference, bit for bit), returning a CdfProbe."""
    x, px = _arr(x)
    out, F, S = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    rec = np.zeros(x.size, dtype=_CDF_REC)
    rc = lib().oracle_dmat_cdf_probe_array(px, x.size, v, sv, a, z, sz, t, st, p_outlier,
                                           w_outlier, int(vcap), out.ctypes.data_as(_PD),
                                           F.ctypes.data_as(_PD), S.ctypes.data_as(_PD),
                                           rec.ctypes.data)
    if rc < 0:
        raise ValueError("at least one of the parameters is out of the support")
    return CdfProbe(int(vcap), out, F, S, rec)


def dmat_cdf_array_ld(x, v, sv, a, z, sz, t, st, p_outlier, w_outlier, probe=None):
    """dmat_cdf_array in long double (x86-64 80-bit; np.longdouble): the same
    source, formulae and order, summing exactly the terms that the double run
    `probe` (default: cdf_probe at the reference's cap) summed, on its branch,
    with no convergence test of its own."""
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("np.longdouble is not the 80-bit extended format here")
    x, px = _arr(x)
    if probe is None:
        probe = cdf_probe(x, v, sv, a, z, sz, t, st, p_outlier, w_outlier)
    rec = np.ascontiguousarray(probe.rec)
    assert rec.size == x.size
    out = np.empty(x.size, dtype=np.longdouble)
    rc = lib().oracle_dmat_cdf_array_ld(px, x.size, v, sv, a, z, sz, t, st, p_outlier, w_outlier,
                                        probe.vcap, rec.ctypes.data, out.ctypes.data)
    if rc < 0:
        raise ValueError("at least one of the parameters is out of the support")
    return out


def cdfdif_probe(t, x, par, vcap=CDF_VMAX, replay=None):
    """One cdfdif(t, x, par) call through the probe: (F, S, prob, branch,
    stop[43]). replay = (branch, stop) sums those terms without testing."""
    par, pp = _arr(par)
    pr = _CdfProbe()
    if replay is None:
        F = lib().oracle_cdfdif_probe(float(t), int(x), pp, int(vcap), ctypes.byref(pr))
    else:
        pr.rec.branch = int(replay[0])
        for k, s in enumerate(replay[1]):
            pr.rec.stop[k] = int(s)
        F = lib().oracle_cdfdif_replay(float(t), int(x), pp, int(vcap), ctypes.byref(pr))
    return F, pr.S, pr.prob, pr.rec.branch, np.array(pr.rec.stop[:], dtype=np.int32)


def count_evals(x, v, sv, a, z, sz, t, st, err=1e-4, n_st=2, n_sz=2, use_adaptive=1,
                simps_err=1e-3):
    x, px = _arr(x)
    return lib().oracle_count_evals(px, x.size, v, sv, a, z, sz, t, st, err, n_st, n_sz,
                                    int(use_adaptive), simps_err)


def _load_ref_module(name):
    import importlib
    import sys
    d = os.path.join(HERE, "_ref")
    if not os.path.isdir(d):
        return None
    if d not in sys.path:
        sys.path.insert(0, d)
    try:
        return importlib.import_module(name)
    except ImportError:
        return None


def load_ref():
    """Import oracle/_ref/ref_shim (the reference's own kernels) or return None."""
    return _load_ref_module("ref_shim")


def load_ref_cdfdif():
    """Import oracle/_ref/cdfdif_wrapper (the reference's own cdfdif_wrapper
    extension, src/cdfdif_wrapper.pyx + src/cdfdif.c) or return None."""
    return _load_ref_module("cdfdif_wrapper")
