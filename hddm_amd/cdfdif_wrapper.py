"""Drop-in for the reference's `cdfdif_wrapper` extension module, on MI355X.

`hddm/__init__.py:11,19` imports it as `hddm.cdfdif`; its one function

    dmat_cdf_array(x, v, sv, a, z, sz, t, st, p_outlier, w_outlier)
                                              src/cdfdif_wrapper.pyx:16-53

returns the per-trial DMAT / Tuerlinckx (2004) CDF of signed RTs with the
outlier mixture: F(|x|, boundary) from cdfdif (src/cdfdif.c:59-221), folded as
(1 - P(upper)) + sign(x) * F, then y (1 - p_out) + (x + 1/(2 w_out)) w_out p_out.
Callers: the stochastic's `cdf` (hddm/likelihoods.py:90-91) and the quantile /
chi-square optimisers built on it (likelihoods.py:200-239, base.py:249-264).

`dmat_cdf_rows` is not in the reference: the same CDF for many rows of
(parameters, a few RTs, bin counts) in one launch, with each row's chi-square
and G-square, for the quantile optimisers (hddm_amd/optimize.py).

The series run in the HIP kernels of libwfpt_amd.so (cdfdif_kernels.hip);
argument checks and their exceptions are the reference's.
"""
import ctypes

import numpy as np

from . import _lib
from .wfpt import _check_x

__all__ = ["dmat_cdf_array", "dmat_cdf_rows"]

MAX_EDGES = 64    # include/wfpt_amd.h: wfpt_dmat_cdf_rows
ROWS_GRID = 2048  # its launch grid (wfpt_internal.h: kCdfRowsGrid); more rows stride over it


def dmat_cdf_rows(x, params, w_outlier, freq_obs=None, n_samples=None):
    """dmat_cdf_array for R rows in one launch, each with its own parameters.

    x (R, E): signed RTs of each row, ascending (the quantile edges of
    hddm_amd.quantiles.quantile_stats); params (R, 8): v, sv, a, z, sz, t, st,
    p_outlier per row. Returns cdf (R, E), row r bit for bit
    dmat_cdf_array(x[r], *params[r], w_outlier).

    With freq_obs (R, E + 1) and n_samples (R,) it returns (cdf, chisq, gsq),
    the reference's quantile statistics (likelihoods.py:200-239) per row:
    p = diff([0, cdf, 1]) with p <= 1e-6 replaced by 1e-6, chisq = the Pearson
    sum of (freq_obs - p n)^2 / (p n), gsq = 2 sum(freq_obs log p).

    A row outside the support (NaN included) does not raise: its chisq is
    +inf, its gsq -inf and its cdf NaN, what the reference's `except
    ValueError` branches return. The RT assertion and the zero w_outlier are
    dmat_cdf_array's, raised before any device work."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    P = np.ascontiguousarray(params, dtype=np.float64)
    if x.ndim != 2 or P.ndim != 2 or P.shape[1] != 8 or P.shape[0] != x.shape[0]:
        raise ValueError("dmat_cdf_rows: x must be (R, E) and params (R, 8)")
    R, E = x.shape
    if R < 1 or not 1 <= E <= MAX_EDGES:
        raise ValueError(f"dmat_cdf_rows: needs R >= 1 and 1 <= E <= {MAX_EDGES}, got R={R}, E={E}")
    if (freq_obs is None) != (n_samples is None):
        raise ValueError("dmat_cdf_rows: freq_obs and n_samples go together")
    if float(w_outlier) == 0.0:  # add_outlier_cdf (cdfdif_wrapper.pyx:11-12)
        raise ZeroDivisionError("float division")
    if np.any(P[:, 7] > 0):  # cdfdif_wrapper.pyx:20-21
        assert np.max(np.abs(x)) < (1. / (2 * w_outlier)), \
            ValueError('1. / (2*w_outlier) must be smaller than RT')
    if freq_obs is not None:
        f = np.ascontiguousarray(freq_obs, dtype=np.float64)
        n = np.ascontiguousarray(n_samples, dtype=np.float64)
        if f.shape != (R, E + 1) or n.shape != (R,):
            raise ValueError("dmat_cdf_rows: freq_obs must be (R, E + 1) and n_samples (R,)")
    c = _lib.context()
    cdf = np.empty((R, E), dtype=np.float64)
    rows = P.ctypes.data_as(ctypes.POINTER(_lib.Params))
    if freq_obs is None:
        _lib.check(_lib.wfpt_dmat_cdf_rows(c.handle, rows, _lib.dptr(x), None, None, R, E,
                                           float(w_outlier), _lib.dptr(cdf), None, None))
        return cdf
    chisq = np.empty(R, dtype=np.float64)
    gsq = np.empty(R, dtype=np.float64)
    _lib.check(_lib.wfpt_dmat_cdf_rows(c.handle, rows, _lib.dptr(x), _lib.dptr(f), _lib.dptr(n),
                                       R, E, float(w_outlier), _lib.dptr(cdf), _lib.dptr(chisq),
                                       _lib.dptr(gsq)))
    return cdf, chisq, gsq


def dmat_cdf_array(x, v, sv, a, z, sz, t, st, p_outlier, w_outlier):
    x = _check_x(x)
    # cdfdif_wrapper.pyx:20-21 (np.max of an empty array raises, as there)
    if p_outlier > 0:
        assert np.max(np.abs(x)) < (1. / (2 * w_outlier)), \
            ValueError('1. / (2*w_outlier) must be smaller than RT')
    # cdfdif_wrapper.pyx:23-25
    if (sv < 0) or (a <= 0) or (z < 0) or (z > 1) or (sz < 0) or (sz > 1) or \
            (z + sz / 2. > 1) or (z - sz / 2. < 0) or (t - st / 2. < 0) or (t < 0) or \
            (st < 0) or not ((p_outlier >= 0) & (p_outlier <= 1)):
        raise ValueError("at least one of the parameters is out of the support")
    n = x.shape[0]
    # add_outlier_cdf (cdfdif_wrapper.pyx:11-12) divides by 2*w_outlier in
    # Python semantics for every trial: a zero raises on the first one.
    if n > 0 and float(w_outlier) == 0.0:
        raise ZeroDivisionError("float division")
    out = np.empty(n, dtype=np.float64)
    if n == 0:
        return out
    c = _lib.context()
    P = _lib.make_params(v, sv, a, z, sz, t, st, p_outlier)
    _lib.check(_lib.wfpt_dmat_cdf_array(c.handle, _lib.dptr(x), n, ctypes.byref(P),
                                        float(w_outlier), _lib.dptr(out)))
    return out
