"""NumPy reference of the row importance weights of the batched ranking (include/abcsmc_hip.h, abc_ctx_set_row_weights), for
one target.  Entry e weighs w_e = k_e * omega[i_e]; the existing references (_loclinear_ref.loclinear, _ridge_ref.ridge,
_hcorr_ref.hcorr, _path_ref.path) all take their weights from _loclinear_ref.weights, so wrapping that one function makes them
the weighted definitions without editing them.  This module adds the all-zero rule and the weighted rejection mean in
np.longdouble."""
import contextlib

import numpy as np

import _hcorr_ref as H
import _loclinear_ref as R
import _path_ref as PT
import _ridge_ref as G

LD = np.longdouble


@contextlib.contextmanager
def row_weighted(omega_rows):
    """inside the block _loclinear_ref.weights(dist, kernel) returns (w * omega_rows[:K], fallback), K = len(dist): omega_rows are
    the row weights of the retained rows in ranking order (omega[idx]); the fallback rule still reads the distances only"""
    om = np.asarray(omega_rows, dtype=np.float64)
    real = R.weights

    def weights(dist, kernel=0):
        w, fallback = real(dist, kernel)
        return w * om[:w.size], fallback
    R.weights = weights
    try:
        yield
    finally:
        R.weights = real


def weights(dist, omega_rows, kernel=0):
    """(k_e * omega_e, fallback)"""
    with row_weighted(omega_rows):
        return R.weights(dist, kernel)


def _all_zero(dist, S_rows, theta_rows, omega_rows, kernel, A):
    """the all-zero rule's outputs, or None when some retained row has a positive weight"""
    w, fallback = weights(dist, omega_rows, kernel)
    if np.any(w > 0):
        return None
    K, nc = np.asarray(S_rows).shape
    P = np.asarray(theta_rows).shape[1]
    A = nc if A is None else A
    coef = np.zeros((A + 1, P))
    coef[:1 + nc] = np.nan
    status = 4 | (1 if nc > 0 else 0) | (2 if fallback else 0)
    return dict(weight=w, coef=coef, theta=np.full((K, P), np.nan), rank=0, status=status)


def loclinear(dist, S_rows, o, theta_rows, omega_rows, kernel=0, A=None):
    z = _all_zero(dist, S_rows, theta_rows, omega_rows, kernel, A)
    if z is not None:
        return z
    with row_weighted(omega_rows):
        return R.loclinear(dist, S_rows, o, theta_rows, kernel=kernel, A=A)


def ridge(dist, S_rows, o, theta_rows, omega_rows, lambdas, kernel=0, A=None):
    z = _all_zero(dist, S_rows, theta_rows, omega_rows, kernel, A)
    if z is not None:                                           # every (slot, parameter) unscored
        P, L = z["coef"].shape[1], len(lambdas)
        z.update(pick=np.full(P, L - 1, dtype=np.int32), press=np.full((L, P), np.inf), gap=np.full(P, np.inf))
        return z
    with row_weighted(omega_rows):
        return G.ridge(dist, S_rows, o, theta_rows, lambdas, kernel=kernel, A=A)


def hcorr(dist, S_rows, o, theta_rows, omega_rows, kernel=0, A=None, lambdas=None):
    """lambdas: the composed definition, the second fit on the residuals of the ridge fit"""
    z = _all_zero(dist, S_rows, theta_rows, omega_rows, kernel, A)
    if z is not None:                                           # every parameter skipped: the record of a skipped parameter
        hcoef = np.zeros_like(z["coef"])
        hcoef[0] = np.nan
        z.update(plain=z["theta"], hcoef=hcoef, skipped=np.ones(hcoef.shape[1], dtype=bool))
        return z
    with row_weighted(omega_rows):
        if lambdas is None:
            return H.hcorr(dist, S_rows, o, theta_rows, kernel=kernel, A=A)
        real = R.loclinear
        R.loclinear = lambda d, S_, o_, th, kernel=0, A=None: G.ridge(d, S_, o_, th, lambdas, kernel=kernel, A=A)
        try:
            return H.hcorr(dist, S_rows, o, theta_rows, kernel=kernel, A=A)
        finally:
            R.loclinear = real


def post_mean(theta_rows, omega_rows):
    """sum omega_e theta_e / sum omega_e in np.longdouble (NaN when every omega_e is 0)"""
    om = np.asarray(omega_rows, dtype=np.float64).astype(LD)
    th = np.asarray(theta_rows, dtype=np.float64).astype(LD)
    with np.errstate(all="ignore"):
        return (om[:, None] * th).sum(axis=0) / om.sum()


def path(dist, S_rows, o, theta_rows, omega_rows, Ks, kernel=0, A=None):
    """_path_ref.path's dict under the row weights: tolerance t is loclinear() above on the first K_t rows, post_mean the weighted
    mean of those rows"""
    dist = np.asarray(dist, dtype=np.float64)
    om = np.asarray(omega_rows, dtype=np.float64)
    Ks = [int(k) for k in Ks]
    assert Ks[0] >= 1 and all(a < b for a, b in zip(Ks, Ks[1:])) and Ks[-1] == dist.size
    if all(np.any(weights(dist[:K], om[:K], kernel)[0] > 0) for K in Ks):
        with row_weighted(om):
            r = PT.path(dist, S_rows, o, theta_rows, Ks, kernel=kernel, A=A)
    else:
        fits = [loclinear(dist[:K], S_rows[:K], o, theta_rows[:K], om[:K], kernel=kernel, A=A) for K in Ks]
        r = dict(coef=np.array([f["coef"] for f in fits]), rank=np.array([f["rank"] for f in fits], dtype=np.int32),
                 status=np.array([f["status"] for f in fits], dtype=np.int32), h=np.array([dist[K - 1] for K in Ks]))
    r["post_mean"] = np.array([post_mean(theta_rows[:K], om[:K]) for K in Ks])
    return r
