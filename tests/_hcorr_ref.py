"""NumPy reference of the heteroscedastic variance correction of the local-linear adjustment (include/abcsmc_hip.h,
abc_ctx_set_adjust_hcorr), for one slot.  Built on _loclinear_ref.loclinear: the first fit is that function's; the second fit
regresses z = 2 log|v - alpha| on the same covariates with the same weights, in np.longdouble, shifted by the first retained
row, with the same sweep; rule 5 (the skipped parameters) included."""
import numpy as np

import _loclinear_ref as R

LD = np.longdouble


def hcorr(dist, S_rows, o, theta_rows, kernel=0, A=None):
    """one slot: the arguments of _loclinear_ref.loclinear.  Returns that function's dict (the first fit, `theta` replaced by
    the corrected rows) plus plain (K, P) the uncorrected rows, hcoef ((A + 1), P) and skipped (P,) bool."""
    S_rows = np.asarray(S_rows, dtype=np.float64)
    theta_rows = np.asarray(theta_rows, dtype=np.float64)
    K, nc = S_rows.shape
    P = theta_rows.shape[1]
    A = nc if A is None else A
    fit = R.loclinear(dist, S_rows, o, theta_rows, kernel=kernel, A=A)
    v, alpha, w = fit["theta"], fit["coef"][0], fit["weight"]
    with np.errstate(all="ignore"):
        r = v - alpha[None, :]                                   # one fp64 subtraction with the stored alpha
        skipped = np.full(P, K <= nc + 2) | ~np.all(np.isfinite(r) & (r != 0.0), axis=0)
    ok = ~skipped
    hcoef = np.zeros((A + 1, P))
    hcoef[0, skipped] = np.nan
    out = v.copy()
    if ok.any():
        z = 2 * np.log(np.abs(r[:, ok].astype(LD)))
        x = S_rows - np.asarray(o, dtype=np.float64)[None, :]
        xs = (S_rows - S_rows[0]).astype(LD)
        zs = z - z[0]
        wl = w.astype(LD)
        W = wl.sum()
        xm = (wl[:, None] * xs).sum(axis=0) / W
        zm = (wl[:, None] * zs).sum(axis=0) / W
        xc, zc = xs - xm, zs - zm
        C = (wl[:, None] * xc).T @ xc
        c2 = (wl[:, None] * xc).T @ zc
        g, _ = R.sweep_solve(C, c2)
        xbar = xm + (S_rows[0] - o).astype(LD)
        a = (zm + z[0]) - g.T @ xbar
        hcoef[0, ok] = a.astype(np.float64)
        hcoef[1:1 + nc][:, ok] = g.astype(np.float64)
        g64 = g.astype(np.float64).astype(LD)
        q = x.astype(LD) @ g64
        out[:, ok] = (alpha[ok].astype(LD) + r[:, ok].astype(LD) * np.exp(-q / 2)).astype(np.float64)
    res = dict(fit)
    res.update(theta=out, plain=v, hcoef=hcoef, skipped=skipped)
    return res
