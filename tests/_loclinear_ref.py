"""NumPy reference of the local-linear regression adjustment (include/abcsmc_hip.h, abc_rank_targets_adjust_dev).

It works on one target from what the ranking returned (idx, dist) and the scores of the returned rows, rebuilt from the
fit's R, mean and sd.  Moments in np.longdouble, centred after a shift by the first retained row (as the device does, so that
rows equal to the first give exact zeros); the same sweep and skip rule as the device."""
import numpy as np

LD = np.longdouble


def z_scores(X, mean, sd):
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    safe = np.where(sd == 0, 1.0, sd)
    return np.where(sd == 0, 0.0, (X - mean) / safe)


def scores(X, mean, sd, R, nc):
    """scores of the rows of X on the first nc components: z-scores times R (longdouble, rounded to float64)"""
    z = z_scores(X, mean, sd).astype(LD)
    return (z @ np.asarray(R, dtype=np.float64)[:, :nc].astype(LD)).astype(np.float64)


def weights(dist, kernel=0):
    """(w, fallback): Epanechnikov 1 - (d/h)^2 with h = d[K - 1], rectangular when h == 0 or the weights sum to 0"""
    dist = np.asarray(dist, dtype=np.float64)
    K = dist.size
    if kernel == 1:
        return np.ones(K), False
    h = dist[-1]
    if h == 0.0:
        return np.ones(K), True
    t = dist / h
    w = 1.0 - t * t
    if w.sum() == 0.0:
        return np.ones(K), True
    return w, False


def sweep_solve(C, c):
    """beta = C^-1 c by the regression sweep in component order; pivot k is skipped when C_kk after the earlier sweeps is
    <= 1e-10 x the original C_kk, or the original C_kk <= 0.  Returns (beta, kept)."""
    nc = C.shape[0]
    Wk = np.concatenate([np.array(C, dtype=LD), np.array(c, dtype=LD)], axis=1)
    kept = np.zeros(nc, dtype=bool)
    for k in range(nc):
        d, c0 = Wk[k, k], C[k, k]
        if not (c0 > 0 and d > LD(1e-10) * c0):
            continue
        kept[k] = True
        rowk = Wk[k].copy() / d
        rowk[k] = 1 / d
        colk = Wk[:, k].copy()
        Wk -= np.outer(colk, rowk)
        Wk[k] = rowk
        Wk[:, k] = -colk / d
        Wk[k, k] = 1 / d
    beta = np.where(kept[:, None], Wk[:, nc:], LD(0))
    return beta, kept


def loclinear(dist, S_rows, o, theta_rows, kernel=0, A=None):
    """one target: dist (K,), S_rows (K, nc) the returned rows' scores, o (nc,) the observed scores, theta_rows (K, P).
    Returns dict(weight, coef ((A + 1), P), theta (K, P), rank, status) in float64."""
    S_rows = np.asarray(S_rows, dtype=np.float64)
    theta_rows = np.asarray(theta_rows, dtype=np.float64)
    K, nc = S_rows.shape
    P = theta_rows.shape[1]
    A = nc if A is None else A
    w, fallback = weights(dist, kernel)
    x = S_rows - np.asarray(o, dtype=np.float64)[None, :]
    xs = (S_rows - S_rows[0]).astype(LD)                 # shifted by the first retained row
    ts = (theta_rows - theta_rows[0]).astype(LD)
    wl = w.astype(LD)
    W = wl.sum()
    xm = (wl[:, None] * xs).sum(axis=0) / W
    tm = (wl[:, None] * ts).sum(axis=0) / W
    xc, tc = xs - xm, ts - tm
    C = (wl[:, None] * xc).T @ xc
    c = (wl[:, None] * xc).T @ tc
    beta, kept = sweep_solve(C, c)
    xbar = xm + (S_rows[0] - o).astype(LD)
    tbar = tm + theta_rows[0].astype(LD)
    alpha = tbar - beta.T @ xbar
    coef = np.zeros((A + 1, P))
    coef[0] = alpha.astype(np.float64)
    coef[1:1 + nc] = beta.astype(np.float64)
    th = (theta_rows.astype(LD) - x.astype(LD) @ beta).astype(np.float64)
    rank = int(kept.sum())
    status = (1 if rank < nc else 0) | (2 if fallback else 0)
    return dict(weight=w, coef=coef, theta=th, rank=rank, status=status)
