"""NumPy reference of the ABC-GLM posterior (include/abcsmc_hip.h, abc_glm_rank_targets_dev), one target at a time.

theta (K, P) the retained parameter rows, x (K, n) their scores (or any statistics), o (n,) the observed ones, w (K,) weights or
None; only the entries with w > 0 count, and a non-finite theta or x among them gives status 4 and NaN everywhere.  Every step
is the header's, in the dtype asked for (np.float64, or np.longdouble for the restatement the tests compare against); the
bandwidths are tests/_density_ref.py's unless given.  Status bits: 1 a Cholesky pivot of M_thth <= 1e-10 of its diagonal entry,
2 n_eff <= P + 1 or such a pivot of Sigma_s, 4 non-finite input."""
import numpy as np

import _density_ref as D

LD = np.longdouble
OUTPUTS = ("dens", "lo_x", "step", "mode", "mode_dens", "mean", "var", "ess", "log_md", "C", "c0", "sigma_s", "T", "peaks", "c")


def chol(A, rel):
    """(L, ok): the Cholesky factor in index order; ok is False when a pivot is <= rel times its own diagonal entry (or NaN)"""
    A = np.array(A)
    m = A.shape[0]
    L = np.zeros_like(A)
    ok = True
    for j in range(m):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > rel * A[j, j]:
            ok = False
        with np.errstate(invalid="ignore"):
            L[j, j] = np.sqrt(d)
        with np.errstate(invalid="ignore", divide="ignore"):
            for i in range(j + 1, m):
                L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L, ok


def solve_lower(L, B):
    """L^-1 B by forward substitution"""
    B = np.array(B)
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def solve_upper(U, B):
    B = np.array(B)
    X = np.zeros_like(B)
    for i in range(U.shape[0] - 1, -1, -1):
        X[i] = (B[i] - U[i, i + 1:] @ X[i + 1:]) / U[i, i]
    return X


def _nan_result(K, P, n, G, status):
    nan = np.nan
    r = dict(dens=np.full((P, G), nan), lo_x=np.full(P, nan), step=np.full(P, nan), mode=np.full(P, nan),
             mode_dens=np.full(P, nan), mean=np.full(P, nan), var=np.full(P, nan), ess=nan, log_md=nan, C=np.full((n, P), nan),
             c0=np.full(n, nan), sigma_s=np.full((n, n), nan), T=np.full((P, P), nan), peaks=np.full((K, P), nan),
             c=np.full(K, nan), status=status, bw=np.full(P, nan))
    return r


def bandwidths(theta, w=None, bw_scale=1.0):
    theta = np.asarray(theta, dtype=np.float64)
    return np.array([D.bandwidth(theta[:, j], w, bw_scale)[0] for j in range(theta.shape[1])])


def mixture_density(x, t, c, Tjj, dtype=LD):
    """f(x) = sum_e c_e N(x; t_e, Tjj) at the points x, in dtype"""
    x, t, c = np.asarray(x).astype(dtype), np.asarray(t).astype(dtype), np.asarray(c).astype(dtype)
    keep = c > 0
    t, c = t[keep], c[keep]
    Tjj = dtype(Tjj)
    out = np.empty(x.size, dtype=dtype)
    for lo in range(0, x.size, 64):
        z = x[lo:lo + 64, None] - t[None, :]
        out[lo:lo + 64] = (c[None, :] * np.exp(-(z * z) / (dtype(2) * Tjj))).sum(axis=1)
    return out / np.sqrt(dtype(8) * np.arctan(dtype(1)) * Tjj)


def glm(theta, x, o, w=None, G=64, cut=3.0, bw=None, bw_scale=1.0, dtype=np.float64):
    """dict of OUTPUTS plus status and bw (the bandwidths used); dens (P, G), peaks (K, P), c (K,) with 0 at the uncounted rows"""
    f = dtype
    theta = np.asarray(theta, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    o = np.asarray(o, dtype=np.float64).reshape(-1)
    K, P = theta.shape
    n = x.shape[1]
    wt = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    keep = wt > 0
    th, xs, om = theta[keep], x[keep], wt[keep]
    if not (np.all(np.isfinite(th)) and np.all(np.isfinite(xs))):
        return _nan_result(K, P, n, G, 4)
    thl, xl, oml = th.astype(f), xs.astype(f), om.astype(f)
    W = oml.sum()
    S2 = (oml * oml).sum()
    neff = W * W / S2
    thbar = (oml[:, None] * thl).sum(axis=0) / W
    xbar = (oml[:, None] * xl).sum(axis=0) / W
    tc, xc = thl - thbar, xl - xbar
    Mtt = (oml[:, None] * tc).T @ tc / W
    Mtx = (oml[:, None] * tc).T @ xc / W
    Mxx = (oml[:, None] * xc).T @ xc / W
    status = 0
    if not neff > P + 1:                                      # (first: without a counted row the moments are NaN)
        return _nan_result(K, P, n, G, 2)
    Lt, ok = chol(Mtt, f(1e-10))
    if not ok:
        return _nan_result(K, P, n, G, 1)
    Ct = solve_upper(Lt.T, solve_lower(Lt, Mtx))              # M_thth^-1 M_thx, P x n
    C = Ct.T
    c0 = xbar - C @ thbar
    R = Mxx - Mtx.T @ Ct
    R = (R + R.T) / f(2)
    Sig = R * (neff / (neff - f(P + 1)))
    Ls, ok = chol(Sig, f(1e-10))
    if not ok:
        return _nan_result(K, P, n, G, 2)
    h = np.asarray(bw, dtype=np.float64).reshape(-1) if bw is not None else bandwidths(th, om, bw_scale)
    hl = h.astype(f)
    tinv = f(1) / (hl * hl)
    Bm = solve_lower(Ls, C)                                   # Ls^-1 C
    yo = solve_lower(Ls, o.astype(f) - xbar)
    Q = Bm.T @ Bm + np.diag(tinv)
    Lq, _ = chol(Q, f(0))
    T = solve_upper(Lq.T, solve_lower(Lq, np.eye(P, dtype=f)))
    T = (T + T.T) / f(2)
    u = Bm.T @ yo
    v = u[None, :] + tc * tinv[None, :]
    Tv = v @ T
    t = thbar[None, :] + Tv
    logc = np.log(oml) - f(0.5) * ((tc * tc * tinv[None, :]).sum(axis=1) - (v * Tv).sum(axis=1))
    ch = np.exp(logc - logc.max())
    ch = ch / ch.sum()
    mean = (ch[:, None] * t).sum(axis=0)
    var = np.diag(T) + (ch[:, None] * (t - mean) ** 2).sum(axis=0)
    ess = f(1) / (ch * ch).sum()
    Smat = Sig + (C * (hl * hl)[None, :]) @ C.T
    LS, _ = chol(Smat, f(0))
    r = (o.astype(f) - xbar)[None, :] - tc @ C.T              # o - c0 - C theta_e
    y = solve_lower(LS, r.T)
    logn = np.log(oml) - f(0.5) * (y * y).sum(axis=0)
    m2 = logn.max()
    two_pi = f(8) * np.arctan(f(1))
    log_md = m2 + np.log(np.exp(logn - m2).sum()) - f(0.5) * (f(n) * np.log(two_pi) + f(2) * np.log(np.diag(LS)).sum()) - np.log(W)
    lo_x, step, dens, mode, mode_dens = np.empty(P), np.empty(P), np.empty((P, G), dtype=f), np.empty(P), np.empty(P, dtype=f)
    for j in range(P):
        sd = np.float64(np.sqrt(T[j, j]))
        tj = t[:, j].astype(np.float64)
        lo_x[j], step[j] = D.grid(tj.min(), tj.max(), sd, cut, G)
        xg = D.grid_points(lo_x[j], step[j], G)
        dens[j] = mixture_density(xg, t[:, j], ch, T[j, j], dtype=f)
        g = int(np.argmax(dens[j]))
        mode[j], mode_dens[j] = xg[g], dens[j, g]
    peaks = np.full((K, P), np.nan, dtype=f)
    peaks[keep] = t
    cfull = np.zeros(K, dtype=f)
    cfull[keep] = ch
    return dict(dens=dens, lo_x=lo_x, step=step, mode=mode, mode_dens=mode_dens, mean=mean, var=var, ess=ess, log_md=log_md, C=C,
                c0=c0, sigma_s=Sig, T=T, peaks=peaks, c=cfull, status=status, bw=h)
