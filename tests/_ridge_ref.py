"""NumPy reference of the ridge adjustment with the penalty chosen by leave-one-out PRESS (include/abcsmc_hip.h,
abc_ctx_set_adjust_ridge), for one slot.  Built on _loclinear_ref: the same weights, the same shift by the first retained row,
the same moments in np.longdouble and the same sweep, here with the swept left block kept (M_l).  The residuals and leverages
of the PRESS use the float64 coefficients the device stores."""
import numpy as np

import _loclinear_ref as R

LD = np.longdouble


def sweep_full(C, c):
    """_loclinear_ref.sweep_solve, operation for operation, returning (beta, kept, M): M the swept left block, the inverse over
    the kept pivots with the rows and columns of skipped pivots zero"""
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
    M = np.where(kept[:, None] & kept[None, :], Wk[:, :nc], LD(0))
    return beta, kept, M


def moments(dist, S_rows, o, theta_rows, kernel=0):
    """the plain fit's pieces in longdouble: dict(w, fallback, x, xs, W, xm, xc, C, c, xbar, tbar)"""
    w, fallback = R.weights(dist, kernel)
    x = S_rows - np.asarray(o, dtype=np.float64)[None, :]
    xs = (S_rows - S_rows[0]).astype(LD)
    ts = (theta_rows - theta_rows[0]).astype(LD)
    wl = w.astype(LD)
    W = wl.sum()
    xm = (wl[:, None] * xs).sum(axis=0) / W
    tm = (wl[:, None] * ts).sum(axis=0) / W
    xc, tc = xs - xm, ts - tm
    C = (wl[:, None] * xc).T @ xc
    c = (wl[:, None] * xc).T @ tc
    xbar = xm + (S_rows[0] - o).astype(LD)
    tbar = tm + theta_rows[0].astype(LD)
    return dict(w=w, fallback=fallback, x=x, W=W, xc=xc, C=C, c=c, xbar=xbar, tbar=tbar)


def fits(m, lambdas):
    """per penalty (alpha (P,), beta (nc, P), M (nc, nc), kept) in longdouble from moments()"""
    out = []
    for lam in lambdas:
        Cl = m["C"].copy()
        dg = np.diag(m["C"])
        Cl[np.diag_indices_from(Cl)] = LD(lam) * dg + dg
        beta, kept, M = sweep_full(Cl, m["c"])
        out.append((m["tbar"] - beta.T @ m["xbar"], beta, M, kept))
    return out


def ridge(dist, S_rows, o, theta_rows, lambdas, kernel=0, A=None):
    """one slot: the arguments of _loclinear_ref.loclinear and the ascending penalties.  Returns that function's dict with coef
    and theta those of the picked fits (rank and status the unpenalised fit's) plus pick (P,), press (L, P) and gap (P,): the
    relative gap (second - best) / best between the two smallest PRESS values of a parameter (inf when fewer than two are
    finite)."""
    S_rows = np.asarray(S_rows, dtype=np.float64)
    theta_rows = np.asarray(theta_rows, dtype=np.float64)
    K, nc = S_rows.shape
    P = theta_rows.shape[1]
    A = nc if A is None else A
    L = len(lambdas)
    m = moments(dist, S_rows, o, theta_rows, kernel)
    w, x = m["w"], m["x"]
    wl, on = w.astype(LD), w > 0
    fl = fits(m, lambdas)
    press = np.full((L, P), np.inf)
    for l, (alpha, beta, M, _) in enumerate(fl):
        a64, b64 = alpha.astype(np.float64).astype(LD), beta.astype(np.float64).astype(LD)
        r = (theta_rows.astype(LD) - x.astype(LD) @ b64) - a64
        h = wl * (1 / m["W"] + np.einsum("ek,km,em->e", m["xc"], M, m["xc"]))
        den = 1 - h
        with np.errstate(all="ignore"):
            if np.any(on & ~(den > LD(1e-10))):
                continue
            p = (wl[on, None] * (r[on] / den[on, None]) ** 2).sum(axis=0).astype(np.float64)
        press[l] = np.where(np.isnan(p), np.inf, p)
    pick = np.where(np.isinf(press).all(axis=0), L - 1, np.argmin(press, axis=0)).astype(np.int32)
    srt = np.sort(press, axis=0)
    with np.errstate(all="ignore"):
        gap = np.where(np.isfinite(srt[1]), (srt[1] - srt[0]) / srt[0], np.inf) if L > 1 else np.full(P, np.inf)
    coef = np.zeros((A + 1, P))
    th = np.empty((K, P))
    for l in sorted(set(pick.tolist())):                         # (the rows as _loclinear_ref.loclinear makes them)
        alpha, beta, _, _ = fl[l]
        js = pick == l
        coef[0, js] = alpha.astype(np.float64)[js]
        coef[1:1 + nc][:, js] = beta.astype(np.float64)[:, js]
        th[:, js] = (theta_rows.astype(LD) - x.astype(LD) @ beta).astype(np.float64)[:, js]
    _, kept0, _ = sweep_full(m["C"], m["c"])
    rank = int(kept0.sum())
    status = (1 if rank < nc else 0) | (2 if m["fallback"] else 0)
    return dict(weight=w, coef=coef, theta=th, rank=rank, status=status, pick=pick, press=press, gap=gap)
