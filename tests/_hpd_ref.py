"""NumPy reference of the highest-density intervals (include/abcsmc_hip.h, abc_rank_targets_hpd_dev), built on _summary_ref.

One segment at a time.  The sorted entries u, the knots p and the quantile function Q are the summaries'.  For a mass m the
candidates are c = 2 r + kind:
    kind 0   plo = p_r,         phi = fl(p_r + m),  lo = u_r,     hi = Q(phi),  valid iff phi <= p_{n-1}
    kind 1   plo = fl(p_r - m), phi = p_r,          lo = Q(plo),  hi = u_r,     valid iff plo >= p_0
and the result is the valid candidate with the smallest (hi - lo, c); without a valid one it is [u_0, u_{n-1}] at (p_0, p_{n-1}).

hpd_literal walks the list as written, every Q through _summary_ref.quantile_sorted (float64: its final fma in exact rational
arithmetic).  hpd_segment gives the same answer faster: every candidate's width first in plain vectorised arithmetic, whose hi or
lo differs from the fma's by at most 3 roundings of max |u|, then the literal evaluation of the candidates within 32 roundings
of the smallest width alone; the test file checks the two against each other.  dtype=np.longdouble is the variant for the accuracy
bounds of unequal weights (no exactness claimed or needed there): it also returns the margin by which the winner beats the best
candidate at another position."""
import numpy as np

from _summary_ref import LD, knots, quantile_sorted, sorted_segment

NAN4 = (np.nan, np.nan, np.nan, np.nan)


def candidate(u, p, m, c, dtype=np.float64):
    """(lo, hi, plo, phi) of candidate c, or None when it is not valid"""
    n = u.size
    r, kind = c >> 1, c & 1
    m = dtype(m)
    if kind == 0:
        q = dtype(p[r] + m)
        if not q <= p[n - 1]:
            return None
        return float(u[r]), quantile_sorted(u, p, q, dtype), p[r], q
    q = dtype(p[r] - m)
    if not q >= p[0]:
        return None
    return quantile_sorted(u, p, q, dtype), float(u[r]), q, p[r]


def _degenerate(u, p):
    return float(u[0]), float(u[-1]), p[0], p[-1]


def hpd_literal(v, w, m):
    """(lo, hi, plo, phi, c) of one segment and one mass in float64, the candidate list walked as written; c = -1: no valid one"""
    v = np.asarray(v, dtype=np.float64)
    if not np.all(np.isfinite(v)):
        return NAN4 + (-1,)
    u, om = sorted_segment(v, w)
    if u.size == 0:
        return NAN4 + (-1,)
    p, _ = knots(om)
    best = None
    for c in range(2 * u.size):
        k = candidate(u, p, m, c)
        if k is not None and (best is None or (k[1] - k[0], c) < best[0]):
            best = ((k[1] - k[0], c), k)
    if best is None:
        return tuple(float(x) for x in _degenerate(u, p)) + (-1,)
    return tuple(float(x) for x in best[1]) + (best[0][1],)


def _q_fast(u, p, q):
    """Q at every q in the arithmetic of p's dtype: t * (u_{r+1} - u_r) + u_r in two roundings where the definition has one fma"""
    n = u.size
    if n == 1:
        return np.full(q.shape, u[0])
    r = np.clip(np.searchsorted(p, q, side="right") - 1, 0, n - 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (q - p[r]) / (p[r + 1] - p[r])
        val = t * (u[r + 1] - u[r]) + u[r]
    return np.where(q <= p[0], u[0], np.where(q >= p[n - 1], u[n - 1], val))


def _widths(u, p, m):
    """(width, valid, plo) of the 2 n candidates in c's order, in p's dtype"""
    n = u.size
    ud = u.astype(p.dtype)
    m = p.dtype.type(m)
    phi0, plo1 = p + m, p - m
    wd = np.empty(2 * n, dtype=p.dtype)
    wd[0::2] = _q_fast(ud, p, phi0) - ud
    wd[1::2] = ud - _q_fast(ud, p, plo1)
    valid = np.empty(2 * n, dtype=bool)
    valid[0::2] = phi0 <= p[n - 1]
    valid[1::2] = plo1 >= p[0]
    plo = np.empty(2 * n, dtype=p.dtype)
    plo[0::2] = p
    plo[1::2] = plo1
    return wd, valid, plo


def hpd_segment(v, w, masses, dtype=np.float64, position_tol=1e-9):
    """The intervals of one segment for every mass: arrays lo, hi, plo, phi (nm,) as float64 and, for dtype=np.longdouble, margin
    (nm,): (the smallest width among the valid candidates whose plo lies more than position_tol away from the winner's, minus the
    winner's width) relative to the winner's width; inf where there is no such candidate."""
    v = np.asarray(v, dtype=np.float64)
    nm = len(masses)
    out = np.full((4, nm), np.nan)
    margin = np.full(nm, np.inf)
    if not np.all(np.isfinite(v)):
        return (*out, margin) if dtype is LD else tuple(out)
    u, om = sorted_segment(v, w)
    if u.size == 0:
        return (*out, margin) if dtype is LD else tuple(out)
    p, _ = knots(om, dtype)
    p = np.asarray(p, dtype=dtype)
    tol = 32.0 * 2.0 ** -52 * float(np.max(np.abs(u)))
    for i, m in enumerate(masses):
        wd, valid, plo = _widths(u, p, m)
        if not valid.any():
            out[:, i] = [float(x) for x in _degenerate(u, p)]
            continue
        wv = np.where(valid, wd, np.inf)
        if dtype is LD:
            c = int(np.argmin(wv))                             # (the first of equal widths: the smallest c)
            out[:, i] = [float(x) for x in candidate(u, p, m, c, LD)]
            other = valid & (np.abs(plo - plo[c]) > position_tol)
            if other.any():
                w0 = float(wv[c])
                d = float(np.min(wv[other])) - w0
                margin[i] = d / w0 if w0 > 0 else (np.inf if d > 0 else 0.0)
            continue
        best = None
        for c in np.nonzero(valid & (wv <= wv.min() + tol))[0]:
            k = candidate(u, p, m, int(c))
            if k is not None and (best is None or (k[1] - k[0], int(c)) < best[0]):
                best = ((k[1] - k[0], int(c)), k)
        out[:, i] = [float(x) for x in best[1]]
    return (*out, margin) if dtype is LD else tuple(out)


def hpd(V, w, masses, dtype=np.float64):
    """The intervals of every column of V (K, P): arrays (nm, P) lo, hi, plo, phi (and margin for np.longdouble)"""
    V = np.asarray(V, dtype=np.float64)
    cols = [hpd_segment(V[:, j], w, masses, dtype) for j in range(V.shape[1])]
    return tuple(np.stack([c[k] for c in cols], axis=1) for k in range(len(cols[0])))


def coda_interval(x, m):
    """coda::HPDinterval's rule for one chain: the shortest [x_i, x_{i + gap}] of the sorted sample, gap = round(n m) kept within
    1 .. n - 1, the first of equal widths"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    gap = max(1, min(n - 1, int(round(n * m))))
    i = int(np.argmin(x[gap:] - x[:n - gap]))
    return x[i], x[i + gap]
