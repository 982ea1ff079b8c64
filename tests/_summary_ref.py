"""NumPy reference of the weighted posterior quantiles and CDF (include/abcsmc_hip.h, abc_rank_targets_summary_dev).

One segment at a time: values v and weights w in the ranking's order.  The entries with w > 0 sorted by the IEEE totalOrder
of the value, ties by position; W_r left to right (float64, or np.longdouble for the accuracy bounds of unequal weights);
knots p_r = fma(-0.5, om_r, W_r) / W; the final fma of a quantile in exact rational arithmetic (fractions.Fraction)."""
from fractions import Fraction

import numpy as np

LD = np.longdouble


def total_order_key(v):
    b = np.asarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def sorted_segment(v, w=None):
    """(u, om): the entries with positive weight in the definition's order"""
    v = np.asarray(v, dtype=np.float64)
    w = np.ones(v.size) if w is None else np.asarray(w, dtype=np.float64)
    e = np.nonzero(w > 0)[0]
    o = e[np.lexsort((e, total_order_key(v[e])))]
    return v[o], w[o]


def _fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def knots(om, dtype=np.float64):
    """(p, W): p_r = fma(-0.5, om_r, W_r) / W with W_r summed left to right in dtype (0.5 om is exact, so the fma is one
    subtraction)"""
    om = np.asarray(om).astype(dtype)
    Wr = np.cumsum(om, dtype=dtype)
    W = Wr[-1]
    return (Wr - dtype(0.5) * om) / W, W


def quantile_sorted(u, p, q, dtype=np.float64):
    n = u.size
    q = dtype(q)
    if q <= p[0]:
        return float(u[0])
    if q >= p[n - 1]:
        return float(u[n - 1])
    r = int(np.nonzero(p <= q)[0].max())
    t = (q - p[r]) / (p[r + 1] - p[r])
    if dtype is np.float64:
        return _fma(t, np.float64(u[r + 1]) - np.float64(u[r]), u[r])
    return float(LD(t) * (LD(u[r + 1]) - LD(u[r])) + LD(u[r]))


def summary(v, w=None, probs=(0.025, 0.5, 0.975), truth=None, dtype=np.float64):
    """(quant (nq,), cdf or None) of one segment"""
    v = np.asarray(v, dtype=np.float64)
    nq = len(probs)
    if not np.all(np.isfinite(v)):
        return np.full(nq, np.nan), (np.nan if truth is not None else None)
    u, om = sorted_segment(v, w)
    p, W = knots(om, dtype)
    qs = np.array([quantile_sorted(u, p, q, dtype) for q in probs])
    cdf = None
    if truth is not None:
        cdf = cdf_sorted(u, om, W, truth, dtype)
    return qs, cdf


def cdf_sorted(u, om, W, tau, dtype=np.float64):
    tau = float(tau)
    if np.isnan(tau):
        return np.nan
    om = np.asarray(om).astype(dtype)
    L = dtype(0)
    E = dtype(0)
    for x, o in zip(u, om):               # left to right in sorted order
        if x < tau:
            L = dtype(L + o)
        elif x == tau:
            E = dtype(E + o)
    if dtype is np.float64:
        return _fma(0.5, E, L) / float(W)
    return float((LD(0.5) * LD(E) + LD(L)) / LD(W))


def quantile_bound(v, w, q, K):
    """allowed |Q_device - Q_reference| for unequal weights: 1e-12 of the range plus what the long-double reference computes as
    the effect of moving the knots by a relative 4 K 2^-53 of the sums (each knot by up to twice that, so q by up to four times)"""
    u, om = sorted_segment(v, w)
    p, _ = knots(om, LD)
    d = 4.0 * K * 2.0 ** -53
    q0 = quantile_sorted(u, p, q, LD)
    eff = max(abs(quantile_sorted(u, p, min(1.0, q + 4 * d), LD) - q0), abs(quantile_sorted(u, p, max(0.0, q - 4 * d), LD) - q0))
    return q0, 1e-12 * (u[-1] - u[0]) + eff
