"""NumPy reference of the weighted posterior densities and modes (include/abcsmc_hip.h, abc_rank_targets_density_dev).

One segment at a time: values v and weights w in the ranking's order; only the entries with w > 0 count; a non-finite value
makes every output NaN.
  moments    W = sum w, S2 = sum w^2, m = sum w v / W, n_eff = W^2 / S2, s^2 = sum w (v - m)^2 / (W - S2 / W) (s = 0 when that
             denominator is <= 0), all in np.longdouble, the centred sum about m in a second pass
  bandwidth  R's bw.nrd0: IQR = Q(0.75) - Q(0.25) by tests/_summary_ref.py; lo = min(s, IQR / 1.34); if 0: s; if 0: |v of the
             first entry with w > 0|; if 0: 1;  h = bw_scale * 0.9 * lo * n_eff^(-1/5); a given bandwidth replaces the rule
  grid       lo_x = u_min - cut * h, step = ((u_max + cut * h) - lo_x) / (G - 1) in float64, x_g = fma(g, step, lo_x) exactly
  density    f(x_g) = sum_e w_e exp(-((x_g - v_e) / h)^2 / 2) / (W h sqrt(2 pi)) in np.longdouble
  mode       the first g at which f is largest"""
from fractions import Fraction

import numpy as np

import _summary_ref as S

LD = np.longdouble
EPS = 2.0 ** -53


def positive(v, w=None):
    v = np.asarray(v, dtype=np.float64)
    w = np.ones(v.size) if w is None else np.asarray(w, dtype=np.float64)
    keep = w > 0
    return v[keep], w[keep]


def moments(v, w=None):
    """dict(W, S2, m, n_eff, s) in long double over the entries with positive weight"""
    u, om = positive(v, w)
    u, om = u.astype(LD), om.astype(LD)
    W = om.sum()
    S2 = (om * om).sum()
    m = (om * u).sum() / W
    den = W - S2 / W
    s = np.sqrt((om * (u - m) ** 2).sum() / den) if den > 0 else LD(0)
    return dict(W=W, S2=S2, m=m, n_eff=W * W / S2, s=s)


def bandwidth(v, w=None, bw_scale=1.0, qdtype=np.float64):
    """(h, branch): branch is "sd", "iqr", or the fallback "s", "first", "one" """
    mo = moments(v, w)
    q, _ = S.summary(v, w, probs=(0.25, 0.75), dtype=qdtype)
    iqr = LD(q[1]) - LD(q[0])
    s = mo["s"]
    lo, branch = (s, "sd") if s <= iqr / LD(1.34) else (iqr / LD(1.34), "iqr")
    if lo == 0:
        lo, branch = s, "s"
    if lo == 0:
        lo, branch = LD(abs(positive(v, w)[0][0])), "first"
    if lo == 0:
        lo, branch = LD(1), "one"
    return float(LD(bw_scale) * LD(0.9) * lo * mo["n_eff"] ** LD(-0.2)), branch


def grid(u_min, u_max, h, cut, G):
    """(lo_x, step) in float64, operation by operation as the definition"""
    f = np.float64
    lo_x = f(u_min) - f(cut) * f(h)
    step = ((f(u_max) + f(cut) * f(h)) - lo_x) / f(G - 1)
    return float(lo_x), float(step)


def grid_points(lo_x, step, G):
    """x_g = fma(g, step, lo_x): exact product and sum, one rounding"""
    fl, fs = Fraction(float(lo_x)), Fraction(float(step))
    return np.array([float(fl + g * fs) for g in range(G)])


def density_at(v, w, x, h):
    """f(x) in long double at the given points and bandwidth"""
    u, om = positive(v, w)
    u, om, x, h = u.astype(LD), om.astype(LD), np.asarray(x).astype(LD), LD(h)
    out = np.empty(x.size, dtype=LD)
    for lo in range(0, x.size, 64):                       # (blocks: bounded memory at K = 8193)
        z = (x[lo:lo + 64, None] - u[None, :]) / h
        out[lo:lo + 64] = (om[None, :] * np.exp(LD(-0.5) * z * z)).sum(axis=1)
    return out / (om.sum() * h * np.sqrt(LD(8) * np.arctan(LD(1))))         # sqrt(2 pi)


def density(v, w=None, G=512, cut=3.0, bw=None, bw_scale=1.0):
    """dict(h, lo_x, step, x, dens (long double), mode, mode_dens) of one segment by the definition"""
    v = np.asarray(v, dtype=np.float64)
    if not np.all(np.isfinite(v)):
        nan = np.full(G, np.nan)
        return dict(h=np.nan, lo_x=np.nan, step=np.nan, x=nan, dens=nan, mode=np.nan, mode_dens=np.nan)
    h = float(bw) if bw is not None else bandwidth(v, w, bw_scale)[0]
    u, _ = positive(v, w)
    lo_x, step = grid(u.min(), u.max(), h, cut, G)
    x = grid_points(lo_x, step, G)
    f = density_at(v, w, x, h)
    g = int(np.argmax(f))
    return dict(h=h, lo_x=lo_x, step=step, x=x, dens=f, mode=x[g], mode_dens=f[g])


def density_bound(f_ref):
    """allowed |f_device - f_ref| per grid point: the header's accuracy contract"""
    f_ref = np.asarray(f_ref, dtype=LD)
    return LD(1e-6) * f_ref + LD(1e-290) * f_ref.max()


def bw_bound(v, w=None, bw_scale=1.0):
    """(h_ref, allowed |h_device - h_ref|): relative 4 K 2^-53 + 1e-14 for the device's fixed-order sums, plus
    (4 K 2^-53 max|v| / s)^2 for the rounding of its mean; where the IQR decides (or nearly) and the weights are unequal, the two
    quantiles' own quantile_bound carried through h = bw_scale 0.9 (IQR / 1.34) n_eff^(-1/5)"""
    v = np.asarray(v, dtype=np.float64)
    K = v.size
    u, om = positive(v, w)
    equal = bool(np.all(om == om[0]))
    # equal weights: the device's quantiles are the float64 definition's bits (the final fma's rounding included), so the
    # quantile part is exact; otherwise the long-double quantiles, with their bound below
    h, branch = bandwidth(v, w, bw_scale, qdtype=np.float64 if equal else LD)
    mo = moments(v, w)
    rel = 4.0 * K * EPS + 1e-14
    if mo["s"] > 0:
        rel += float(4.0 * K * EPS * np.abs(positive(v, w)[0]).max() / mo["s"]) ** 2
    tol = rel * h
    if not equal:
        q25, t25 = S.quantile_bound(v, w, 0.25, K)
        q75, t75 = S.quantile_bound(v, w, 0.75, K)
        if (LD(q75) - LD(q25)) / LD(1.34) <= mo["s"] * (1 + LD(1e-6)) + LD(t25 + t75):
            tol += float(bw_scale * 0.9 * (t25 + t75) / 1.34 * float(mo["n_eff"]) ** -0.2)
    return h, tol
