"""NumPy reference of the joint posterior of one target (include/abcsmc_hip.h, abc_rank_targets_joint_dev).

Values v (K, P) and weights w (K,) in the ranking's order; only the entries with w > 0 count; a parameter j that holds any
non-finite value is bad: every output that involves j is NaN, the others are unaffected.
  moments      W = sum w, S2 = sum w^2, mean_j = sum w v_j / W, cov_ij = sum w (v_i - mean_i)(v_j - mean_j) / (W - S2 / W), the
               centred sum about the means in a second pass, all in np.longdouble; cov = 0 everywhere when that denominator is <= 0.
               This is numpy.cov(aweights=w).  One triangle is computed and mirrored.
  correlation  corr_ij = cov_ij / (sqrt(cov_ii) sqrt(cov_jj)) clamped to [-1, 1]; corr_ii = 1 when cov_ii > 0; NaN when either
               variance is 0
  bandwidth h_j and grid (lo_x_j, step_j): those of tests/_density_ref.py for segment j (bw.nrd0 on the weighted moments and
               quantiles; a given bandwidth replaces the rule)
  pair density, pair (i, j), i on the first grid axis:
               f(x_g, y_g') = sum_e w_e exp(-((x_g - v_ei) / h_i)^2 / 2) exp(-((y_g' - v_ej) / h_j)^2 / 2) / (W 2 pi h_i h_j)
  joint mode   the smallest flat index g G + g' at which f is largest: (x_g, y_g') and f there"""
import numpy as np

import _density_ref as D

LD = np.longdouble


def bad_parameters(v):
    return ~np.isfinite(np.asarray(v, dtype=np.float64)).all(axis=0)


def moments(v, w=None):
    """dict(mean (P,), cov (P, P), corr (P, P)) in long double; NaN where a bad parameter is involved"""
    v = np.asarray(v, dtype=np.float64)
    K, P = v.shape
    w = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    bad = bad_parameters(v)
    keep = w > 0
    u = np.where(bad[None, :], 0.0, v[keep]).astype(LD)
    om = w[keep].astype(LD)
    W, S2 = om.sum(), (om * om).sum()
    mean = (om[:, None] * u).sum(axis=0) / W
    dev = u - mean[None, :]
    den = W - S2 / W
    cov = np.zeros((P, P), dtype=LD)
    if den > 0:
        for i in range(P):
            for j in range(i, P):
                cov[i, j] = cov[j, i] = (om * dev[:, i] * dev[:, j]).sum() / den
    corr = np.full((P, P), np.nan, dtype=LD)
    for i in range(P):
        for j in range(i, P):
            if cov[i, i] > 0 and cov[j, j] > 0:
                c = LD(1) if i == j else min(max(cov[i, j] / (np.sqrt(cov[i, i]) * np.sqrt(cov[j, j])), LD(-1)), LD(1))
                corr[i, j] = corr[j, i] = c
    mean[bad] = np.nan
    cov[bad, :] = np.nan
    cov[:, bad] = np.nan
    corr[bad, :] = np.nan
    corr[:, bad] = np.nan
    return dict(mean=mean, cov=cov, corr=corr)


def kernel_matrix(v, x, h):
    """E[g, e] = exp(-((x_g - v_e) / h)^2 / 2) in long double"""
    z = (np.asarray(x).astype(LD)[:, None] - np.asarray(v).astype(LD)[None, :]) / LD(h)
    return np.exp(LD(-0.5) * z * z)


def pair_density_at(vi, vj, w, x, y, hi, hj):
    """f (len(x), len(y)) in long double at the given points and bandwidths"""
    vi, vj = np.asarray(vi, dtype=np.float64), np.asarray(vj, dtype=np.float64)
    w = np.ones(vi.size) if w is None else np.asarray(w, dtype=np.float64)
    keep = w > 0
    om = w[keep].astype(LD)
    Ei, Ej = kernel_matrix(vi[keep], x, hi), kernel_matrix(vj[keep], y, hj)
    two_pi = LD(8) * np.arctan(LD(1))
    return (Ei * om[None, :]) @ Ej.T / (om.sum() * two_pi * LD(hi) * LD(hj))


def joint(v, w=None, G=64, cut=3.0, bw=None, bw_scale=1.0, pairs=None):
    """the whole definition for one target: dict(mean, cov, corr, h (P,), lo_x (P,), step (P,), x (P, G), pairs (n, 2),
    dens (n, G, G) long double, mode (n, 2), mode_dens (n,))"""
    v = np.asarray(v, dtype=np.float64)
    K, P = v.shape
    out = moments(v, w)
    bad = bad_parameters(v)
    given = None if bw is None else np.broadcast_to(np.asarray(bw, dtype=np.float64), (P,))
    out["h"] = np.array([np.nan if bad[j] else float(given[j]) if given is not None else D.bandwidth(v[:, j], w, bw_scale)[0]
                         for j in range(P)])
    lo, st = [], []
    for j in range(P):
        if np.isnan(out["h"][j]):
            lo.append(np.nan), st.append(np.nan)
            continue
        u, _ = D.positive(v[:, j], w)
        a, b = D.grid(u.min(), u.max(), out["h"][j], cut, G)
        lo.append(a), st.append(b)
    out["lo_x"], out["step"] = np.array(lo), np.array(st)
    out["x"] = np.array([D.grid_points(lo[j], st[j], G) if np.isfinite(lo[j]) else np.full(G, np.nan) for j in range(P)])
    if pairs is None:
        pairs = [(i, j) for i in range(P) for j in range(i + 1, P)]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n = pairs.shape[0]
    dens = np.full((n, G, G), np.nan, dtype=LD)
    mode, md = np.full((n, 2), np.nan), np.full(n, np.nan, dtype=LD)
    for p, (i, j) in enumerate(pairs):
        if np.isnan(out["h"][i]) or np.isnan(out["h"][j]):
            continue
        f = pair_density_at(v[:, i], v[:, j], w, out["x"][i], out["x"][j], out["h"][i], out["h"][j])
        dens[p] = f
        g = int(np.argmax(f))                                  # the first on ties, in flat order
        mode[p] = out["x"][i][g // G], out["x"][j][g % G]
        md[p] = f.reshape(-1)[g]
    out.update(pairs=pairs, dens=dens, mode=mode, mode_dens=md)
    return out


def density_bound(f_ref):
    """allowed |f_device - f_ref| per cell: the header's accuracy contract over the pair's grid"""
    return D.density_bound(np.asarray(f_ref, dtype=LD).reshape(-1)).reshape(np.shape(f_ref))


def hpd_levels(dens, step_x, step_y, probs):
    """the definition of abcutil.hpd_levels, cell by cell"""
    f = sorted((float(t) for t in np.asarray(dens).reshape(-1)), reverse=True)
    cell = float(step_x) * float(step_y)
    total = 0.0
    for t in f:
        total += t * cell
    out = []
    for a in np.atleast_1d(probs):
        run, level = 0.0, f[-1]
        for t in f:
            run += t * cell
            if run >= a * total:
                level = t
                break
        out.append(level)
    return np.array(out)
