"""Reference of the exact CDF and quantiles of an ABC-GLM marginal (include/abcsmc_hip.h, abc_glm_rank_targets_summary_dev): the
mixture sum_e c_e N(t_e, sigma^2) of one (target, parameter).  NumPy and the standard library only.

F_ref is an exactly rounded sum (math.fsum) of terms c_e erfc(.) / 2, each good to a few ulps; f_ref likewise for the density;
Q_ref is bisection on F_ref inside the guaranteed bracket [min t + sigma z_q, max t + sigma z_q] until no double lies between the
ends.  t, c: the peaks and weights of the counted rows (entries with c <= 0 or a NaN peak are dropped, as the uncounted rows)."""
import math
from statistics import NormalDist

import numpy as np

SQRT2 = math.sqrt(2.0)
U = 2.0 ** -52


def counted(t, c):
    t, c = np.asarray(t, dtype=np.float64).reshape(-1), np.asarray(c, dtype=np.float64).reshape(-1)
    keep = (c > 0) & np.isfinite(t)
    return t[keep].tolist(), c[keep].tolist()


def F_ref(x, t, c, sigma):
    """sum_e c_e Phi((x - t_e) / sigma), t and c as lists of floats"""
    s = sigma * SQRT2
    return math.fsum(ce * 0.5 * math.erfc(-(x - te) / s) for te, ce in zip(t, c))


def f_ref(x, t, c, sigma):
    """the density sum_e c_e N(x; t_e, sigma^2)"""
    k = 1.0 / (sigma * math.sqrt(2.0 * math.pi))
    return math.fsum(ce * k * math.exp(-0.5 * ((x - te) / sigma) ** 2) for te, ce in zip(t, c))


def z_of(q):
    return NormalDist().inv_cdf(q)


def bracket(t, sigma, q, pad=8):
    """the guaranteed bracket of the root of F(x) = q, widened by pad spacings of its larger end for the rounding of its own terms"""
    z = z_of(q)
    lo, hi = min(t) + sigma * z, max(t) + sigma * z
    w = pad * max(np.spacing(abs(lo)), np.spacing(abs(hi)), np.spacing(abs(sigma * z)))
    return lo - w, hi + w


def Q_ref(q, t, c, sigma):
    """bisection on F_ref inside the bracket until no double lies between the ends; the end whose F_ref is nearer q"""
    lo, hi = bracket(t, sigma, q)
    while True:
        mid = lo + 0.5 * (hi - lo)
        if not (lo < mid < hi):
            break
        if F_ref(mid, t, c, sigma) < q:
            lo = mid
        else:
            hi = mid
    return hi if abs(F_ref(hi, t, c, sigma) - q) <= abs(F_ref(lo, t, c, sigma) - q) else lo


def quant_bound(x, t, c, sigma):
    """the bar of |F_ref(quant) - q|: the worst-case rounding of a K-term fp64 sum of values in [0, 1] whose weights add to 1, plus
    what one spacing of x is worth in F (twice, for the two ends of the last bracket)"""
    return (len(t) + 8) * U + 2.0 * f_ref(x, t, c, sigma) * float(np.spacing(abs(x)))


def cdf_bound(t):
    return (len(t) + 8) * U


def summary(peaks, c, T, probs=None, truth=None):
    """quant (nq, P) and cdf (P,) of one target from its peaks (K, P), weights c (K,) and T (P, P): Q_ref and F_ref per parameter;
    a NaN truth gives NaN, -inf gives 0 and +inf gives 1"""
    peaks = np.asarray(peaks, dtype=np.float64)
    P = peaks.shape[1]
    out = {}
    if probs is not None:
        out["quant"] = np.empty((len(probs), P))
    if truth is not None:
        out["cdf"] = np.empty(P)
    for j in range(P):
        t, cc = counted(peaks[:, j], c)
        sigma = math.sqrt(T[j][j])
        if probs is not None:
            for i, q in enumerate(probs):
                out["quant"][i, j] = Q_ref(float(q), t, cc, sigma)
        if truth is not None:
            x = float(truth[j])
            out["cdf"][j] = math.nan if math.isnan(x) else (0.0 if x == -math.inf else (1.0 if x == math.inf else F_ref(x, t, cc, sigma)))
    return out


def numpy_posterior(oracle, R, GC):
    """particle_ranking_PLS_targets_glm's answer, probs and truth included, from the CPU oracle's fit, a NumPy ranking
    (tests/_glm_cases.py) and the references (R: tests/_glm_ref.py); records the keyword arguments of every call in .calls"""
    def call(X, Y, T, training_fraction, K, bw_scale=1.0, exclude=None, max_comp=0, rule=0, ctx=None, outputs=(), **kw):
        call.calls.append(dict(kw, bw_scale=bw_scale, exclude=exclude, max_comp=max_comp, rule=rule, ctx=ctx, outputs=outputs))
        probs, truth = kw.pop("probs", None), kw.pop("truth", None)
        assert not kw, sorted(kw)
        fit = oracle.particle_ranking_pls(X, Y, T[0], training_fraction, max_comp=max_comp, rule=rule)
        nc = fit["ncomp"]
        idx, S, O = GC.rank(X, fit["mean"], fit["sd"], fit["R"], nc, T, K, exclude)
        B, P = T.shape[0], Y.shape[1]
        rs = [R.glm(Y[idx[b]], S[idx[b]], O[b], G=2, bw_scale=bw_scale) for b in range(B)]
        out = {k: np.array([r[k] for r in rs]) for k in ("mean", "mode", "log_md", "status")}
        if probs is not None or truth is not None:
            quant = np.full((B, 0 if probs is None else len(probs), P), np.nan)
            cdf = np.full((B, P), np.nan)
            for b, r in enumerate(rs):
                if r["status"] == 0:
                    s = summary(r["peaks"], r["c"], r["T"], probs, None if truth is None else truth[b])
                    if probs is not None:
                        quant[b] = s["quant"]
                    if truth is not None:
                        cdf[b] = s["cdf"]
            out["quant"] = quant if probs is not None else None
            out["cdf"] = cdf if truth is not None else None
        out.update(idx=idx, ncomp=nc)
        return out
    call.calls = []
    return call


# ---- the device's iteration (k_glm_quant of csrc/glm.hip), restated: plain fp64 sums instead of the kernel's chains and trees ----
QSLACK, QCAP = 24, 64 + 24 + 2


def _ord(x):
    u = int(np.float64(x).view(np.uint64))
    return (~u) & 0xFFFFFFFFFFFFFFFF if u >> 63 else u | 0x8000000000000000


def _unord(k):
    u = k & 0x7FFFFFFFFFFFFFFF if k >> 63 else (~k) & 0xFFFFFFFFFFFFFFFF
    return float(np.uint64(u).view(np.float64))


def newton_model(q, t, c, sigma):
    """(x, iterations): the safeguarded Newton iteration with Halley's correction as the kernel runs it; t, c as arrays"""
    t, c = np.asarray(t, dtype=np.float64), np.asarray(c, dtype=np.float64)
    erfc = np.vectorize(math.erfc, otypes=[np.float64])
    ri = 1.0 / (sigma * 1.4142135623730951)
    kf, kd = ri * 0.5641895835477563, 2.0 * ri
    z, eps = z_of(q), 2.0 ** -49
    mean = float(c @ t)
    sd = math.sqrt(sigma * sigma + float(c @ (t - mean) ** 2))
    tlo, thi, sz = float(t.min()), float(t.max()), sigma * z
    lo = _unord(_ord((tlo + sz) - eps * (abs(tlo) + abs(sz))) - 4)
    hi = _unord(_ord((thi + sz) + eps * (abs(thi) + abs(sz))) + 4)
    x = sd * z + mean
    if not (lo < x < hi):
        x = _unord(_ord(lo) + (_ord(hi) - _ord(lo)) // 2)
    Flo = Fhi = math.nan
    slack = QSLACK
    for it in range(1, QCAP + 1):
        a = (t - x) * ri
        ex = c * np.exp(-(a * a))
        F, E, A = 0.5 * float(np.sum(c * erfc(a))), float(np.sum(ex)), float(np.sum(a * ex))
        r = F - q
        W = _ord(hi) - _ord(lo)
        if r < 0:
            lo, Flo = x, F
        else:
            hi, Fhi = x, F
        W2 = _ord(hi) - _ord(lo)
        if W2 <= 1:
            break
        if W2 > W - W // 2:
            slack -= 1
        with np.errstate(all="ignore"):
            s = np.float64(r) / np.float64(kf * E)
            h = 1.0 - 0.5 * s * (kd * (np.float64(A) / np.float64(E)))
            if 0.5 <= h <= 2.0:
                s = s / h
            xn = float(x - s)
        if xn == x:
            xn = _unord(_ord(x) + 1 if r < 0 else _ord(x) - 1)
        x = xn if (slack > 0 and lo < xn < hi) else _unord(_ord(lo) + W2 // 2)
    up = not math.isnan(Fhi) and (math.isnan(Flo) or Fhi - q <= q - Flo)
    return (hi if up else lo), it
