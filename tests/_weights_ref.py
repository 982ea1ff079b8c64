"""A long-double NumPy statement of ABC::weight_predictive_prior (AbcUtil.cpp:539-586) as the oracle restates it
(oracle/abc_oracle.cpp: orc_weights_importance, orc_weights_epanechnikov), for the tests of the weight stage.

The oracle multiplies the per-parameter Gaussian factors of a pair in double, as the reference does: a term below 1e-308
underflows, and a row whose terms all do has no weight there.  Here the terms are kept as logarithms,
    log w'_j - sum_p [(th_ip - tp_jp)^2 / (2 dv_p) + 1/2 log(2 pi dv_p)],
in np.longdouble (64-bit mantissa, 15-bit exponent on x86), and summed over j by a log-sum-exp, so that previous weights of
2^-300 and rows 20 proposal deviations apart keep their digits.  tests/test_weights_ref_cpu.py holds it against the oracle
where the oracle's products are normal numbers.

The loops run over the parameters, not over the pairs: K x K' = 300 x 1200 at 61 parameters takes half a second.
"""
import numpy as np

LD = np.longdouble
PRIOR_GAUSS, PRIOR_UNIF_INT, PRIOR_UNIF_REAL = 0, 1, 2
_TWO_PI = 2 * np.arccos(LD(-1))


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def prior_product(spec, th):
    """prod_p likelihood_p(th_ip) (Priors.h:54-56, 76-78, 102-104) -> K long doubles"""
    th = _ld(th)
    num = np.ones(th.shape[0], dtype=LD)
    for p, (kind, a, b) in enumerate(spec):
        v, a, b = th[:, p], LD(float(a)), LD(float(b))
        if int(kind) == PRIOR_GAUSS:
            u = (v - a) / abs(b)
            f = np.exp(-u * u / 2) / (np.sqrt(_TWO_PI) * abs(b))
        elif int(kind) == PRIOR_UNIF_INT:
            f = np.where((v == np.floor(v)) & (a <= v) & (v <= b), 1 / (b - a + 1), LD(0))
        else:
            f = np.where((a <= v) & (v <= b), 1 / (b - a), LD(0))
        num = num * f
    return num


def log_denominator(th, tp, wp, dv, zero_dv_policy=0):
    """log sum_j w'_j prod_p pdf(th_ip - tp_jp; sqrt(dv_p)) -> K long doubles (-inf: no term; NaN: see raw)"""
    th, tp, wp, dv = _ld(th), _ld(tp), _ld(wp), _ld(dv)
    K, Kp = th.shape[0], tp.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        # terms that vanish (w' = 0, a converged parameter that differs) are kept in a mask and set to -inf at the end: x87
        # arithmetic on infinite operands is an order of magnitude slower
        dead = np.broadcast_to((wp == 0)[None, :], (K, Kp)).copy()
        L = np.broadcast_to(np.log(np.where(wp == 0, LD(1), wp))[None, :], (K, Kp)).copy()     # (a negative or NaN weight: NaN)
        bad = np.zeros((K, Kp), dtype=bool)
        const = LD(0)                                                        # sum_p 1/2 log(2 pi dv_p): the same in every term
        for p in range(th.shape[1]):
            if dv[p] != 0:
                d = th[:, p][:, None] - tp[:, p][None, :]
                L -= d * d * (1 / (2 * dv[p]))                           # (one rounding of 5e-20 more than the division, at a fifth of its time)
                const += np.log(_TWO_PI * dv[p]) / 2
            else:
                # a converged parameter (AbcUtil.cpp:573): factor 1 where the two values are equal; where they differ the
                # reference evaluates a Gaussian of deviation 0 (inf * 0 = NaN: policy 1), the library and the oracle's
                # policy 0 use 0 (the declared deviation)
                differ = th[:, p][:, None] != tp[:, p][None, :]
                if zero_dv_policy == 0:
                    dead |= differ
                else:
                    bad |= differ
        L[dead] = -np.inf
        m = L.max(axis=1)
        ok = np.isfinite(m)
        s = np.full(K, -np.inf, dtype=LD)
        # (terms more than e^-11000 below the row's largest are left out: below a long double's range beside it, and expl is
        # slow on arguments whose result is subnormal or zero)
        rel = L[ok] - m[ok][:, None]
        live = rel > -11000
        s[ok] = m[ok] + np.log((np.exp(np.where(live, rel, LD(0))) * live).sum(axis=1)) - const
        s[np.isnan(m)] = np.nan
        s[bad.any(axis=1)] = np.nan                                          # (w'_j * NaN is NaN whatever w'_j)
    return s


def raw(spec, th, tp, wp, dv, zero_dv_policy=0):
    """the unnormalised weights numerator / denominator (AbcUtil.cpp:557-580) -> K long doubles (a long double holds what a
    double would lose: a denominator below 1e-308 and its reciprocal)"""
    num = prior_product(spec, th)
    ld = log_denominator(th, tp, wp, dv, zero_dv_policy)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # (num / 0 = inf and 0 / 0 = NaN as in the reference's division)
        return np.where(np.isneginf(ld), num / LD(0), num * np.exp(-ld))


def _normalise(w):
    with np.errstate(invalid="ignore", over="ignore"):
        sq = (w * w).sum()
        return (w / np.sqrt(sq) if sq > 0 else w).astype(np.float64)        # Eigen normalize(): only if squaredNorm > 0


def normalised(spec, th, tp, wp, dv, zero_dv_policy=0):
    """raw() divided by its L2 norm (AbcUtil.cpp:583) -> K doubles"""
    return _normalise(raw(spec, th, tp, wp, dv, zero_dv_policy))


def epanechnikov(spec, th, tp, wp, dv, normalise=True):
    """the extension (orc_weights_epanechnikov): numerator / sum_j w'_j max(0, 1 - r2_ij / (P' + 4)), r2 over the P' parameters
    with dv_p != 0; a row nothing supports gets weight 0 -> K doubles (normalised) or long doubles (raw)"""
    num = prior_product(spec, th)
    th, tp, wp, dv = _ld(th), _ld(tp), _ld(wp), _ld(dv)
    K, Kp = th.shape[0], tp.shape[0]
    r2 = np.zeros((K, Kp), dtype=LD)
    pnz = 0
    for p in range(th.shape[1]):
        if dv[p] == 0:
            continue
        pnz += 1
        d = th[:, p][:, None] - tp[:, p][None, :]
        r2 += d * d / dv[p]
    k = 1 - r2 / LD(pnz + 4)
    den = (np.where(k > 0, k, LD(0)) * wp[None, :]).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(den > 0, num / np.where(den > 0, den, LD(1)), LD(0))
    return _normalise(w) if normalise else w
