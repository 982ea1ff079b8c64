"""Long-double NumPy reference of the Box-Cox skewness search and transform (include/abcsmc_hip.h, "Box-Cox transform of the
metrics"): the grid loop, the definition with two-pass centred sums, the pick rule, the status bits, the transform, and the
reference implementation's own double-precision formula (AbcUtil.cpp:82-105) for comparison.  No GPU, no library."""
import numpy as np

LD = np.longdouble
BAD, CONSTANT, SKIPPED = 1, 2, 4
MAXL = 512


def grid(lambda_min=-5.0, lambda_max=5.0, step=0.1):
    """lambda_0 = min, lambda_{k+1} = lambda_k + step in float64 while lambda_k <= max, the three arguments first rounded to
    float32 (the reference's `const float` parameters) and widened"""
    lo, hi, st = (float(np.float32(v)) for v in (lambda_min, lambda_max, step))
    out = []
    lam = lo
    while lam <= hi:
        out.append(lam)
        lam = lam + st
        if len(out) > MAXL:
            raise ValueError("grid too long")
    return np.array(out, dtype=np.float64)


def skew_centred(t):
    """(sum (t - tbar)^3 / N) / (sum (t - tbar)^2 / (N - 1))^(3/2) in long double, two passes"""
    t = np.asarray(t, dtype=LD)
    n = t.size
    c = t - t.sum() / LD(n)
    m2 = (c * c).sum() / LD(n - 1)
    return ((c * c * c).sum() / LD(n)) / (m2 * np.sqrt(m2))


def skew_table(x, lambdas, shift=0.0):
    """the definition for one column: skew[k] as long double (NaN row for an invalid column, zeros for a constant one), status
    bits 0 and 1"""
    z = np.asarray(x, dtype=np.float64) + np.float64(shift)              # z_i = x_ij + c_j is an fp64 sum
    L = len(lambdas)
    if not (np.isfinite(z).all() and (z > 0).all()):
        return np.full(L, np.nan, dtype=LD), BAD
    if z.min() == z.max():
        return np.zeros(L, dtype=LD), CONSTANT
    l = np.log(z.astype(LD))
    u = l - l.sum() / LD(l.size)
    out = np.empty(L, dtype=LD)
    with np.errstate(all="ignore"):
        for k, lam in enumerate(lambdas):
            if lam == 0:
                out[k] = skew_centred(u)
            else:
                # t - 1 in place of t: the same skewness (a shift), but exp(lambda u) rounded to long double keeps only
                # 1e-19 / |lambda u| of t - tbar, 1e-6 of it on a narrow column at the grid's lambda = 7.45e-8
                s = skew_centred(np.expm1(LD(lam) * u))
                out[k] = s if lam > 0 else -s
    return out, 0


def pick(skews):
    """the reference's rule: ascending k, strict |skew_k| < |best| from +inf, a non-finite skew never taken, 0 if none;
    -> (pick, some skew was non-finite)"""
    best, pk, skipped = np.inf, 0, False
    for k, s in enumerate(skews):
        if not np.isfinite(s):
            skipped = True
            continue
        if abs(s) < abs(best):
            best, pk = s, k
    return pk, skipped


def margin(skews):
    """second-smallest minus smallest |skew| over the finite entries (inf with fewer than two)"""
    a = np.sort(np.abs(np.asarray(skews, dtype=LD)[np.isfinite(np.asarray(skews, dtype=np.float64))]))
    return float(a[1] - a[0]) if a.size > 1 else np.inf


def search(X, lambdas, shift=None):
    """every column of X (N, M): dict(lam, pick, status, skew (M, L) long double, skew_best)"""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    M = X.shape[1]
    sh = np.zeros(M) if shift is None else np.broadcast_to(np.asarray(shift, dtype=np.float64), (M,))
    r = dict(lam=np.empty(M), pick=np.empty(M, dtype=np.int32), status=np.empty(M, dtype=np.int32),
             skew=np.empty((M, len(lambdas)), dtype=LD), skew_best=np.empty(M, dtype=LD))
    for j in range(M):
        sk, st = skew_table(X[:, j], lambdas, sh[j])
        if st & BAD:
            pk, lam = -1, 1.0
        else:
            pk, skipped = pick(sk)
            st |= SKIPPED if skipped else 0
            lam = lambdas[pk]
        r["lam"][j], r["pick"][j], r["status"][j], r["skew"][j], r["skew_best"][j] = lam, pk, st, sk, sk[max(pk, 0)]
    return r


def apply(x, lam, shift=0.0):
    """y = expm1(lam l) / lam (lam == 0: l), l = log(x + shift), in long double; -> (y, |lam l|) as long double"""
    with np.errstate(all="ignore"):
        z = (np.asarray(x, dtype=np.float64) + np.float64(shift)).astype(LD)
        l = np.log(z)
        if lam == 0:
            return l, np.zeros_like(l)
        a = LD(lam) * l
        return np.expm1(a) / LD(lam), np.abs(a)


def reference_double_skew(data):
    """ABC::skewness (AbcUtil.cpp:82-87) as the reference evaluates it, in float64"""
    data = np.asarray(data, dtype=np.float64)
    m = data.mean()
    v = ((data - m) ** 2).sum() / (data.size - 1)
    if v == 0:
        return 0.0
    return (((data - m) ** 3).sum() / data.size) / v ** 1.5


def reference_double_search(x, lambdas):
    """ABC::optimize_box_cox (AbcUtil.cpp:89-105) in float64: (skew per grid value, pick)"""
    x = np.asarray(x, dtype=np.float64)
    sk = np.empty(len(lambdas))
    with np.errstate(all="ignore"):
        for k, lam in enumerate(lambdas):
            sk[k] = reference_double_skew(np.log(x)) if lam == 0 else reference_double_skew((x ** lam - 1) / lam)
    best, pk = np.inf, 0
    for k, s in enumerate(sk):
        if abs(s) < abs(best):
            best, pk = s, k
    return sk, pk


# ---- the column families of the tests (seeded; the same arrays on the CPU and the GPU side) ---------------------------------------
FAMILIES = ("lognormal", "gamma", "uniform", "sqnormal", "nearconst", "wide1000", "wide1000_shift")
ORDINARY = FAMILIES[:4]


def column(family, N, seed):
    """(x (N,), shift) of one test column"""
    g = np.random.default_rng([seed, FAMILIES.index(family), N])
    if family == "lognormal":
        return np.exp(0.6 * g.standard_normal(N) + 1.0), 0.0
    if family == "gamma":
        return g.gamma(2.5, 1.7, N) + 1e-3, 0.0
    if family == "uniform":
        return g.uniform(0.5, 3.0, N), 0.0
    if family == "sqnormal":
        return g.standard_normal(N) ** 2 + 1e-2, 0.0
    if family == "nearconst":
        return 1000.0 * (1.0 + 1e-6 * g.uniform(0.0, 1.0, N) ** 2), 0.0       # relative spread 1e-6, right-skewed
    if family == "wide1000":
        return 1000.0 + 50.0 * g.uniform(-1.0, 1.0, N), 0.0
    if family == "wide1000_shift":
        return 1000.0 + 50.0 * g.uniform(-1.0, 1.0, N), -900.0
    raise KeyError(family)


def near_tie_column(N=1000, seed=3):
    """(x, grid): a column whose logs are symmetric about 0, and a grid symmetric about 0 without 0.  exp(-lambda u) is then the same
    multiset as exp(lambda u), so skew(-lambda) = -skew(lambda) up to rounding: the two grid values next to 0 tie for the pick."""
    a = np.random.default_rng([seed, N]).uniform(0.1, 1.0, N // 2)
    return np.exp(np.concatenate([a, -a])), grid(-1.75, 1.75, 0.5)


def near_tie_indices(skews):
    """the two indices with the smallest |skew|"""
    return sorted(int(i) for i in np.argsort(np.abs(np.asarray(skews, dtype=np.float64)))[:2])


def table(N, M, seed):
    """(X (N, M), shift (M,)): column j is family j mod 7"""
    cols = [column(FAMILIES[j % len(FAMILIES)], N, seed + j // len(FAMILIES)) for j in range(M)]
    return np.stack([c[0] for c in cols], axis=1), np.array([c[1] for c in cols])
