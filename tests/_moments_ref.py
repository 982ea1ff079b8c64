"""Host model of the posterior's moments (mvn.hip: k_cov_chol, k_post_tail<PP>, k_dv_from_stats; weights.hip:
k_doubled_variance): a long-double reference, an fp64 emulation of the kernels' arithmetic with switches for deliberately wrong
variants, and entrywise bounds on what the kernels may differ from the reference by.

The reference (AbcUtil.cpp:462-488, 528-537): two-pass centred covariance with n - 1, its diagonal doubled, the Cholesky factor of
that in gsl_linalg_cholesky_decomp1's layout (lower triangle and diagonal: L; strict upper triangle: the covariance entries),
dv = the doubled diagonal (0 for fewer than 2 rows).

THE BOUNDS.  They follow from the operations of the kernels, in any summation order, with eps = 2^-53; nothing in them is fitted
to device output.

(1) E, the Gram path (gram.hip k_pilot_shift + k_gram + k_stats_reduce, then mvn.hip).  With shift s (the pilot), d = theta - s,
delta = mean(d), m = mean|d| (columnwise), n = K:
  - the kernel forms d^ = fl(theta - s): one rounding, |d^ - d| <= eps |d|;
  - g^_ab = sum_k d^_ka d^_kb by fused multiply-adds in some order, partial records added after: a term passes at most K
    roundings, so |g^ - g| <= (K + 2) eps |d|'|d|;
  - the column sum likewise: |s^_a - sum_k d_ka| <= K eps sum_k |d_ka| -- relative to the sum of the MAGNITUDES, not to the sum;
    delta^ = s^ / n adds one rounding: |delta^_a - delta_a| <= (K + 1) eps m_a;
  - n delta^_a delta^_b (two roundings) is then off by at most (K + 2) eps n (m_a |delta_b| + |delta_a| m_b), as |delta| <= m;
  - the subtraction and the division by n - 1 add 2 eps of both terms; doubling the diagonal is exact.
  Together, with K + 8 in place of K + 4 for the second-order terms and the (exact here) sum of the two partitions:
      E = (K + 8) eps (|d|'|d| + K (m |delta|' + |delta| m')) / (K - 1),   diagonal doubled.
  (The form this started from had 3 K |delta||delta|' for the mean's share.  It misses the rounding of the column sum named
  above, which is of the size of m, not of delta: with a pilot close to the mean, |delta| is far below m.)
  dv of the Gram path (dv_of_stats) is the diagonal of the same expression, clamped at 0 from below, which moves it towards
  the truth: diag(E) bounds it.

(2) B, the factor.  cov_chol_wave / cov_chol_regs compute column j as GSL does: temp = sum_{k<j} A_jk A_ik (a product and an add
each, j roundings per term at most), A_ij -= temp (one more), then the WHOLE column, diagonal included, times inv =
fl(1 / fl(sqrt(A_jj))).  So L_ij L_jj = v_ij (1 + e)^6 where the reference has v_ij exactly, and the computed factor is the
exact factor of C^ + dA with |dA| <= (P + 8) eps |L||L|' (the textbook (P + 1) assumes a division by the rounded root; the
rounded reciprocal, applied to the diagonal too, is the rounding that form misses).  First-order perturbation of a Cholesky
factor: dL = L Phi(L^-1 dC L^-T), Phi = lower triangle with half the diagonal; entrywise in absolute values, and doubled for
the second order:
      B = 2 |L| tril(|L^-1| (E + (P + 8) eps |L||L|') |L^-T|).

(3) E2, the two-pass kernel k_doubled_variance, which centres on the column's first row x0 first: d = x - x0, e = x - mean(x).
  - d^ = fl(x - x0), m^ = fl(sum d^ / K): |m^ - mean(d)| <= eta = (K + 1) eps mean|d|;
  - e^ = fl(d^ - m^): |e^ - e| <= eps |d| + eta + eps |e|.  In sum e^2 - sum e^2 = 2 sum e (e^ - e) + sum (e^ - e)^2 the share
    of m^ in the first sum is (m^ - mean d) sum e = 0, so the first order is 2 eps sum |e| (|d| + |e|) and the mean's error enters
    squared only: sum (e^ - e)^2 <= K (eta + eps (max|d| + max|e|))^2;
  - the fma sum of K squares, the division and the (exact) doubling: (K + 2) eps sum e^2.
      E2 = 2 ((K + 8) eps sum e^2 + 2 eps sum |e||d| + K (eta + eps (max|d| + max|e|))^2) / (K - 1).
  A constant column has d = 0 exactly, hence m^ = 0, e^ = 0 and dv = 0.0 exactly; E2 is 0 there as well."""
import numpy as np

EPS = 2.0 ** -53
LD = np.longdouble
PILOT_ROWS = 256


# ---- the long-double reference -------------------------------------------------------------------------------------------------
def chol_ld(A):
    """lower Cholesky factor of A in long double"""
    A = np.asarray(A).astype(LD)
    P = A.shape[0]
    L = np.zeros_like(A)
    for j in range(P):
        s = A[j, j] - np.sum(L[j, :j] ** 2)
        L[j, j] = np.sqrt(s)
        if j + 1 < P:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _centred(t):
    """t minus its column means, long double.  The first row is taken off first (the deviations do not depend on it): the mean
    of K copies of c need not be c even in long double, and a constant column's deviations are to be exactly 0"""
    d = t - t[0]
    return d - d.mean(axis=0)


def cov_ld(th):
    """doubled-diagonal n - 1 covariance of the rows of th, two-pass centred, long double (zeros for fewer than 2 rows)"""
    t = np.asarray(th).astype(LD)
    K, P = t.shape
    if K < 2:
        return np.zeros((P, P), dtype=LD)
    d = _centred(t)
    cov = (d.T @ d) / LD(K - 1)
    cov[np.diag_indices(P)] *= 2
    return cov


def gsl_layout(L, cov):
    """lower triangle and diagonal from L, strict upper triangle from cov"""
    return np.tril(L) + np.triu(cov, 1)


def reference(th, factor=True):
    """dict: cov (long double, diagonal doubled), dv (fp64), L (fp64 lower factor), gsl_ld / Lgsl (GSL's layout, long double / fp64)"""
    cov = cov_ld(th)
    out = {"cov": cov, "dv": np.diag(cov).astype(np.float64)}
    if factor:
        L = chol_ld(cov)
        out["L"] = L.astype(np.float64)
        out["gsl_ld"] = gsl_layout(L, cov)
        out["Lgsl"] = out["gsl_ld"].astype(np.float64)
    return out


# ---- the kernels' arithmetic in fp64 -------------------------------------------------------------------------------------------
def pilot_shift(th, last=False):
    """k_pilot_shift: the mean of the first min(K, 256) rows (last: of the last ones -- a wrong variant)"""
    th = np.asarray(th, dtype=np.float64)
    m = min(th.shape[0], PILOT_ROWS)
    rows = th[-m:] if last else th[:m]
    return rows.sum(axis=0) / m


def chol_gsl_f64(A, transposed=False):
    """gsl_linalg_cholesky_decomp1's order in fp64, as cov_chol_wave runs it: temp += a * b (product and add rounded separately),
    A_ij -= temp, the column from the diagonal down times 1 / sqrt(A_jj).  Returns (matrix in GSL's layout, ok)"""
    A = np.array(A, dtype=np.float64)
    P = A.shape[0]
    ok = True
    for j in range(P):
        temp = np.zeros(P - j)
        for k in range(j):
            temp = temp + A[j, k] * A[j:, k]
        A[j:, j] += -1.0 * temp
        ajj = A[j, j]
        if not ajj > 0.0:
            ok = False
            break
        inv = 1.0 / np.sqrt(ajj)
        A[j:, j] *= inv
    return (A.T.copy() if transposed else A), ok


def emulate(th, shifted=True, nm1=True, doubled=True, transposed=False, pilot_last=False):
    """What the Gram path computes, in fp64: pilot shift, one-pass sums of the shifted values, (G - n delta delta') / (n - 1), the
    diagonal doubled, the factor in GSL's order.  The switches turn single steps into wrong variants.
    Returns dict: Lgsl (P x P, GSL's layout), dv, ok"""
    th = np.asarray(th, dtype=np.float64)
    K, P = th.shape
    s = pilot_shift(th, last=pilot_last) if shifted else np.zeros(P)
    d = th - s
    n = float(K)
    G = d.T @ d
    delta = d.sum(axis=0) / n
    den = (n - 1.0) if nm1 else n
    C_ = (G - n * delta[:, None] * delta[None, :]) / den
    ss = np.maximum(np.diag(G) - n * delta * delta, 0.0)
    dv = 2.0 * (ss / den) if K > 1 else np.zeros(P)
    if doubled:
        C_[np.diag_indices(P)] *= 2.0
    else:
        dv = 0.5 * dv
    Lg, ok = chol_gsl_f64(C_, transposed)
    return {"Lgsl": Lg, "dv": dv, "ok": ok}


def _block_sum_256(col_terms):
    """block_sum_256 over a column's terms: thread t adds terms t, t + 256, ... in order, the 64 lanes of a wave meet in an xor
    butterfly, then (w0 + w1) + (w2 + w3)"""
    s = np.zeros(256)
    for i in range(0, len(col_terms), 256):
        c = col_terms[i:i + 256]
        s[:len(c)] = s[:len(c)] + c
    v = s.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return (v[0, 0] + v[1, 0]) + (v[2, 0] + v[3, 0])


def emulate_two_pass_dv(col, centre_first_row=True):
    """k_doubled_variance on one column in fp64.  centre_first_row=False: the kernel as it was, mean = block sum / K of the raw
    values -- its dv of a constant column is K e^2 > 0 whenever that mean misses the constant by e"""
    col = np.asarray(col, dtype=np.float64)
    K = len(col)
    x0 = col[0] if (centre_first_row and K) else 0.0
    d = col - x0
    mean = _block_sum_256(d) / float(K)
    e = d - mean
    sq = np.zeros(256)
    for i in range(0, K, 256):                  # ss = fma(e, e, ss) per thread: one rounding per step, as long double does it
        c = e[i:i + 256].astype(LD)
        sq[:len(c)] = (sq[:len(c)].astype(LD) + c * c).astype(np.float64)
    v = sq.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    ss = (v[0, 0] + v[1, 0]) + (v[2, 0] + v[3, 0])
    return 2.0 * (ss / float(K - 1)) if K > 1 else 0.0


# ---- the bounds ----------------------------------------------------------------------------------------------------------------
def cov_bound(th, shift=None):
    """E of (1): entrywise bound on the device's doubled covariance for the shift the kernels use (default: the true pilot)"""
    th = np.asarray(th, dtype=np.float64)
    K, P = th.shape
    if K < 2:
        return np.zeros((P, P))
    s = pilot_shift(th) if shift is None else np.asarray(shift, dtype=np.float64)
    d = (th.astype(LD) - s.astype(LD))
    ad = np.abs(d).astype(np.float64)              # (the bound itself in fp64: its own rounding is 1e-16 of it)
    delta = np.abs(d.mean(axis=0)).astype(np.float64)
    m = ad.mean(axis=0)
    E = (K + 8) * EPS * (ad.T @ ad + K * (np.outer(m, delta) + np.outer(delta, m))) / (K - 1)
    E[np.diag_indices(P)] *= 2
    return E


def dv_ld(th):
    """the reference's dv alone, long double: diag(cov_ld(th)) without the P x P products (a copy kept for speed at 130 columns;
    tests/test_moments_ref_cpu.py holds the two together)"""
    t = np.asarray(th).astype(LD)
    K, P = t.shape
    if K < 2:
        return np.zeros(P, dtype=LD)
    d = _centred(t)
    return 2 * (d * d).sum(axis=0) / LD(K - 1)


def dv_bound_gram(th):
    """diag(E) of (1) alone: diag(cov_bound(th)) without the P x P products (a copy of that formula kept for speed; a constant
    changed there changes here -- tests/test_moments_ref_cpu.py holds the two together)"""
    th = np.asarray(th, dtype=np.float64)
    K, P = th.shape
    if K < 2:
        return np.zeros(P)
    d = th.astype(LD) - pilot_shift(th).astype(LD)
    ad = np.abs(d)
    g = (ad * ad).sum(axis=0) + 2 * K * ad.mean(axis=0) * np.abs(d.mean(axis=0))
    return (2 * (K + 8) * EPS * g / (K - 1)).astype(np.float64)


def factor_bound(L, E):
    """B of (2) for the reference factor L (fp64, lower) and the covariance bound E"""
    L = np.tril(np.asarray(L, dtype=np.float64))
    P = L.shape[0]
    aL = np.abs(L)
    Li = np.abs(np.linalg.inv(L))
    return 2.0 * aL @ np.tril(Li @ (E + (P + 8) * EPS * aL @ aL.T) @ Li.T)


def dv_bound_two_pass(th):
    """E2 of (3), per column"""
    t = np.asarray(th).astype(LD)
    K, P = t.shape
    if K < 2:
        return np.zeros(P)
    d = np.abs(t - t[0])
    e = np.abs(_centred(t))
    eta = (K + 1) * EPS * d.mean(axis=0)
    first = (K + 8) * EPS * (e * e).sum(axis=0) + 2 * EPS * (e * d).sum(axis=0)
    second = K * (eta + EPS * (d.max(axis=0) + e.max(axis=0))) ** 2
    return (2 * (first + second) / (K - 1)).astype(np.float64)


def share(err, bound):
    """largest err / bound over the entries; an error where the bound is 0 counts as infinite, 0 / 0 as 0"""
    err = np.asarray(err, dtype=np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r))


def check_factor(Lgsl_dev, th, ref=None, shift=None):
    """shares of the bounds a device result in GSL's layout takes: (share of B on the lower triangle and diagonal, share of E on
    the strict upper triangle, E, B, ref)"""
    ref = reference(th) if ref is None else ref
    E = cov_bound(th, shift)
    B = factor_bound(ref["L"], E)
    P = E.shape[0]
    lo = np.tril_indices(P)
    up = np.triu_indices(P, 1)
    err = np.abs(np.asarray(Lgsl_dev).astype(LD) - ref["gsl_ld"]).astype(np.float64)     # (against the long-double values)
    return share(err[lo], B[lo]), share(err[up], E[up]), E, B, ref


# ---- test data -----------------------------------------------------------------------------------------------------------------
CONSTANTS = (0.1, 1.0 / 3.0, 7.3, 1e-3)
KINDS = ("benign", "far", "sorted")


def data(kind, K, P, seed, const_col=None, const=None):
    """(K, P) rows.  benign: scales 10^U(-2, 2), correlated columns, means about 100 sd; far: the means at 1e6 sd; sorted: benign
    with the rows ordered by column 0 (the pilot then sits in the lowest rows).  const_col: that column is the constant"""
    g = np.random.default_rng(seed)
    scale = 10.0 ** g.uniform(-2, 2, P)
    A = g.normal(size=(P, P)) / np.sqrt(P) + np.eye(P)
    z = g.normal(size=(K, P)) @ A
    off = {"benign": 100.0, "far": 1e6, "sorted": 100.0}[kind] * g.choice([-1.0, 1.0], P)
    th = (z + off * np.sqrt((A * A).sum(axis=0))) * scale
    if kind == "sorted":
        th = th[np.argsort(th[:, 0], kind="stable")]
    if const_col is not None:
        th[:, const_col] = const
    return np.ascontiguousarray(th)
