"""The header's definition of the k-nearest-neighbour posterior entropy (abc_entropy) in long double, by brute force: every pair's
squared distance, the k-th smallest per row, the Singh et al. (2003) form of the Kozachenko-Leonenko estimate.  The scaled values
are the double division of the definition (they are inputs of the chain, not part of it); everything after them is long double.
tests/test_entropy_cpu.py checks this file against scipy; tests/test_gpu_entropy.py holds the device to it."""
import numpy as np

LD = np.longdouble
EULER = LD("0.577215664901532860606512090082402431042")
PI = LD("3.141592653589793238462643383279502884197")


def psi(k):
    """digamma at the integer k >= 1: -gamma + sum_{m < k} 1 / m"""
    return -EULER + sum((LD(1) / LD(m) for m in range(1, int(k))), LD(0))


def lgamma_half(P):
    """log Gamma(P / 2 + 1): log (P / 2)! for even P, log (sqrt(pi) prod_{m = 0}^{(P - 1) / 2} (m + 1 / 2)) for odd P"""
    P = int(P)
    if P % 2 == 0:
        return sum((np.log(LD(m)) for m in range(1, P // 2 + 1)), LD(0))
    return LD(0.5) * np.log(PI) + sum((np.log(LD(m) + LD(0.5)) for m in range((P - 1) // 2 + 1)), LD(0))


def constant(n, P, k):
    """c = (P / 2) log pi - lgamma(P / 2 + 1) - psi(k) + log n"""
    return LD(P) / 2 * np.log(PI) - lgamma_half(P) - psi(k) + np.log(LD(n))


def scaled(V, scale=None):
    """u = v / scale in double, as the definition makes it"""
    V = np.asarray(V, dtype=np.float64)
    V = V.reshape(-1, 1) if V.ndim == 1 else V
    return V if scale is None else V / np.asarray(scale, dtype=np.float64).reshape(1, -1)


def dist2(U):
    """(K, K) squared distances of the rows of U in long double, +inf on the diagonal (f != e by position)"""
    U = np.asarray(U, dtype=np.float64).astype(LD)
    K, P = U.shape
    D = np.zeros((K, K), dtype=LD)
    for j in range(P):
        d = U[:, None, j] - U[None, :, j]
        D += d * d
    D[np.arange(K), np.arange(K)] = np.inf
    return D


def entropy(V, k=4, scale=None):
    """dict(H, rho2 (K,), zeros) of the rows of V (K, P), all long double; NaN by the rules for K <= k and non-finite values"""
    U = scaled(V, scale)
    K, P = U.shape
    nan = dict(H=LD(np.nan), rho2=np.full(K, np.nan, dtype=LD), zeros=0)
    if K <= k or not np.isfinite(U).all():
        return nan
    rho2 = np.partition(dist2(U), k - 1, axis=1)[:, k - 1]
    zeros = int((rho2 == 0).sum())
    with np.errstate(divide="ignore"):
        logs = np.log(rho2)
    H = LD(-np.inf) if zeros else constant(K, P, k) + LD(P) / (2 * LD(K)) * logs.sum()
    return dict(H=H, rho2=rho2, zeros=zeros, logs=logs)


def entropy_scipy(V, k=4):
    """the same estimate from scipy's parts, in double: cKDTree distances, digamma and gammaln"""
    from scipy.spatial import cKDTree
    from scipy.special import digamma, gammaln
    V = np.asarray(V, dtype=np.float64)
    K, P = V.shape
    rho = cKDTree(V).query(V, k=k + 1)[0][:, k]
    return 0.5 * P * np.log(np.pi) - gammaln(0.5 * P + 1) - digamma(k) + np.log(K) + P / K * np.log(rho).sum()
