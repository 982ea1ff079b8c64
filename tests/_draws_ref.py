"""NumPy form of the posterior draws' definition (include/abcsmc_hip.h, "posterior draws of the batched ranking"), for one target:

    cumulative  c_e = w_0 + ... + w_e in long double (the device sums in fp64 in another fixed order: |dc_e| <= 4 K 2^-53 W)
    selection   block = Philox4x32-10 of counter (lo32(t), hi32(t), s, 0) under key (lo32(seed), hi32(seed)), t the stream id;
                m = (word0 << 21) | (word1 >> 11), u = m 2^-53, tau = u W; src = the smallest e with c_e > tau
    values      smooth: fma(h_j, z_j, v_src[j]), z_j = deviate j mod 4 of normal4 of the block of counter (.., s, 1 + j // 4)

A draw is marked ambiguous when tau lies within 4 K 2^-53 W of a knot: the device's own sums may then put it on the other side.
With equal weights nothing is ambiguous: src = floor(u K) in integer arithmetic.  The deviates come from tests/_philox_ref.py with
their bound zbound (the device evaluates them on the f32 transcendental hardware)."""
import numpy as np

from _philox_ref import normal4_ref, philox4x32_10

M32 = 0xFFFFFFFF


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & M32, seed >> 32


def _counter(stream, S, w3):
    t = int(stream) & 0xFFFFFFFFFFFFFFFF
    s = np.arange(S, dtype=np.uint64)
    full = lambda v: np.full(S, v, dtype=np.uint64)
    return full(t & M32), full(t >> 32), s, full(w3)


def selection_words(seed, stream, S):
    """m (S,) uint64: the 53 selection bits of draws 0..S-1 of a stream; u = m 2^-53"""
    k0, k1 = _key(seed)
    w = philox4x32_10(_counter(stream, S, 0), k0, k1)
    return (w[0] << np.uint64(21)) | (w[1] >> np.uint64(11))


def select(weights, K, seed, stream, S):
    """(src (S,) int64, ambiguous (S,) bool) for K entries with the given weights (None: equal)"""
    m = selection_words(seed, stream, S)
    if weights is None:
        src = np.array([(int(v) * int(K)) >> 53 for v in m], dtype=np.int64)           # floor(u K), exact
        return src, np.zeros(S, dtype=bool)
    w = np.asarray(weights, dtype=np.float64)
    assert w.shape == (K,)
    c = np.cumsum(np.where(w > 0.0, w, 0.0).astype(np.longdouble))
    W = c[-1]
    tau = m.astype(np.longdouble) * np.longdouble(2.0) ** -53 * W
    src = np.minimum(np.searchsorted(c, tau, side="right"), K - 1).astype(np.int64)
    bound = 4.0 * K * np.longdouble(2.0) ** -53 * W
    below = np.where(src > 0, c[np.maximum(src - 1, 0)], np.longdouble(-np.inf))      # the knot at or below tau
    amb = (c[src] - tau <= bound) | (tau - below <= bound)
    return src, np.asarray(amb, dtype=bool)


def noise(seed, stream, S, P):
    """(z, zbound), both (S, P): the deviates of the smoothed draws and the bound on |z_dev - z|"""
    k0, k1 = _key(seed)
    zs, zb = [], []
    for q in range((P + 3) // 4):
        z, b = normal4_ref(philox4x32_10(_counter(stream, S, 1 + q), k0, k1))
        zs.append(z)
        zb.append(b)
    return np.concatenate(zs)[:P].T.copy(), np.concatenate(zb)[:P].T.copy()


def draws(values, weights, seed, stream, S, h=None):
    """The draws of one target.  values: (K, P) rows in ranking order; weights: (K,) or None (equal); h: (P,) bandwidths (the
    smoothed bootstrap) or None.  Returns dict(src, ambiguous (S,), draws (S, P), tol (S, P): bound on |x_dev - x| of a smoothed
    value = h_j zbound + 2 ulp(x), 0 for plain draws)."""
    v = np.asarray(values, dtype=np.float64)
    K, P = v.shape
    src, amb = select(weights, K, seed, stream, S)
    x = v[src]
    tol = np.zeros((S, P))
    if h is not None:
        h = np.asarray(h, dtype=np.float64)
        z, zb = noise(seed, stream, S, P)
        with np.errstate(invalid="ignore"):
            x = (h.astype(np.longdouble) * z + x).astype(np.float64)
            tol = np.abs(h) * zb + 2.0 * np.spacing(np.abs(x))
    return dict(src=src, ambiguous=amb, draws=x, tol=tol)


def ess(weights, K):
    """W^2 / S2 over the entries with w > 0, in long double"""
    if weights is None:
        return np.longdouble(K)
    w = np.asarray(weights, dtype=np.longdouble)
    w = w[w > 0]
    return w.sum() ** 2 / (w * w).sum()
