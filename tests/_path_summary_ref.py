"""NumPy reference of the summaries along a tolerance path (include/abcsmc_hip.h, abc_rank_targets_path_summary_dev).

The definition: segment (b, t, j) is the summaries' segment (_summary_ref.py) built on the first K_t rows of the ranking at
K_max -- path_summary().  Beside it the two facts the rejection kernels rest on, in the form the device uses them:
shared_sort() sorts (key, e) ONCE at K_max and filters by e < K_t; quantile_int() and cdf_int() evaluate a sorted
equal-weight segment with the knots' numerators as exact integers plus a half (H_r = r + 0.5, W = n) and integer counts for the
CDF; walk_down() is the kernels' order of work: the tolerances from the largest down, each list compacted in place from the one
before by per-thread counts and an integer scan."""
import numpy as np

import _summary_ref as R


def path_summary(v, Ks, probs=(0.025, 0.5, 0.975), truth=None, w=None, dtype=np.float64):
    """one (target, parameter): v (K_max,) in ranking order; w: None (equal weights) or a function K -> the K weights of the
    prefix.  Returns (quant (T, nq), cdf (T,) or None): _summary_ref.summary of every prefix"""
    v = np.asarray(v, dtype=np.float64)
    qs, cs = [], []
    for K in Ks:
        q, c = R.summary(v[:K], None if w is None else w(K), probs, truth, dtype)
        qs.append(q)
        cs.append(c)
    return np.array(qs), (np.array(cs, dtype=np.float64) if truth is not None else None)


def shared_sort(v, Ks):
    """the entries sorted once at K_max by (totalOrder key, e), then for every K_t those with e < K_t in that order:
    a list of (u, e) per tolerance"""
    v = np.asarray(v, dtype=np.float64)
    Kmax = int(Ks[-1])
    e = np.arange(Kmax)
    o = e[np.lexsort((e, R.total_order_key(v[:Kmax])))]
    return [(v[o[o < K]], o[o < K]) for K in Ks]


def quantile_int(u, q):
    """the quantile of a sorted equal-weight segment with the knots in integer form: H_r = r + 0.5 and W = n, both exact"""
    n = u.size
    W = float(n)
    q = float(q)
    if q <= 0.5 / W:
        return float(u[0])
    if q >= (float(n - 1) + 0.5) / W:
        return float(u[n - 1])
    lo, hi = 0, n - 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if (float(mid) + 0.5) / W <= q:
            lo = mid
        else:
            hi = mid
    plo, phi = (float(lo) + 0.5) / W, (float(hi) + 0.5) / W
    t = (q - plo) / (phi - plo)
    return R._fma(t, np.float64(u[hi]) - np.float64(u[lo]), u[lo])


def cdf_int(u, tau):
    """F = fma(0.5, E, L) / W from the integer counts of entries below and equal to tau"""
    tau = float(tau)
    if np.isnan(tau):
        return np.nan
    L, E = int(np.count_nonzero(u < tau)), int(np.count_nonzero(u == tau))
    return R._fma(0.5, float(E), float(L)) / float(u.size)


def summary_shared(v, Ks, probs=(0.025, 0.5, 0.975), truth=None):
    """what the rejection kernels compute: one sort, the filter, integer knots; a non-finite value among the first K_t entries
    makes tolerance t NaN and no other"""
    qs, cs = [], []
    for (u, e) in shared_sort(v, Ks):
        if not np.all(np.isfinite(u)):
            qs.append(np.full(len(probs), np.nan))
            cs.append(np.nan)
            continue
        qs.append(np.array([quantile_int(u, q) for q in probs]))
        cs.append(cdf_int(u, truth) if truth is not None else np.nan)
    return np.array(qs), (np.array(cs) if truth is not None else None)


def walk_down(v, Ks, threads=512, per=16):
    """the kernels' walk: the list sorted at K_max; from the largest tolerance down, the first K_t entries are tolerance t's dense
    sorted segment, then they are compacted (stable) to those with e < K_{t-1}: tiles of threads * per entries, every thread
    holding `per` consecutive ones, its kept count scanned over the threads, the tile's offset carried.  Returns the (u, e) lists
    in the order of Ks"""
    v = np.asarray(v, dtype=np.float64)
    Kmax = int(Ks[-1])
    e = np.arange(Kmax)
    o = e[np.lexsort((e, R.total_order_key(v[:Kmax])))]
    key, ids = v[o].copy(), o.copy()
    out = [None] * len(Ks)
    tile = threads * per
    for t in range(len(Ks) - 1, -1, -1):
        n = int(Ks[t])
        out[t] = (key[:n].copy(), ids[:n].copy())
        if t == 0:
            break
        keep = int(Ks[t - 1])
        carry = 0
        for base in range(0, n, tile):
            regs = []                                                    # every thread reads its entries before any writes
            for th in range(threads):
                r0 = base + th * per
                regs.append([(key[r], ids[r]) for r in range(r0, min(r0 + per, n))])
            counts = np.array([sum(1 for _, i in rg if i < keep) for rg in regs])
            offs = np.cumsum(counts) - counts                            # exclusive scan over the threads
            for th in range(threads):
                pos = carry + offs[th]
                for k, i in regs[th]:
                    if i < keep:
                        key[pos], ids[pos] = k, i
                        pos += 1
            carry += int(counts.sum())
        assert carry == keep
    return out
