"""Exact references of the Wilcoxon signed-rank reduction (abcsmc_amd/csrc/wilcoxon.hip), in integers.

A test's statistic is W = sum over the non-zero paired differences d_i of sign(d_i) rank(|d_i|), ranks 1 .. m with the
"average" rank for ties.  An average rank is a multiple of 1/2, so 2 W is an integer: everything here works on 2 W, in numpy
int64 (m < 2^31 keeps every sum below 2^63) or Python integers, and nothing is rounded.

    signed_rank_sum2(d)          (m, 2 W) from the differences, by sorted unique |d| and their counts -- a second restatement,
                                 independent of the oracle's sort-and-walk (oracle/abc_oracle.cpp: orc_wilcoxon_stat)
    bounds2(c_all, c_pos)        the interval of 2 W that the counts of ANY non-decreasing binning of the keys leave
    bin_counts(d, bin_of_key)    those counts, for a binning given as a non-decreasing function of |d|
    passes(m, W2) / p_value      a float64 copy of the decision (normal approximation, A&S 26.2.18 polynomial, alpha = 0.1)
    counts_from_verdicts(...)    the per-response component counts that follow from the tests' verdicts

The bounds, derived (not copied from k_wx_bounds).  Bin b holds c keys, p of them of positive differences, and B keys lie in the
bins below it.  Whatever the order inside the bin, its keys take the ranks B + 1 .. B + c between them (tie groups that straddle
nothing: a group lies inside one bin because the binning is a function of the key; average ranks inside the bin keep the bin's
rank total and move a subset's total only between the extremes below).  The ranks of the bin add up to
    T = c B + c (c + 1) / 2,
and the positives' share Pos lies between the p lowest and the p highest of them,
    p B + p (p + 1) / 2  <=  Pos  <=  p B + p c - p (p - 1) / 2.
The bin's part of W is Pos - (T - Pos) = 2 Pos - T, so twice it is 4 Pos - 2 T:
    lo2_b = 4 p B + 2 p (p + 1) - 2 c B - c (c + 1),        hi2_b = 4 p B + 4 p c - 2 p (p - 1) - 2 c B - c (c + 1),
and the interval of 2 W is the sum over the bins.  It is a point when every bin has p = 0 or p = c.
"""
import math

import numpy as np


def signed_rank_sum2(d):
    """(m, 2 W) as Python integers from the paired differences d (zeros dropped, average ranks for ties in |d|)"""
    d = np.asarray(d, dtype=np.float64).ravel()
    nzm = d != 0.0
    a, pos = np.abs(d[nzm]), d[nzm] > 0.0
    m = int(a.size)
    if m == 0:
        return 0, 0
    u, inv, cnt = np.unique(a, return_inverse=True, return_counts=True)
    cnt = cnt.astype(np.int64)
    below = np.cumsum(cnt) - cnt                                   # keys strictly smaller than the group
    rank2 = 2 * below + cnt + 1                                    # twice the average of below + 1 .. below + cnt
    npos = np.bincount(inv, weights=pos, minlength=u.size).astype(np.int64)
    return m, int(np.sum(rank2 * (2 * npos - cnt)))                # (npos - (cnt - npos)) keys of each sign


def bounds2(c_all, c_pos):
    """(lo2, hi2): the interval of 2 W from the per-bin counts of all keys and of positive keys, bins in ascending key order"""
    lo2 = hi2 = 0
    B = 0
    for c, p in zip((int(v) for v in c_all), (int(v) for v in c_pos)):
        assert 0 <= p <= c
        total2 = 2 * c * B + c * (c + 1)
        lo2 += 4 * p * B + 2 * p * (p + 1) - total2
        hi2 += 4 * p * B + 4 * p * c - 2 * p * (p - 1) - total2
        B += c
    return lo2, hi2


def bin_counts(d, bin_of_key, nbins):
    """(c_all, c_pos) of the non-zero differences under bin_of_key: |d| (array) -> bin (integer array), non-decreasing in |d|"""
    d = np.asarray(d, dtype=np.float64).ravel()
    nzm = d != 0.0
    a, pos = np.abs(d[nzm]), d[nzm] > 0.0
    b = np.asarray(bin_of_key(a), dtype=np.int64)
    if a.size > 1:                                                 # the one property the bounds rest on
        o = np.argsort(a, kind="stable")
        assert np.all(np.diff(b[o]) >= 0), "the binning is not a non-decreasing function of |d|"
    return np.bincount(b, minlength=nbins).astype(np.int64), np.bincount(b, weights=pos, minlength=nbins).astype(np.int64)


def normalcdf_poly(z):
    """[PLS] normalcdf, Abramowitz & Stegun 26.2.18, term by term in float64"""
    c1, c2, c3, c4 = 0.196854, 0.115194, 0.000344, 0.019527
    x = abs(float(z))
    dd = 1.0 + c1 * x + c2 * x * x + c3 * x * x * x + c4 * x * x * x * x
    tail = 0.5 / (dd * dd * dd * dd)
    return 1.0 - tail if z >= 0.0 else tail


def p_value(m, W2):
    """two-sided p of the normal approximation; no non-zero difference: 1"""
    m = int(m)
    if m == 0:
        return 1.0
    md = float(m)
    sigma = math.sqrt(md * (md + 1.0) * (2.0 * md + 1.0) / 6.0)
    return 2.0 * (1.0 - normalcdf_poly(abs((float(int(W2)) / 2.0) / sigma)))


def passes(m, W2):
    """the candidate is not significantly different from the optimum (alpha = 0.1)"""
    return p_value(m, W2) > 0.1


def counts_from_verdicts(seg_j, seg_a, passed, optima):
    """per response: the first candidate (ascending a') whose test passes, else the PRESS optimum.  optima: the optimum of EVERY
    response (those with optimum 1 have no test); tests in plan order."""
    out = [int(v) for v in optima]
    done = set()
    for j, a, ok in zip(seg_j, seg_a, passed):
        j = int(j)
        if j in done:
            continue
        if ok:
            out[j] = int(a)
            done.add(j)
    return out
