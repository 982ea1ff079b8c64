"""The exact references of the Wilcoxon reduction against each other and against cases small enough to enumerate (no GPU):
oracle/abc_oracle.cpp's orc_wilcoxon_stat / orc_pls_wilcoxon_tests, tests/_wilcoxon_ref.py's rank sum and bounds."""
import itertools

import numpy as np
import pytest

import _wilcoxon_ref as WR


def _brute2(d):
    """(m, 2 W) the slow way: every key's average rank from counting smaller and equal keys"""
    nz = [v for v in d if v != 0.0]
    tot = 0
    for v in nz:
        less = sum(1 for u in nz if abs(u) < abs(v))
        eq = sum(1 for u in nz if abs(u) == abs(v))
        tot += (1 if v > 0 else -1) * (2 * less + eq + 1)          # twice (less + (eq + 1) / 2)
    return len(nz), tot


def _data(kind, n, rng):
    if kind == "plain":
        return rng.normal(size=n)
    if kind == "ties":
        return rng.integers(-4, 5, size=n).astype(float)          # heavy ties, zeros among them
    if kind == "zeros":
        d = rng.normal(size=n)
        d[rng.random(n) < 0.4] = 0.0
        return d
    if kind == "positive":
        return np.abs(rng.normal(size=n)) + 1e-3
    if kind == "negative":
        return -np.abs(rng.integers(1, 6, size=n).astype(float))
    if kind == "allzero":
        return np.zeros(n)
    raise ValueError(kind)


KINDS = ("plain", "ties", "zeros", "positive", "negative", "allzero")


def test_hand_cases():
    # one key; two keys of either order; a tie of two of opposite signs; a tie group of three above a single key
    assert WR.signed_rank_sum2([]) == (0, 0)
    assert WR.signed_rank_sum2([0.0, 0.0]) == (0, 0)
    assert WR.signed_rank_sum2([2.5]) == (1, 2)
    assert WR.signed_rank_sum2([-2.5]) == (1, -2)
    assert WR.signed_rank_sum2([1.0, -3.0]) == (2, 2 * (1 - 2))
    assert WR.signed_rank_sum2([1.0, -1.0]) == (2, 0)                          # both rank 1.5
    assert WR.signed_rank_sum2([0.5, 2.0, -2.0, 2.0, 0.0]) == (4, 2 * 1 + 6 * (1 - 1 + 1))     # ranks 1, then 3, 3, 3
    # 1 .. n all positive: W = n (n + 1) / 2, all negative: minus that
    for n in (1, 2, 7, 300):
        assert WR.signed_rank_sum2(np.arange(1, n + 1.0)) == (n, n * (n + 1))
        assert WR.signed_rank_sum2(-np.arange(1, n + 1.0)) == (n, -n * (n + 1))
    # every sign pattern of four distinct keys
    for signs in itertools.product((-1, 1), repeat=4):
        d = [s * v for s, v in zip(signs, (0.1, 0.2, 0.3, 0.4))]
        assert WR.signed_rank_sum2(d) == (4, 2 * sum(s * r for s, r in zip(signs, (1, 2, 3, 4))))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 1, 2, 5, 63, 257])
def test_the_two_statistics_agree(oracle, kind, n):
    rng = np.random.default_rng(100 + n)
    d = _data(kind, n, rng)
    # the oracle takes two error vectors: |e1| - |e2| = d exactly, for every row, with e1 = max(d, 0) and e2 = max(-d, 0), the
    # signs of the errors themselves at random
    e1 = np.maximum(d, 0.0) * rng.choice([-1.0, 1.0], size=n)
    e2 = np.maximum(-d, 0.0) * rng.choice([-1.0, 1.0], size=n)
    m, W2, p, dd = oracle.wilcoxon_stat(e1, e2, want_d=True) if n else (0, 0, 1.0, np.zeros(0))
    assert np.array_equal(dd, d) and m == int((d != 0.0).sum())
    assert (m, W2) == WR.signed_rank_sum2(d) == _brute2(list(d))
    if n:
        assert p == oracle.wilcoxon_p(e1, e2)                      # the same p the reduction's oracle decides with
        assert abs(p - WR.p_value(m, W2)) <= 1e-15
        assert WR.passes(m, W2) == (p > 0.1) or abs(p - 0.1) < 1e-12


def _random_binning(a_sorted_unique, nbins, rng):
    """a non-decreasing map from the distinct keys to bins 0 .. nbins - 1 (some bins may stay empty)"""
    cuts = np.sort(rng.integers(0, a_sorted_unique.size + 1, size=nbins - 1))
    edges = np.concatenate([[0], cuts, [a_sorted_unique.size]])
    bin_of_unique = np.zeros(a_sorted_unique.size, dtype=np.int64)
    for b in range(nbins):
        bin_of_unique[edges[b]:edges[b + 1]] = b
    return lambda a: bin_of_unique[np.searchsorted(a_sorted_unique, a)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 1, 2, 9, 200])
def test_bounds_contain_the_statistic(kind, n):
    rng = np.random.default_rng(7 * n + 1)
    for rep in range(20):
        d = _data(kind, n, rng)
        m, W2 = WR.signed_rank_sum2(d)
        u = np.unique(np.abs(d[d != 0.0]))
        for nbins in (1, 2, 3, 17, max(1, u.size)):
            call, cpos = WR.bin_counts(d, _random_binning(u, nbins, rng) if u.size else (lambda a: np.zeros(a.size, dtype=np.int64)), nbins)
            assert call.sum() == m
            lo2, hi2 = WR.bounds2(call, cpos)
            assert lo2 <= W2 <= hi2, (kind, n, nbins, lo2, W2, hi2)
        # a single bin: the widest interval, +- m (m + 1) about the sign counts' extremes
        call, cpos = WR.bin_counts(d, lambda a: np.zeros(a.size, dtype=np.int64), 1)
        lo2, hi2 = WR.bounds2(call, cpos)
        p_ = int(cpos[0])
        assert lo2 == 2 * p_ * (p_ + 1) - m * (m + 1) and hi2 == 4 * p_ * m - 2 * p_ * (p_ - 1) - m * (m + 1)
        # all-distinct bins (one bin per distinct key): a point where no tie group mixes signs
        if u.size:
            call, cpos = WR.bin_counts(d, lambda a: np.searchsorted(u, a), u.size)
            lo2, hi2 = WR.bounds2(call, cpos)
            assert lo2 <= W2 <= hi2
            if np.all((cpos == 0) | (cpos == call)):
                assert lo2 == hi2 == W2
            else:
                assert lo2 < hi2


def test_bounds_collapse_to_a_point():
    """every bin one key, or one tie group of one sign: the interval is the statistic"""
    rng = np.random.default_rng(5)
    a = np.repeat(np.arange(1.0, 41.0), rng.integers(1, 5, size=40))           # tie groups of 1 .. 4
    sign_of_group = rng.choice([-1.0, 1.0], size=41)
    d = a * sign_of_group[a.astype(int)]
    u = np.unique(a)
    call, cpos = WR.bin_counts(d, lambda k: np.searchsorted(u, k), u.size)
    m, W2 = WR.signed_rank_sum2(d)
    assert WR.bounds2(call, cpos) == (W2, W2)
    d1 = rng.permutation(np.arange(1.0, 30.0)) * rng.choice([-1.0, 1.0], size=29)          # distinct keys, a bin each
    u1 = np.unique(np.abs(d1))
    call, cpos = WR.bin_counts(d1, lambda k: np.searchsorted(u1, k), u1.size)
    assert WR.bounds2(call, cpos) == (WR.signed_rank_sum2(d1)[1],) * 2
    assert WR.bounds2([], []) == (0, 0) and WR.bounds2([1], [1]) == (2, 2) and WR.bounds2([1], [0]) == (-2, -2)


def test_bin_counts_refuses_a_binning_that_is_not_monotone():
    with pytest.raises(AssertionError):
        WR.bin_counts([1.0, 2.0, 3.0], lambda a: np.array([1, 0, 2]), 3)


def test_oracle_tests_follow_the_reduction(oracle):
    """orc_pls_wilcoxon_tests lists the tests orc_pls_optimal_components decides on, with the same p: the counts that follow from
    its verdicts are the reduction's counts (orc_pls_optimal_components itself is untouched)"""
    rng = np.random.default_rng(3)
    nt, M, P, A = 400, 6, 5, 5
    Xt = rng.normal(size=(nt, M))
    R = rng.normal(size=(M, A)) * 0.4
    Q = rng.normal(size=(P, A)) * np.array([1.0, 0.6, 0.3, 0.1, 0.03])
    Yt = Xt @ R @ Q.T + rng.normal(size=(nt, P)) * 0.8
    Yt[:, 4] = 0.25                                                # a constant response
    best_p, per_p = oracle.pls_optimal_components(Xt, Yt, R, Q, oracle.RULE_MIN_PRESS)
    best_w, per_w = oracle.pls_optimal_components(Xt, Yt, R, Q, oracle.RULE_WILCOXON)
    t = oracle.pls_wilcoxon_tests(Xt, Yt, R, Q, want_d=True)
    assert len(t["seg_j"]) == int(np.sum(per_p - 1)) > 0
    assert [int(a) for j in range(P) for a in range(1, per_p[j])] == t["seg_a"].tolist()
    assert np.array_equal(t["astar"], per_p[t["seg_j"]])
    for s in range(len(t["seg_j"])):
        assert (int(t["m"][s]), int(t["W2"][s])) == WR.signed_rank_sum2(t["d"][s])
        assert t["p"][s] == WR.p_value(t["m"][s], t["W2"][s]) or abs(t["p"][s] - WR.p_value(t["m"][s], t["W2"][s])) < 1e-15
    counts = WR.counts_from_verdicts(t["seg_j"], t["seg_a"], t["p"] > 0.1, per_p)
    assert counts == per_w.tolist() and max(counts) == best_w
    assert np.all(per_w <= per_p)
