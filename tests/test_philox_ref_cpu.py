"""The host model of the device noise stream (tests/_philox_ref.py) on its own: Philox known answers, the deviates' stated range,
and the proposal rules on hand-made cases.  No GPU."""
import numpy as np

import _philox_ref as R


def _words(*c):
    return [np.array([w], dtype=np.uint64) for w in c]


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32_10"""
    cases = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
              (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in cases:
        got = R.philox4x32_10(_words(*ctr), *key)
        assert [int(w[0]) for w in got] == list(want), (ctr, key)


def test_philox_key_derivation():
    assert R.philox_key(0, 0, 0) == (0x5BD1E995, 0)
    assert R.philox_key(0x5BD1E995, 7, 1) == (0, 7 ^ 0x9E3779B1)
    assert R.philox_key(1, 2, 3) == (1 ^ 0x5BD1E995, 2 ^ ((3 * 0x9E3779B1) & 0xFFFFFFFF))


def test_normal4_range_and_extreme_words():
    """|z| <= 6.76 (the radius of u = 2^-33), zero radius at the top word, angle 0 from a zero angle word"""
    g = np.random.default_rng(1)
    w = g.integers(0, 2 ** 32, size=(4, 200000), dtype=np.uint64)
    z, zb = R.normal4_ref(w)
    assert np.all(np.abs(z) <= 6.7638) and np.all(zb > 0) and np.all(np.isfinite(zb))
    assert abs(z.mean()) < 0.01 and abs(z.var() - 1.0) < 0.01
    z, zb = R.normal4_ref(np.array(_words(0, 0, 0xFFFFFFFF, 0xFFFFFFFF)))
    assert abs(z[0, 0] - np.sqrt(-2.0 * np.log(0.5 * 2.0 ** -32))) < 1e-6 and z[1, 0] == 0.0      # u = 2^-33, angle 0
    assert z[2, 0] == 0.0 and z[3, 0] == 0.0                                                      # u rounds to 1: radius 0
    assert zb[2, 0] > zb[0, 0]           # the top of the range: one ulp of the logarithm is a large step of the radius


def test_c_round_is_half_away_from_zero():
    v = np.array([0.5, 1.5, 2.5, -0.5, -2.5, 0.49999999999999994, -0.49999999999999994, 3.0, -7.2])
    assert np.array_equal(R.c_round(v), [1.0, 2.0, 3.0, -1.0, -3.0, 0.0, -0.0, 3.0, -7.0])


def _key():
    return R.philox_key(0x12345678, 0x9ABCDEF0, 0x0BADF00D)


def test_identity_factor_equals_independent_noise_of_the_first_deviates():
    """with L = I the multivariate noise of column p is deviate p % 4 of block p // 4; the independent noise of column p is
    deviate 0 of block 0x80000000 | p -- one formula, two counters: the same when the counters agree"""
    K, P, n = 5, 6, 300
    th = np.arange(K * P, dtype=np.float64).reshape(K, P)
    par = np.arange(n) % K
    pri = [(R.UNIF_REAL, -1e300, 1e300)] * P
    mv = R.proposals_ref(_key(), th, par, pri, np.eye(P), True, 7, n)
    z = np.concatenate([R.normal4_ref(R.philox4x32_10(R._counters(np.uint64(7) + np.arange(n, dtype=np.uint64), 0, q), *_key()))[0]
                        for q in range(2)])[:P]
    assert np.array_equal(mv["x"], z.T + th[par]) and np.all(mv["attempt"] == 0) and mv["giveups"] == 0
    ind = R.proposals_ref(_key(), th, par, pri, np.ones(P), False, 7, n)
    for p in range(P):
        w = R.philox4x32_10(R._counters(np.uint64(7) + np.arange(n, dtype=np.uint64), 0, 0x80000000 | p), *_key())
        assert np.array_equal(ind["x"][:, p], R.normal4_ref(w)[0][0] + th[par, p])
    # a multivariate call with L = I is NOT the independent one: the counters differ
    assert not np.allclose(mv["x"], ind["x"])


def test_give_up_rules():
    """multivariate: after the last attempt the parent is kept, one give-up per row; independent: the prior mean, one give-up
    per coordinate"""
    K, n = 3, 5
    th = np.array([[0.5, 1.0], [0.5, 2.0], [0.5, 3.0]])
    par = np.array([0, 1, 2, 1, 0])
    pri = [(R.UNIF_REAL, 0.5, 0.5), (R.GAUSS, 0.0, 5.0)]           # a zero-width support: no candidate lands in it
    mv = R.proposals_ref(_key(), th, par, pri, np.eye(2), True, 0, n, max_attempts=50)
    assert mv["giveups"] == n and np.array_equal(mv["x"], th[par]) and np.all(mv["attempt"] == -1)
    ind = R.proposals_ref(_key(), th, par, [(R.UNIF_REAL, 0.5, 0.5), (R.UNIF_REAL, 4.0, 6.0)], np.array([1.0, 1e-4]),
                          False, 0, n)
    assert ind["giveups"] == 2 * n
    assert np.all(ind["x"][:, 0] == 0.5) and np.all(ind["x"][:, 1] == 5.0)


def test_integer_recasting():
    K, n = 4, 2000
    th = np.column_stack([np.arange(K) * 10.0, np.arange(K) * 1.0])
    par = np.arange(n) % K
    pri = [(R.UNIF_INT, 0, 40), (R.UNIF_REAL, -100, 100)]
    L = np.array([[3.0, 0.0], [0.5, 1.0]])
    out = R.proposals_ref(_key(), th, par, pri, L, True, 0, n)
    assert np.all(out["x"][:, 0] == np.round(out["x"][:, 0])) and out["x"][:, 0].min() >= 0 and out["x"][:, 0].max() <= 40
    assert np.all(out["tol"][:, 0] == 0.0) and np.all(out["tol"][:, 1] > 0.0)
    assert np.any(out["attempt"] > 0)                  # parent 0 at the edge 0: about half its first candidates are rejected
    # the recast value is the rounding of the candidate the noise model gives
    acc = out["attempt"] >= 0
    gi = np.arange(n, dtype=np.uint64)
    for i in np.flatnonzero(acc)[:50]:
        x, _, _, _ = R.mv_noise_ref(_key(), gi[i:i + 1], int(out["attempt"][i]), L)
        assert out["x"][i, 0] == R.c_round(x[0, 0] + th[par[i], 0])


def test_ambiguity_flag_at_a_constructed_edge():
    """a candidate within its error bound of a uniform edge, of a .5 rounding edge or of the Gaussian underflow edge is
    ambiguous; one clear of them is not"""
    t = np.array([1e-6])
    assert R.recast_valid((R.UNIF_REAL, 0.0, 1.0), np.array([1.0 + 5e-7]), t)[2][0]
    assert not R.recast_valid((R.UNIF_REAL, 0.0, 1.0), np.array([1.0 + 5e-6]), t)[2][0]
    assert R.recast_valid((R.UNIF_INT, 0, 9), np.array([2.5 - 5e-7]), t)[2][0]
    assert not R.recast_valid((R.UNIF_INT, 0, 9), np.array([2.4]), t)[2][0]
    # the Gaussian edge, |u| ~ 38.6 for sigma = 1: valid well inside, invalid well outside, ambiguous where exp(-u^2 / 2) is
    # 1.5 units of 2^-1074 (one unit either way decides whether 0.399 x exp rounds to zero)
    edge = np.sqrt(-2.0 * (np.log(1.5) - 1074.0 * np.log(2.0)))
    v = np.array([38.0, edge, 39.5])
    _, ok, amb = R.recast_valid((R.GAUSS, 0.0, 1.0), v, t)
    assert list(ok[[0, 2]]) == [True, False] and list(amb) == [False, True, False]
    # through proposals_ref: a parent exactly at an edge with a tiny factor flags every row
    th = np.array([[1.0]])
    out = R.proposals_ref(_key(), th, np.zeros(10, dtype=np.int64), [(R.UNIF_REAL, 0.0, 1.0)], np.array([[1e-300]]), True, 0, 10)
    assert np.all(out["ambiguous"])
    out = R.proposals_ref(_key(), th, np.zeros(10, dtype=np.int64), [(R.UNIF_REAL, 0.0, 2.0)], np.array([[0.1]]), True, 0, 10)
    assert not np.any(out["ambiguous"])
