"""The NumPy form of the posterior draws (tests/_draws_ref.py), which the device is held to in tests/test_gpu_draws.py, on its own:
the selection is a weighted bootstrap (equal weights: floor(u K); zero weights are never drawn; the frequencies follow the weights),
the smoothed draws add noise of variance h^2, and the stream's addressing gives independent streams and prefixes.  No GPU."""
import numpy as np

import _draws_ref as R

SEED = 0x9E3779B97F4A7C15


def test_equal_weights_take_floor_u_k():
    for K in (1, 2, 63, 1000, 1 << 20):
        m = R.selection_words(SEED, 3, 4096)
        src, amb = R.select(None, K, SEED, 3, 4096)
        assert not amb.any()
        assert np.array_equal(src, np.floor(m.astype(np.longdouble) * np.longdouble(2.0) ** -53 * K).astype(np.int64))
        assert src.min() >= 0 and src.max() <= K - 1
        # the weighted path with all weights 1 agrees: c_e = e + 1 exactly
        if K <= 1000:
            src1, amb1 = R.select(np.ones(K), K, SEED, 3, 4096)
            assert np.array_equal(src1[~amb1], src[~amb1])


def test_zero_weight_is_never_drawn():
    K = 64
    rng = np.random.default_rng(1)
    for zero in (0, 31, K - 1):
        w = rng.uniform(0.1, 1.0, size=K)
        w[zero] = 0.0
        src, _ = R.select(w, K, SEED, 0, 1 << 14)
        assert zero not in src
        assert set(range(K)) - {zero} == set(src.tolist())             # every other entry is (2^14 draws of 63 entries)


def test_frequencies_follow_the_weights():
    """chi-square of 2^16 draws from 8 unequal weights: 7 degrees of freedom, 24.32 is the 0.999 quantile"""
    w = np.array([0.05, 0.3, 0.02, 0.2, 0.08, 0.15, 0.12, 0.08])
    S = 1 << 16
    src, amb = R.select(w, 8, SEED, 11, S)
    assert not amb.any()
    n = np.bincount(src, minlength=8)
    e = S * w / w.sum()
    chi2 = float(((n - e) ** 2 / e).sum())
    print("chi-square %.3f on 7 degrees of freedom" % chi2)
    assert chi2 < 24.32


def test_smoothing_adds_h_squared():
    """Var(v_src + h z) = Var(v_src) + h^2 with independent z.  The sample variance of S draws of a variable of variance s^2 and
    bounded kurtosis has a standard error of about s^2 sqrt(2 / S) (exactly for a normal variable); the sum here is a mixture of
    normals around 50 atoms and its excess kurtosis is negative, so 5 sqrt(2 / S) of the expected variance is a 5-sigma bound, and
    the covariance between v_src and h z contributes 2 h s_v / sqrt(S) at one sigma, inside the same bound."""
    rng = np.random.default_rng(2)
    K, P, S = 50, 5, 1 << 15
    v = rng.normal(size=(K, P)) * np.array([1.0, 2.0, 0.5, 3.0, 1.5])
    w = rng.uniform(0.1, 1.0, size=K)
    h = np.array([0.5, 1.0, 0.25, 2.0, 0.1])
    plain = R.draws(v, w, SEED, 5, S)
    smooth = R.draws(v, w, SEED, 5, S, h=h)
    assert np.array_equal(plain["src"], smooth["src"])
    var_p, var_s = plain["draws"].var(axis=0, ddof=1), smooth["draws"].var(axis=0, ddof=1)
    expect = var_p + h * h
    print("variance ratio to plain + h^2:", var_s / expect)
    assert np.all(np.abs(var_s - expect) <= 5.0 * np.sqrt(2.0 / S) * expect)
    # and the noise itself is standard normal per column
    z = (smooth["draws"] - plain["draws"]) / h
    assert np.all(np.abs(z.mean(axis=0)) <= 5.0 / np.sqrt(S))
    assert np.all(np.abs(z.var(axis=0, ddof=1) - 1.0) <= 5.0 * np.sqrt(2.0 / S))


def test_streams_differ():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(100, 4))
    w = rng.uniform(0.1, 1.0, size=100)
    h = np.ones(4)
    a = R.draws(v, w, SEED, 0, 512, h=h)
    for other in (1, 1 << 32, (1 << 32) + 1):                             # the low and the high word of the stream id both count
        b = R.draws(v, w, SEED, other, 512, h=h)
        assert np.mean(a["src"] == b["src"]) < 0.1
        assert not np.any(a["draws"] - v[a["src"]] == b["draws"] - v[b["src"]])
    c = R.draws(v, w, SEED + (1 << 32), 0, 512, h=h)                      # and so do both words of the seed
    assert np.mean(a["src"] == c["src"]) < 0.1


def test_smaller_s_is_a_prefix():
    rng = np.random.default_rng(4)
    v = rng.normal(size=(100, 5))
    w = rng.uniform(0.1, 1.0, size=100)
    h = np.full(5, 0.3)
    big = R.draws(v, w, SEED, 2, 257, h=h)
    small = R.draws(v, w, SEED, 2, 100, h=h)
    for k in ("src", "ambiguous", "draws", "tol"):
        assert np.array_equal(small[k], big[k][:100]), k
