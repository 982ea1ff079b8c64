"""CPU: the NumPy reference of the weighted posterior densities (tests/_density_ref.py) pinned against closed forms, SciPy and
its own definition, so that the GPU tests compare the device with something checked."""
import numpy as np
import pytest

import _density_ref as D


def test_sd_branch_one_to_ten():
    v = np.arange(1.0, 11.0)
    h, branch = D.bandwidth(v)
    assert branch == "sd"                                     # sd = 3.0277, IQR / 1.34 = 5 / 1.34 = 3.73 (type 5)
    assert h == pytest.approx(0.9 * np.std(v, ddof=1) * 10 ** -0.2, rel=1e-15)
    assert D.bandwidth(v, bw_scale=2.5)[0] == pytest.approx(2.5 * h, rel=1e-15)


def test_iqr_branch():
    v = np.array([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 100.0])        # one outlier inflates the sd
    h, branch = D.bandwidth(v)
    assert branch == "iqr"
    iqr = np.quantile(v, 0.75, method="hazen") - np.quantile(v, 0.25, method="hazen")
    assert h == pytest.approx(0.9 * iqr / 1.34 * 10 ** -0.2, rel=1e-15)


def test_fallbacks():
    assert D.bandwidth([2.5]) == (pytest.approx(0.9 * 2.5, rel=1e-15), "first")           # K = 1: s = 0, IQR = 0, n_eff = 1
    assert D.bandwidth([-3.0] * 7) == (pytest.approx(0.9 * 3.0 * 7 ** -0.2, rel=1e-15), "first")
    assert D.bandwidth([0.0] * 5) == (pytest.approx(0.9 * 5 ** -0.2, rel=1e-15), "one")
    assert D.bandwidth([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 9.0]) [1] == "s"               # IQR = 0 but the values vary
    assert D.bandwidth([0.0, 4.0], [0.0, 1.0]) == (pytest.approx(0.9 * 4.0, rel=1e-15), "first")   # first with positive weight


def test_weighted_moments():
    rng = np.random.default_rng(0)
    v, w = rng.normal(size=50), rng.uniform(0.1, 1, size=50)
    mo = D.moments(v, w)
    W, S2 = w.sum(), (w * w).sum()
    m = (w * v).sum() / W
    assert float(mo["m"]) == pytest.approx(m, rel=1e-13) and float(mo["n_eff"]) == pytest.approx(W * W / S2, rel=1e-13)
    assert float(mo["s"]) ** 2 == pytest.approx((w * (v - m) ** 2).sum() / (W - S2 / W), rel=1e-12)
    assert float(D.moments(v)["s"]) == pytest.approx(np.std(v, ddof=1), rel=1e-13)       # equal weights: the n - 1 variance
    shifted = D.moments(v + 1e6)
    assert float(shifted["s"]) == pytest.approx(np.std(v, ddof=1), rel=1e-9)             # two passes: no cancellation


def test_integrates_to_one():
    rng = np.random.default_rng(1)
    v, w = rng.normal(size=200), rng.uniform(0, 1, size=200)
    r = D.density(v, w, G=4096, cut=8.0)
    f = r["dens"].astype(np.float64)
    integral = r["step"] * (f.sum() - 0.5 * (f[0] + f[-1]))
    # trapezoid error <= (b - a) step^2 max|f''| / 12, |f''| <= max f / h^2 (0.4 / h^3 at most); tails beyond 8 h: < 1e-14
    bound = (r["x"][-1] - r["x"][0]) * r["step"] ** 2 * 0.4 / r["h"] ** 3 / 12 + 1e-13
    assert abs(integral - 1.0) <= bound, (integral, bound)
    assert bound < 1e-3


def test_equals_scipy_mixture():
    from scipy.stats import norm
    rng = np.random.default_rng(2)
    v, w = rng.normal(size=64) * 3 + 5, rng.uniform(0.2, 1, size=64)
    r = D.density(v, w, G=65)
    ref = (w[None, :] * norm.pdf(r["x"][:, None], loc=v[None, :], scale=r["h"])).sum(axis=1) / w.sum()
    assert np.allclose(r["dens"].astype(np.float64), ref, rtol=1e-12, atol=0)
    assert r["mode"] == r["x"][np.argmax(r["dens"])] and r["mode_dens"] == r["dens"].max()
    g = D.density(v, w, G=65, bw=0.7, bw_scale=3.0)            # a given bandwidth: bw_scale not applied
    assert g["h"] == 0.7
    lo_x, step = D.grid(v.min(), v.max(), 0.7, 3.0, 65)
    assert (g["lo_x"], g["step"]) == (lo_x, step) and g["x"][0] == lo_x
    assert abs(g["x"][-1] - (v.max() + 3.0 * 0.7)) <= 4e-16 * abs(g["x"][-1])


def test_zero_weights_change_nothing():
    rng = np.random.default_rng(3)
    v, w = rng.normal(size=40), rng.uniform(0.1, 1, size=40)
    v2 = np.concatenate([[55.0], v[:20], [-70.0, 1e9], v[20:]])
    w2 = np.concatenate([[0.0], w[:20], [0.0, 0.0], w[20:]])
    a, b = D.density(v, w, G=63), D.density(v2, w2, G=63)
    for k in ("h", "lo_x", "step", "mode", "mode_dens"):
        assert a[k] == b[k], k
    assert np.array_equal(a["dens"], b["dens"]) and np.array_equal(a["x"], b["x"])


def test_nan_gives_nan():
    for bad in (np.nan, np.inf, -np.inf):
        r = D.density([1.0, bad, 2.0], [1.0, 0.0, 1.0], G=8)      # even at weight 0
        assert np.isnan(r["h"]) and np.isnan(r["mode"]) and np.isnan(r["mode_dens"]) and np.isnan(r["dens"]).all()


def test_bounds_helpers():
    f = np.array([0.0, 1e-300, 0.5, 2.0], dtype=D.LD)
    b = D.density_bound(f).astype(np.float64)
    assert np.allclose(b, 1e-6 * f.astype(np.float64) + 2e-290, rtol=1e-12)
    v = np.arange(1.0, 11.0)
    h, tol = D.bw_bound(v)
    assert h == D.bandwidth(v)[0] and 0 < tol < 1e-13 * h
