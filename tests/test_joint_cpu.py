"""CPU: the NumPy reference of the joint posterior (tests/_joint_ref.py) pinned against numpy.cov, closed forms and the marginal
densities' reference, abcutil.hpd_levels against a gridded bivariate normal, and the library's new bindings, so that the GPU tests
compare the device with something checked."""
import math

import numpy as np
import pytest

import _density_ref as D
import _joint_ref as J


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def test_cov_is_numpy_cov_with_aweights():
    rng = np.random.default_rng(0)
    K, P = 80, 4
    v = rng.normal(size=(K, P)) @ rng.normal(size=(P, P)) + rng.normal(size=P) * 10
    w = rng.uniform(0.1, 1, size=K)
    w[::9] = 0.0                                               # zero weights do not count
    mo = J.moments(v, w)
    assert np.allclose(_f64(mo["cov"]), np.cov(v.T, aweights=w), rtol=1e-12, atol=0)
    assert np.allclose(_f64(mo["mean"]), np.average(v, axis=0, weights=w), rtol=1e-13, atol=0)
    c = np.cov(v.T, aweights=w)
    assert np.allclose(_f64(mo["corr"]), c / np.sqrt(np.outer(np.diag(c), np.diag(c))), rtol=1e-12, atol=0)
    assert np.all(np.diag(mo["corr"]) == 1) and np.array_equal(mo["cov"], mo["cov"].T) and np.array_equal(mo["corr"], mo["corr"].T)
    eq = J.moments(v)                                          # equal weights: the n - 1 covariance
    assert np.allclose(_f64(eq["cov"]), np.cov(v.T), rtol=1e-12, atol=0)


def test_shift_constant_single_entry_and_bad_parameters():
    rng = np.random.default_rng(1)
    v = rng.normal(size=(60, 3))
    w = rng.uniform(0.1, 1, size=60)
    a, b = J.moments(v, w), J.moments(v + 1e6, w)
    scale = np.sqrt(np.outer(np.diag(a["cov"]), np.diag(a["cov"])))
    assert np.all(np.abs(b["cov"] - a["cov"]) <= 1e-9 * scale)                   # two passes: no cancellation
    c = J.moments(np.column_stack([v[:, 0], np.full(60, -2.5)]), w)               # a constant column: variance 0, no correlation
    assert c["cov"][1, 1] == 0 and c["cov"][0, 1] == 0 and np.isnan(c["corr"][0, 1]) and np.isnan(c["corr"][1, 1])
    assert c["corr"][0, 0] == 1
    one = J.moments(v[:1])                                     # one entry: the denominator is 0
    assert np.all(one["cov"] == 0) and np.all(np.isnan(one["corr"])) and np.array_equal(_f64(one["mean"]), v[0])
    one = J.moments(v, np.where(np.arange(60) == 7, 2.0, 0.0))
    assert np.all(one["cov"] == 0) and np.array_equal(_f64(one["mean"]), v[7])
    u = v.copy()
    u[5, 1] = np.nan
    m = J.moments(u, w)
    bad = np.array([False, True, False])
    assert np.array_equal(np.isnan(m["mean"]), bad) and np.array_equal(np.isnan(m["cov"]), bad[:, None] | bad[None, :])
    assert m["cov"][0, 2] == a["cov"][0, 2] and m["corr"][0, 2] == a["corr"][0, 2]
    r = J.joint(u, w, G=5)
    assert np.isnan(r["dens"][0]).all() and np.isnan(r["dens"][2]).all() and np.isfinite(_f64(r["dens"][1])).all()
    assert np.array_equal(r["pairs"], [[0, 1], [0, 2], [1, 2]]) and np.isnan(r["mode"][0]).all() and np.isnan(r["h"][1])


def test_one_entry_is_the_outer_product_of_the_marginals():
    """K = 1: the product kernel factorises, so the pair density is the outer product of the two marginal densities"""
    v = np.array([[3.0, -0.25]])
    G = 33
    r = J.joint(v, G=G)
    a, b = D.density(v[:, 0], G=G), D.density(v[:, 1], G=G)
    assert (r["h"][0], r["lo_x"][0], r["step"][0]) == (a["h"], a["lo_x"], a["step"])
    assert (r["h"][1], r["lo_x"][1], r["step"][1]) == (b["h"], b["lo_x"], b["step"])
    outer = a["dens"][:, None] * b["dens"][None, :]
    assert np.all(np.abs(r["dens"][0] - outer) <= 8 * np.finfo(np.longdouble).eps * outer)
    assert tuple(r["mode"][0]) == (a["mode"], b["mode"])
    # independent columns with equal weights, many entries: the x-marginal of the pair density is the marginal density
    rng = np.random.default_rng(2)
    v = rng.normal(size=(40, 2)) * np.array([1.0, 5.0])
    r = J.joint(v, G=129, cut=9.0)
    a = D.density(v[:, 0], G=129, cut=9.0)
    f = r["dens"][0]
    marg = r["step"][1] * (f.sum(axis=1) - 0.5 * (f[:, 0] + f[:, -1]))
    # trapezoid in y of a Gaussian mixture, bound as in test_integrates_to_one below, relative to the marginal's own scale
    tol = (r["x"][1][-1] - r["x"][1][0]) * r["step"][1] ** 2 * 0.4 / r["h"][1] ** 3 / 12 + 1e-13
    assert np.all(np.abs(marg - a["dens"]) <= tol * a["dens"].max() * np.sqrt(2 * np.pi) * r["h"][0])


def test_integrates_to_one():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(100, 2)) @ np.array([[1.0, 0.6], [0.0, 0.8]])
    w = rng.uniform(0, 1, size=100)
    G = 512
    r = J.joint(v, w, G=G, cut=8.0)
    f = _f64(r["dens"][0])
    tw = np.ones(G)
    tw[0] = tw[-1] = 0.5
    integral = r["step"][0] * r["step"][1] * (tw[:, None] * f * tw[None, :]).sum()
    # T_x T_y f - 1 = T_x (T_y f - m_x) + (T_x m_x - 1), m_x the x-marginal, itself a kernel estimate.  Per axis the trapezoid error
    # is <= (b - a) step^2 max|f''| / 12 with |k''| <= 0.4 / h^3 for a normal density k of scale h, so T_x m_x - 1 is within b_x,
    # and T_y f(x, .) - m_x(x) within b_y m_x(x), which T_x sums to at most b_y (1 + b_x); tails beyond 8 h: < 1e-13 each
    b = [(r["x"][a][-1] - r["x"][a][0]) * r["step"][a] ** 2 * 0.4 / r["h"][a] ** 3 / 12 for a in (0, 1)]
    bound = b[0] + b[1] * (1 + b[0]) + 2e-13
    assert abs(integral - 1.0) <= bound, (integral, bound)
    assert bound < 1e-2


def test_mode_is_the_first_largest_cell_and_transpose():
    rng = np.random.default_rng(4)
    v = rng.normal(size=(30, 3))
    r = J.joint(v, G=9, pairs=[(0, 2), (2, 0)])
    assert np.all(np.abs(r["dens"][0] - r["dens"][1].T) <= 8 * np.finfo(np.longdouble).eps * r["dens"][0])
    g = int(np.argmax(r["dens"][0]))
    assert tuple(r["mode"][0]) == (r["x"][0][g // 9], r["x"][2][g % 9]) and r["mode_dens"][0] == r["dens"][0].max()
    two = np.array([[-1.0, -1.0], [1.0, 1.0]])                 # two equal peaks: the smaller flat index wins
    t = J.joint(two, G=5, cut=0.0, bw=0.3)
    assert tuple(t["mode"][0]) == (-1.0, -1.0)


def test_hpd_levels_of_a_gridded_normal():
    """Standard bivariate normal: the region f >= t holds mass 1 - t / f_max, so level(alpha) = (1 - alpha) f_max.
    On a grid the cumulative sum up to the returned level t differs from that mass by
      - at most one cell's mass f_max sx sy, the step of the cumulative sum at which alpha is reached,
      - the truncated tail, 4 (1 - Phi(L)) for a box reaching L in every direction, which the grid's total lacks,
      - the cells that the contour of t cuts, which the sum counts whole or not at all.  With D the disc f >= t, of radius
        r_t = sqrt(-2 log(t / f_max)), and U the union of the counted cells (those whose centre lies in D), the sum stands for the
        integral over U, and that differs from the integral over D by the mass of U - D less the mass of D - U.  A point of either
        lies within d = half a cell's diagonal of its cell's centre, which is on the other side of the circle, so U - D lies in
        the ring r_t < r <= r_t + d, where f < t, and D - U in the ring r_t - d <= r < r_t, where f <= f_max exp(-(r_t - d)^2 / 2);
        both have at most the area 2 pi d (r_t + d / 2), and the difference of the two masses is at most the larger,
      - the midpoint rule inside cells, (sx^2 + sy^2) / 24 times the integral of |f_xx| (= 4 phi(1) < 1), in the sum and the total.
    A mass error dm moves the level by f_max dm.  The first two terms alone are not a bound: on these grids the definition
    itself is off the closed form by 1.35 times their sum at alpha = 0.5 (steps 0.05 x 0.04) and 2.95 times at alpha = 0.1
    (0.03 x 0.025), the lattice-point discrepancy of the cut cells."""
    from abcsmc_amd import abcutil
    fmax = 1 / (2 * np.pi)
    probs = np.array([0.5, 0.9, 0.95])
    for sx, sy, L in ((0.05, 0.04, 7.0), (0.03, 0.025, 7.0)):
        x, y = np.arange(-L + 0.013, L, sx), np.arange(-L - 0.007, L, sy)            # (not symmetric about the mean)
        f = np.exp(-0.5 * (x[:, None] ** 2 + y[None, :] ** 2)) * fmax
        lv = abcutil.hpd_levels(f, sx, sy, probs)
        reach = min(-x[0], x[-1], -y[0], y[-1]) - max(sx, sy)
        tail = 4 * 0.5 * math.erfc(reach / math.sqrt(2))
        d = 0.5 * math.hypot(sx, sy)
        r = np.sqrt(-2 * np.log(lv / fmax))                     # of the returned levels' own contours
        cut = 2 * np.pi * d * (r + d / 2) * fmax * np.exp(-0.5 * np.maximum(r - d, 0) ** 2)
        tol = fmax * (fmax * sx * sy + tail + cut + 2 * (sx * sx + sy * sy) / 24)
        assert np.all(np.abs(lv - (1 - probs) * fmax) <= tol), (sx, sy, lv, (1 - probs) * fmax, tol)
        assert np.all(tol < 0.025 * fmax)
        assert np.array_equal(lv, J.hpd_levels(f, sx, sy, probs))
    assert np.all(np.diff(abcutil.hpd_levels(f, sx, sy, [0.1, 0.5, 0.9, 1.0])) < 0)
    small = np.array([[1.0, 4.0, 2.0], [0.5, 3.0, 0.25]])      # masses 4, 7, 9, 10, 10.5, 10.75 in descending order of f
    assert abcutil.hpd_levels(small, 1, 1, 1.0) == 0.25 and abcutil.hpd_levels(small, 1, 1, 0.0) == 4.0
    assert np.array_equal(abcutil.hpd_levels(small, 2, 0.5, [0.3, 0.5, 0.9, 0.97, 0.98]), [4.0, 3.0, 1.0, 0.5, 0.25])
    assert abcutil.hpd_levels(f, sx, sy, [[0.5, 0.9]]).shape == (1, 2)
    with pytest.raises(ValueError):
        abcutil.hpd_levels(f, sx, sy, [1.5])
    with pytest.raises(ValueError):
        abcutil.hpd_levels(np.array([[1.0, np.nan]]), 1, 1, [0.5])


def test_library_exposes_the_joint_entries():
    import ctypes as C
    import os
    import __graft_entry__ as g
    from abcsmc_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    L = _lib.lib()
    for n in ("abc_rank_targets_joint_dev", "abc_particle_ranking_pls_targets_joint", "abc_weighted_joint_dev", "abc_weighted_joint"):
        assert n in _lib.SIGNATURES and hasattr(L, n), n
        assert getattr(L, n).argtypes == _lib.SIGNATURES[n][1]
    # abc_joint as the header lays it out: three words, four pointers / sizes, eight output pointers
    assert C.sizeof(_lib.Joint) == 14 * 8 and _lib.Joint.npairs.offset == 40 and _lib.Joint.mean.offset == 48
