"""CPU: the NumPy reference of the tolerance path is the adjustment's reference on prefixes of one ranking, the ranking's prefix
property it rests on holds with ties, rows past a tolerance never reach it, and the new surfaces exist (no GPU call)."""
import os
import re

import numpy as np

import _loclinear_ref as R
import _path_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(K, nc, P, seed):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((K, nc)) * rng.uniform(0.5, 5.0, nc) + rng.standard_normal(nc)
    o = rng.standard_normal(nc)
    theta = rng.standard_normal((K, P)) + (S - o) @ rng.standard_normal((nc, P))
    dist = np.sort(rng.uniform(0.1, 2.0, K))
    return dist, S, o, theta


def test_one_tolerance_is_loclinear():
    for K, nc, P, kernel in ((1, 2, 3, 0), (7, 3, 2, 0), (300, 8, 16, 0), (300, 4, 1, 1)):
        dist, S, o, theta = _case(K, nc, P, seed=K + nc)
        p = PR.path(dist, S, o, theta, (K,), kernel=kernel, A=nc + 2)
        r = R.loclinear(dist, S, o, theta, kernel=kernel, A=nc + 2)
        assert np.array_equal(p["coef"][0], r["coef"]) and p["rank"][0] == r["rank"] and p["status"][0] == r["status"]
        assert p["h"][0] == dist[-1]
        assert np.allclose(p["post_mean"][0].astype(np.float64), theta.mean(axis=0), rtol=1e-13, atol=1e-15)


def test_every_tolerance_is_loclinear_on_its_prefix():
    dist, S, o, theta = _case(500, 5, 4, seed=11)
    Ks = (1, 2, 40, 256, 257, 500)
    p = PR.path(dist, S, o, theta, Ks, A=8)
    for t, K in enumerate(Ks):
        r = R.loclinear(dist[:K], S[:K], o, theta[:K], A=8)
        assert np.array_equal(p["coef"][t], r["coef"]) and p["rank"][t] == r["rank"] and p["status"][t] == r["status"]
        assert p["h"][t] == dist[K - 1]
    assert p["status"][0] & 2 and p["rank"][0] == 0                 # K = 1: the rectangular fallback
    assert p["coef"].shape == (6, 9, 4) and p["post_mean"].shape == (6, 4)


def test_prefix_property_with_ties():
    """the first K entries of the ascending (dist, row) order are the same for every K' >= K: the ranking at K_max holds every
    smaller tolerance's ranking as a prefix, also where distances tie across the cut"""
    rng = np.random.default_rng(5)
    for trial in range(20):
        N = 400
        d = rng.integers(0, 12, N).astype(np.float64) / 4.0          # many ties
        full = np.lexsort((np.arange(N), d))
        Kmax = int(rng.integers(50, N))
        top = full[:Kmax]
        for K in (1, 2, 17, Kmax // 2, Kmax - 1, Kmax):
            alone = np.lexsort((np.arange(N), d))[:K]               # the ranking at K on its own
            part = np.argpartition(d + np.arange(N) * 1e-9, K - 1)[:K]
            part = part[np.lexsort((part, d[part]))]                # selection then sort, as a top-K does it
            assert np.array_equal(top[:K], alone) and np.array_equal(top[:K], part), (trial, K)
            assert np.array_equal(d[top][:K], d[alone])


def test_rows_past_a_tolerance_do_not_reach_it():
    dist, S, o, theta = _case(300, 4, 3, seed=2)
    Ks = (100, 200, 300)
    clean = PR.path(dist, S, o, theta, Ks)
    bad = theta.copy()
    bad[150, 1] = np.nan
    p = PR.path(dist, S, o, bad, Ks)
    for key in ("post_mean", "coef"):
        assert np.array_equal(p[key][0], clean[key][0]) and np.all(np.isfinite(p[key][0].astype(np.float64)))
        for t in (1, 2):
            col = np.isnan(p[key][t].astype(np.float64))
            assert col[..., 1].any() and not col[..., 0].any() and not col[..., 2].any()
    # a zero weight would not have kept it out: 0 * NaN is NaN
    assert np.isnan(0.0 * bad[150, 1])


def test_surfaces_exist():
    hdr = open(os.path.join(ROOT, "include", "abcsmc_hip.h")).read()
    assert re.search(r"\}\s*abc_path;", hdr)
    for name in ("abc_rank_targets_path_dev", "abc_particle_ranking_pls_targets_path"):
        assert re.search(r"\bint %s\(" % name, hdr), name
    from abcsmc_amd import _lib
    assert [f[0] for f in _lib.Path._fields_] == ["Ks", "T", "post_mean", "coef", "rank", "status", "h"]
    assert "path" not in _lib.PRODUCTS and len(_lib.PRODUCTS) == 4
    assert len(_lib.SIGNATURES["abc_rank_targets_path_dev"][1]) == 18
    assert len(_lib.SIGNATURES["abc_particle_ranking_pls_targets_path"][1]) == 17
    from abcsmc_amd import abcutil
    assert callable(abcutil.particle_ranking_PLS_targets_path) and callable(abcutil.cross_validate_pls_path)
