"""CPU: the NumPy reference of the local-linear adjustment is the regression it claims to be, and the new surfaces exist
(no GPU call)."""
import os
import re
import subprocess

import numpy as np
import pytest

import _loclinear_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(K, nc, P, seed):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((K, nc)) * rng.uniform(0.5, 5.0, nc) + rng.standard_normal(nc)
    o = rng.standard_normal(nc)
    theta = rng.standard_normal((K, P)) + (S - o) @ rng.standard_normal((nc, P))
    dist = np.sort(rng.uniform(0.1, 2.0, K))
    return dist, S, o, theta


def _lstsq(w, x, theta):
    D = np.hstack([np.ones((x.shape[0], 1)), x])
    sw = np.sqrt(w)[:, None]
    return np.linalg.lstsq(D * sw, theta * sw, rcond=None)[0]          # rows: alpha, beta_0 .. beta_{nc-1}


@pytest.mark.parametrize("K,nc,P", [(50, 3, 2), (400, 8, 16), (40, 1, 5), (200, 12, 1)])
def test_reference_equals_weighted_least_squares(K, nc, P):
    dist, S, o, theta = _case(K, nc, P, seed=K + nc)
    r = R.loclinear(dist, S, o, theta, kernel=0)
    w = 1.0 - (dist / dist[-1]) ** 2
    assert np.array_equal(r["weight"], w) and w[-1] == 0.0
    ref = _lstsq(w, S - o, theta)
    scale = theta.max(axis=0) - theta.min(axis=0)
    assert np.all(np.abs(r["coef"] - ref) <= 1e-10 * np.maximum(scale, np.abs(ref).max(axis=0)))
    adj = theta - (S - o) @ ref[1:]
    assert np.all(np.abs(r["theta"] - adj) <= 1e-10 * scale)
    assert r["rank"] == nc and r["status"] == 0


def test_rectangular_kernel_is_ordinary_least_squares():
    dist, S, o, theta = _case(300, 4, 3, seed=3)
    r = R.loclinear(dist, S, o, theta, kernel=1)
    assert np.array_equal(r["weight"], np.ones(300))
    ref = _lstsq(np.ones(300), S - o, theta)
    assert np.allclose(r["coef"], ref, rtol=0, atol=1e-10 * np.abs(ref).max())
    assert r["status"] == 0                     # the rectangular kernel asked for is not a fallback
    # the fitted value at the observation: the plain mean when there are no components
    r0 = R.loclinear(dist, S[:, :0], o[:0], theta, kernel=1)
    assert np.allclose(r0["coef"][0], theta.mean(axis=0), rtol=1e-14) and r0["rank"] == 0


@pytest.mark.parametrize("K,nc", [(2, 3), (3, 5), (4, 4), (6, 8)])
def test_skip_pattern_on_deficient_rank(K, nc):
    """K rows span at most K - 1 centred directions: the first K - 1 pivots are kept, the rest skipped (status bit 0)"""
    dist, S, o, theta = _case(K, nc, 2, seed=10 * K + nc)
    r = R.loclinear(dist, S, o, theta, kernel=1)
    assert r["rank"] == K - 1 and r["status"] == 1
    assert np.all(r["coef"][K:] == 0.0)                              # beta of the skipped components
    assert np.all(np.abs(r["theta"] - r["coef"][0]) <= 1e-9 * np.abs(theta).max())   # an exact fit: every row on alpha
    # a component that does not vary at all (original C_kk == 0) is skipped as well
    S2 = np.array(_case(30, 3, 2, seed=7)[1])
    S2[:, 1] = 4.0
    r2 = R.loclinear(np.linspace(0.1, 1, 30), S2, np.zeros(3), _case(30, 3, 2, seed=7)[3], kernel=0)
    assert r2["rank"] == 2 and r2["coef"][2].tolist() == [0.0, 0.0] and r2["status"] == 1


def test_fallbacks():
    dist, S, o, theta = _case(20, 2, 3, seed=5)
    r = R.loclinear(np.zeros(20), S, o, theta, kernel=0)              # h == 0
    assert r["status"] & 2 and np.array_equal(r["weight"], np.ones(20))
    one = R.loclinear(dist[:1], S[:1], o, theta[:1], kernel=0)        # K = 1: the only weight is 0
    assert one["status"] == 1 | 2 and one["rank"] == 0 and np.array_equal(one["weight"], [1.0])
    assert np.array_equal(one["coef"][0], theta[0]) and np.array_equal(one["theta"], theta[:1])
    flat = R.loclinear(np.full(20, 0.7), S, o, theta, kernel=0)       # all rows at distance h: all weights 0
    assert flat["status"] & 2
    # rectangular asked for: never flagged
    assert not R.loclinear(np.zeros(20), S, o, theta, kernel=1)["status"] & 2


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "abcsmc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    return [a for a in m.group(1).split(",") if a.strip()]


def test_abi_entries_bound():
    from abcsmc_amd import _lib
    for n in ("abc_rank_targets_adjust_dev", "abc_particle_ranking_pls_targets_adjust"):
        assert n in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[n][1]) == len(_header_args(n)), n
    assert [f[0] for f in _lib.AdjustOut._fields_] == ["theta", "weight", "coef", "rank", "status"]


def test_cross_validate_pls_loclinear_uses_alpha(monkeypatch):
    from abcsmc_amd import abcutil
    N, M, P, n = 100, 3, 2, 10
    rng = np.random.default_rng(1)
    X, Y = rng.standard_normal((N, M)), rng.standard_normal((N, P))
    seen = {}

    def fake(Xa, Ya, T, f, K, exclude=None, kernel="epanechnikov", max_comp=0, rule=0, theta=True, ctx=None):
        seen.update(kernel=kernel, theta=theta, exclude=np.array(exclude))
        coef = np.zeros((len(exclude), 3, P))
        coef[:, 0] = Ya[np.asarray(exclude)] + 0.5
        return dict(idx=np.zeros((len(exclude), K), np.uint64), coef=coef, post_mean=coef[:, 0], ncomp=1)

    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets_adjust", fake)
    cv = abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear", kernel="rectangular")
    assert seen["kernel"] == "rectangular" and seen["theta"] is False
    assert np.array_equal(seen["exclude"], cv["rows"])
    th = Y[cv["rows"]]
    assert np.allclose(cv["pred_error"], 0.25 * n / (n * th.var(axis=0, ddof=1)), rtol=1e-14)
    with pytest.raises(ValueError):
        abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="ridge")


def test_facade_declares_adjustment():
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "std::vector<ABC::TargetAdjustment> f(const ABC::Mat2D& X, const ABC::Mat2D& Y, const ABC::Mat2D& T) {\n"
           "  return ABC::particle_ranking_PLS_targets_adjust(X, Y, T, 0.5, 10, 1); }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
