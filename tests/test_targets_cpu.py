"""CPU: the batched-target ranking's surfaces exist and its cross-validation arithmetic is right (no GPU call)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_entries_bound():
    from abcsmc_amd import _lib
    for n in ("abc_rank_targets_dev", "abc_particle_ranking_pls_targets", "abc_targets_fallbacks"):
        assert n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["abc_rank_targets_dev"][1]) == 18
    assert len(_lib.SIGNATURES["abc_particle_ranking_pls_targets"][1]) == 17


def test_cross_validate_pls_arithmetic(monkeypatch):
    """rows drawn without replacement from the seed, each excluded for its own target, and the cv4abc prediction error
    sum_b (mean_bj - theta_bj)^2 / (n Var_j(theta)) from the means the ranking returns"""
    from abcsmc_amd import abcutil
    N, M, P, n = 200, 3, 4, 25
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((N, M)), rng.standard_normal((N, P))
    Y[:, 3] = 1.0                                   # a parameter that does not vary: NaN error
    seen = {}

    def fake(Xa, Ya, T, f, K, exclude=None, max_comp=0, rule=0, details=False, ctx=None):
        seen.update(T=np.array(T), exclude=np.array(exclude), K=K, f=f)
        pm = Ya[np.asarray(exclude)] + 0.1 * np.arange(P)
        return dict(idx=np.zeros((len(exclude), K), np.uint64), post_mean=pm, ncomp=2)

    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets", fake)
    cv = abcutil.cross_validate_pls(X, Y, n, 10, seed=9, training_fraction=0.4)
    rows = cv["rows"]
    assert len(np.unique(rows)) == n and rows.min() >= 0 and rows.max() < N
    assert np.array_equal(seen["exclude"], rows) and np.array_equal(seen["T"], X[rows]) and seen["K"] == 10
    assert np.array_equal(cv["theta"], Y[rows])
    th = Y[rows]
    expect = ((cv["post_mean"] - th) ** 2).sum(0)[:3] / (n * th.var(axis=0, ddof=1)[:3])
    assert np.allclose(cv["pred_error"][:3], expect, rtol=1e-14)
    assert np.isnan(cv["pred_error"][3])
    again = abcutil.cross_validate_pls(X, Y, n, 10, seed=9)
    assert np.array_equal(again["rows"], rows)


def test_facade_declares_batched_ranking():
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "std::vector<std::vector<size_t>> f(const ABC::Mat2D& X, const ABC::Mat2D& Y, const ABC::Mat2D& T) {\n"
           "  return ABC::particle_ranking_PLS_targets(X, Y, T, 0.5, 10); }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
