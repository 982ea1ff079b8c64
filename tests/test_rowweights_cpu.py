"""CPU: row importance weights of the batched ranking (include/abcsmc_hip.h, abc_ctx_set_row_weights).  The wrapped references
(_rowweights_ref) with unit weights are the existing references bit for bit; integer weights equal row repetition, which pins the
semantics independently of the wrapper; the all-zero rule; the new entries are declared, exported and bound and the wrappers take
row_weights=; and the weights remove the design bias on the references alone (no GPU call)."""
import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _hcorr_ref as H
import _loclinear_ref as R
import _path_ref as PT
import _ridge_ref as G
import _rowweights_ref as RW
from test_loclinear_cpu import ROOT, _header_args
from test_ridge_cpu import LAMBDAS, _case

NEW = {"abc_ctx_set_row_weights": 3, "abc_ctx_set_row_weights_dev": 3, "abc_row_weights_info": 4}


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same_dict(a, b):
    assert set(a) == set(b)
    for k in a:
        assert _same(np.asarray(a[k]), np.asarray(b[k])), k


# ---- unit weights --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("K,nc,P", [(40, 3, 2), (257, 4, 5), (9, 8, 3)])
def test_unit_weights_are_the_existing_references_bit_for_bit(K, nc, P, kernel):
    d, S, o, theta = _case(K, nc, P, 3 * K + nc)
    one = np.ones(K)
    _same_dict(RW.loclinear(d, S, o, theta, one, kernel=kernel), R.loclinear(d, S, o, theta, kernel=kernel))
    _same_dict(RW.ridge(d, S, o, theta, one, LAMBDAS, kernel=kernel), G.ridge(d, S, o, theta, LAMBDAS, kernel=kernel))
    _same_dict(RW.hcorr(d, S, o, theta, one, kernel=kernel), H.hcorr(d, S, o, theta, kernel=kernel))
    Ks = tuple(sorted({nc + 1, (nc + 1 + K) // 2, K}))
    a, b = RW.path(d, S, o, theta, one, Ks, kernel=kernel), PT.path(d, S, o, theta, Ks, kernel=kernel)
    for k in ("coef", "rank", "status", "h"):
        assert _same(a[k], b[k]), k
    assert np.all(np.abs(a["post_mean"] - b["post_mean"]) <= 4 * np.finfo(np.longdouble).eps * np.abs(b["post_mean"]).max())
    assert R.weights is not None and R.weights.__module__ == "_loclinear_ref"       # the wrapper restored the function


def test_the_wrapper_multiplies_and_keeps_the_fallback_rule():
    d = np.array([0.0, 1.0, 2.0, 4.0])
    om = np.array([2.0, 0.0, 3.0, 5.0])
    w, fb = RW.weights(d, om)
    assert not fb and np.array_equal(w, (1.0 - (d / 4.0) ** 2) * om)
    w, fb = RW.weights(np.array([3.0, 3.0, 3.0]), om[:3])            # every Epanechnikov weight 0: the fallback, distances only
    assert fb and np.array_equal(w, om[:3])
    w, fb = RW.weights(d, om, kernel=1)
    assert not fb and np.array_equal(w, om)


# ---- integer weights equal row repetition --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,nc,P,seed", [(60, 3, 2, 1), (200, 4, 5, 2), (33, 2, 1, 3)])
def test_integer_weights_equal_row_repetition(K, nc, P, seed):
    """rectangular kernel: the wrapped reference on K rows with omega in {0, 1, 2, 3} against the unwrapped reference on the table
    in which row e appears omega_e times; coef within 1e-12 of each parameter's range"""
    d, S, o, theta = _case(K, nc, P, seed, collinear=0.5)
    om = np.random.default_rng(seed).integers(0, 4, K).astype(np.float64)
    om[0] = 0.0                                                   # the shift row itself has weight 0
    rep = np.repeat(np.arange(K), om.astype(np.int64))
    span = theta.max(axis=0) - theta.min(axis=0)
    a = RW.loclinear(d, S, o, theta, om, kernel=1)
    b = R.loclinear(d[rep], S[rep], o, theta[rep], kernel=1)
    assert a["rank"] == b["rank"] == nc and a["status"] == b["status"] == 0
    err = np.abs(a["coef"] - b["coef"]).max(axis=0)
    print("repetition: err/range", (err / span).max())
    assert np.all(err <= 1e-12 * span)
    on = om > 0
    assert np.all(np.abs(a["theta"][on] - b["theta"][np.searchsorted(rep, np.flatnonzero(on))]) <= 1e-12 * span)
    # the weighted rejection mean is the repeated table's mean
    pm = RW.post_mean(theta, om)
    assert np.all(np.abs(pm - theta[rep].astype(np.longdouble).mean(axis=0)) <= 1e-15 * span)
    # and under ridge the same penalised fits
    ar = RW.ridge(d, S, o, theta, om, (0.5,), kernel=1)
    br = G.ridge(d[rep], S[rep], o, theta[rep], (0.5,), kernel=1)
    assert np.all(np.abs(ar["coef"] - br["coef"]).max(axis=0) <= 1e-12 * span)


# ---- the all-zero rule ---------------------------------------------------------------------------------------------------------
def test_all_zero_rule():
    K, nc, P, A = 12, 3, 2, 5
    d, S, o, theta = _case(K, nc, P, 4)
    z = np.zeros(K)
    r = RW.loclinear(d, S, o, theta, z, A=A)
    assert r["rank"] == 0 and r["status"] == 5 and np.all(r["weight"] == 0.0) and np.all(np.isnan(r["theta"]))
    assert np.all(np.isnan(r["coef"][:1 + nc])) and np.all(r["coef"][1 + nc:] == 0.0) and r["coef"].shape == (A + 1, P)
    assert RW.loclinear(np.full(K, 2.0), S, o, theta, z, A=A)["status"] == 7         # with the fallback's bit
    g = RW.ridge(d, S, o, theta, z, LAMBDAS, A=A)
    assert np.all(g["pick"] == len(LAMBDAS) - 1) and np.all(np.isinf(g["press"])) and np.all(np.isnan(g["coef"][0]))
    h = RW.hcorr(d, S, o, theta, z, A=A)
    assert np.all(h["skipped"]) and np.all(np.isnan(h["hcoef"][0])) and np.all(h["hcoef"][1:] == 0.0)
    assert np.all(np.isnan(RW.post_mean(theta, z)))
    # Epanechnikov: the last row has k_e = 0, so a single positive row weight there is still an all-zero slot
    last = z.copy()
    last[-1] = 1.0
    assert RW.loclinear(d, S, o, theta, last, A=A)["status"] & 4
    p = RW.path(d, S, o, theta, np.r_[np.zeros(6), np.ones(6)], (5, 12), A=A)
    assert p["status"][0] & 4 and not p["status"][1] & 4 and np.all(np.isnan(p["post_mean"][0])) and np.all(np.isfinite(p["post_mean"][1]))
    # a zero-weight row is an ordinary row: the fit is the fit without it (rectangular kernel, up to rounding)
    om = np.ones(K)
    om[5] = 0.0
    keep = om > 0
    a, b = RW.loclinear(d, S, o, theta, om, kernel=1), R.loclinear(d[keep], S[keep], o, theta[keep], kernel=1)
    assert np.allclose(a["coef"], b["coef"], rtol=0, atol=1e-12)


# ---- declarations and wrappers -------------------------------------------------------------------------------------------------
def test_abi_entries_declared_exported_and_bound():
    from abcsmc_amd import _lib, device
    exports = open(os.path.join(ROOT, "abcsmc_amd", "csrc", "exports.map")).read()
    pats = [p.strip() for g in re.findall(r"global:\s*([^;]+);", exports) for p in g.split()]
    for n, nargs in NEW.items():
        assert len(_header_args(n)) == nargs, n
        assert n in _lib.SIGNATURES and len(_lib.SIGNATURES[n][1]) == nargs, n
        assert any(fnmatch.fnmatchcase(n, p) for p in pats), n
    for name in ("set_row_weights", "row_weights", "row_weights_info"):
        assert callable(getattr(_lib.Context, name)), name
    assert callable(device.row_weights)
    assert [f[0] for f in _lib.AdjustOut._fields_] == ["theta", "weight", "coef", "rank", "status"]


def test_facade_declares_the_setting():
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "void f() {\n"
           "  ABC::set_row_weights(std::vector<double>{1.0, 0.5});\n"
           "  ABC::clear_row_weights();\n"
           "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "set_row_weights" in open(os.path.join(ROOT, "abcsmc_amd", "cxx", "facade_demo.cpp")).read()


def test_row_weights_is_accepted_by_every_targets_wrapper():
    from abcsmc_amd import abcutil
    seen = 0
    for name, fn in inspect.getmembers(abcutil, inspect.isfunction):
        if name.startswith("particle_ranking_PLS_targets") or name in ("cross_validate_pls", "cross_validate_pls_path"):
            ps = inspect.signature(fn).parameters
            assert "row_weights" in ps and ps["row_weights"].default is None, name
            seen += 1
    assert seen == 10
    assert "weight_predictive_prior" in abcutil.particle_ranking_PLS_targets.__doc__


def test_row_weights_is_forwarded_only_when_given(monkeypatch):
    from abcsmc_amd import abcutil
    N, M, P, n = 100, 3, 2, 10
    rng = np.random.default_rng(1)
    X, Y, om = rng.standard_normal((N, M)), rng.standard_normal((N, P)), rng.uniform(size=N)
    seen = {}

    def fake(Xa, Ya, T, f, K, exclude=None, kernel="epanechnikov", max_comp=0, rule=0, theta=True, ctx=None, **kw):
        seen["adj"] = kw
        coef = np.zeros((len(exclude), 3, P))
        return dict(idx=np.zeros((len(exclude), K), np.uint64), coef=coef, post_mean=coef[:, 0] + 1.0, ncomp=1)

    def fake_rej(Xa, Ya, T, f, K, **kw):
        seen["rej"] = kw
        return dict(idx=np.zeros((T.shape[0], K), np.uint64), post_mean=np.zeros((T.shape[0], P)), ncomp=1)

    def fake_path(Xa, Ya, T, f, Ks, kernel="epanechnikov", exclude=None, max_comp=0, rule=0, ctx=None, **kw):
        seen["path"] = kw
        z = np.zeros((len(exclude), len(Ks), P))
        return dict(post_mean=z, alpha=z + 2.0, Ks=np.asarray(Ks), idx=np.zeros((len(exclude), Ks[-1]), np.uint64), ncomp=1)

    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets_adjust", fake)
    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets", fake_rej)
    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets_path", fake_path)
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear")
    assert seen["adj"] == {}
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear", row_weights=om)
    assert list(seen["adj"]) == ["row_weights"] and seen["adj"]["row_weights"] is om
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="rejection")
    assert "row_weights" not in seen["rej"]
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="rejection", row_weights=om)     # both methods take them
    assert seen["rej"]["row_weights"] is om
    abcutil.cross_validate_pls_path(X, Y, n, (3, 7), seed=4, method="rejection", row_weights=om)
    assert seen["path"]["row_weights"] is om


# ---- the bias example on the references alone --------------------------------------------------------------------------------------
BIAS_SEED, BIAS_K = 20261019, 1000


def bias_example(seed, N=20000, n_targets=40):
    """the issue's example: a U(0, 1) prior, four metrics theta + 0.5 eps, the table's rows drawn from the density 0.5 + theta
    (omega = prior / design = 1 / (0.5 + theta)), and a table of the same size drawn from the prior to compare with"""
    rng = np.random.default_rng(seed)
    theta = -0.5 + np.sqrt(0.25 + 2.0 * rng.uniform(size=N))      # the inverse of F(t) = t / 2 + t^2 / 2
    theta_prior = rng.uniform(size=N)
    X = theta[:, None] + 0.5 * rng.standard_normal((N, 4))
    X_prior = theta_prior[:, None] + 0.5 * rng.standard_normal((N, 4))
    truth = rng.uniform(size=n_targets)
    targets = truth[:, None] + 0.5 * rng.standard_normal((n_targets, 4))
    return dict(theta=theta, theta_prior=theta_prior, X=np.ascontiguousarray(X), X_prior=np.ascontiguousarray(X_prior),
                targets=np.ascontiguousarray(targets), omega=1.0 / (0.5 + theta))


def _rejection_means(X, theta, targets, K, omega=None):
    out = np.empty(targets.shape[0])
    for b, t in enumerate(targets):
        idx = np.argsort(((X - t) ** 2).sum(axis=1), kind="stable")[:K]
        out[b] = float(RW.post_mean(theta[idx, None], np.ones(K) if omega is None else omega[idx])[0])
    return out


def test_the_weights_remove_the_design_bias():
    """raw Euclidean distance on the metrics, K = 1000 of N = 20 000, 40 targets: the weighted mean bias over the targets is at
    most a quarter of the unweighted one (measured over eight seeds: 0.002 to 0.0045 against 0.042 to 0.051)"""
    e = bias_example(BIAS_SEED)
    prior = _rejection_means(e["X_prior"], e["theta_prior"], e["targets"], BIAS_K)
    unw = _rejection_means(e["X"], e["theta"], e["targets"], BIAS_K)
    wtd = _rejection_means(e["X"], e["theta"], e["targets"], BIAS_K, e["omega"])
    bu, bw = abs(float((unw - prior).mean())), abs(float((wtd - prior).mean()))
    print("bias example (reference): unweighted %.4f, weighted %.4f" % (bu, bw))
    assert bw <= 0.25 * bu, (bu, bw)
