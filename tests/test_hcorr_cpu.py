"""CPU: the heteroscedastic variance correction of the local-linear adjustment (include/abcsmc_hip.h, abc_ctx_set_adjust_hcorr).
The NumPy reference (_hcorr_ref) is the two-stage regression it claims to be, rule 5 skips what it says, the new entries are
declared, exported and bound, the wrappers take hcorr=, and the correction does what it is for on the reference alone (no GPU
call)."""
import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _hcorr_ref as H
import _loclinear_ref as R
from test_loclinear_cpu import ROOT, _header_args

NEW = {"abc_ctx_set_adjust_hcorr": 2, "abc_adjust_last_hcorr": 6, "abc_adjust_hcorr_skipped": 3}


def _case(K, nc, P, seed, gamma=0.6):
    """K retained rows in ranking order: parameters linear in the scores plus noise whose log sd is linear in score 0"""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((K, nc))
    o = np.full(nc, 0.2)
    d = np.sqrt(((S - o) ** 2).sum(axis=1))
    order = np.argsort(d, kind="stable")
    S, d = S[order], d[order]
    theta = S @ rng.normal(0.0, 1.0, (nc, P)) + np.exp(gamma * S[:, :1]) * rng.standard_normal((K, P))
    return d, S, o, theta


def _wlstsq(w, x, y):
    D = np.hstack([np.ones((x.shape[0], 1)), x])
    sw = np.sqrt(w)[:, None]
    return np.linalg.lstsq(D * sw, y * sw, rcond=None)[0]


@pytest.mark.parametrize("K,nc,P,kernel", [(60, 2, 3, 0), (400, 5, 4, 0), (300, 3, 2, 1), (1000, 8, 6, 0)])
def test_reference_equals_two_weighted_least_squares(K, nc, P, kernel):
    d, S, o, theta = _case(K, nc, P, seed=K + nc)
    h = H.hcorr(d, S, o, theta, kernel=kernel)
    assert not h["skipped"].any()
    w, x = h["weight"], S - o
    c1 = _wlstsq(w, x, theta)
    res = theta - np.hstack([np.ones((K, 1)), x]) @ c1
    c2 = _wlstsq(w, x, np.log(res ** 2))
    # the log residuals change by |d r / r|: a bound relative to the smallest residual of the column
    scale = 1e-9 * np.abs(theta).max() / np.abs(res).min(axis=0)
    assert np.all(np.abs(h["hcoef"] - c2) <= np.maximum(1e-9, scale) * (1.0 + np.abs(c2).max(axis=0)))
    corrected = c1[0] + res * np.exp(-0.5 * (x @ c2[1:]))
    span = theta.max(axis=0) - theta.min(axis=0)
    assert np.all(np.abs(h["theta"] - corrected) <= 1e-8 * span)
    assert np.array_equal(h["coef"], R.loclinear(d, S, o, theta, kernel=kernel)["coef"])     # the first fit is untouched
    assert np.array_equal(h["plain"], R.loclinear(d, S, o, theta, kernel=kernel)["theta"])


def test_zero_slopes_leave_alpha_plus_r():
    """scores that carry no variance signal, forced to g == 0 by a rank-deficient design: every pivot of a constant score column
    is skipped, so g == 0 and the corrected rows are alpha + r"""
    d, S, o, theta = _case(200, 2, 3, seed=5)
    S = np.zeros_like(S) + 0.7                                           # constant columns: C == 0, both pivots skipped
    h = H.hcorr(d, S, o, theta)
    assert h["rank"] == 0 and not h["skipped"].any()
    assert np.all(h["hcoef"][1:] == 0.0) and np.all(np.isfinite(h["hcoef"][0]))
    r = h["plain"] - h["coef"][0]
    assert np.array_equal(h["theta"], h["coef"][0] + r)


def test_rule5_constant_column():
    d, S, o, theta = _case(150, 3, 4, seed=7)
    theta[:, 2] = 1.25
    h = H.hcorr(d, S, o, theta)
    assert h["skipped"].tolist() == [False, False, True, False]
    assert np.isnan(h["hcoef"][0, 2]) and np.all(h["hcoef"][1:, 2] == 0.0)
    assert np.all(np.isfinite(h["hcoef"][:, [0, 1, 3]]))
    assert np.array_equal(h["theta"][:, 2], h["plain"][:, 2])
    assert not np.array_equal(h["theta"][:, 0], h["plain"][:, 0])


def test_rule5_duplicated_rows_with_h_zero():
    """identical rows at the observation: h == 0, the rectangular fallback, no pivot kept; two parameter rows repeat so that
    the weighted mean alpha hits one of them exactly in column 1 (a zero residual), column 0 has none"""
    K = 4
    S = np.full((K, 2), 0.3)
    o = np.full(2, 0.3)
    d = np.zeros(K)
    theta = np.array([[0.1, 1.0], [0.7, 3.0], [1.9, 2.0], [2.3, 2.0]])    # column 1: mean 2.0 exactly, rows 2 and 3 equal it
    h = H.hcorr(d, S, o, theta)
    assert h["status"] & 2 and h["rank"] == 0
    assert h["skipped"].tolist() == [True, True]                          # K = 4 <= nc + 2 skips everything
    S5 = np.full((6, 2), 0.3)
    th5 = np.vstack([theta, [[3.1, 1.5], [4.5, 2.5]]])                    # column 1 still averages 2.0
    h = H.hcorr(np.zeros(6), S5, o, th5)
    assert h["skipped"].tolist() == [False, True]
    assert np.array_equal(h["theta"][:, 1], h["plain"][:, 1]) and np.isnan(h["hcoef"][0, 1])
    assert np.all(h["hcoef"][1:] == 0.0)


def test_rule5_k_at_most_nc_plus_two():
    for K, nc, skip in ((5, 3, True), (6, 3, False)):
        d, S, o, theta = _case(K, nc, 2, seed=K)
        h = H.hcorr(d, S, o, theta, kernel=1)
        assert h["skipped"].tolist() == [skip, skip], K
        if skip:
            assert np.array_equal(h["theta"], h["plain"]) and np.isnan(h["hcoef"][0]).all()


def test_rule5_nan_touches_only_its_own_column():
    d, S, o, theta = _case(120, 2, 3, seed=9)
    clean = H.hcorr(d, S, o, theta)
    theta = theta.copy()
    theta[-1, 1] = np.nan                                                # the last row has weight 0: it still counts
    h = H.hcorr(d, S, o, theta)
    assert h["weight"][-1] == 0.0
    assert h["skipped"].tolist() == [False, True, False]
    for j in (0, 2):
        assert np.array_equal(h["theta"][:, j], clean["theta"][:, j])
        assert np.array_equal(h["hcoef"][:, j], clean["hcoef"][:, j])
    assert np.array_equal(h["theta"][:, 1], h["plain"][:, 1], equal_nan=True)


def test_abi_entries_declared_exported_and_bound():
    from abcsmc_amd import _lib
    exports = open(os.path.join(ROOT, "abcsmc_amd", "csrc", "exports.map")).read()
    pats = [p.strip() for g in re.findall(r"global:\s*([^;]+);", exports) for p in g.split()]
    for n, nargs in NEW.items():
        assert len(_header_args(n)) == nargs, n
        assert n in _lib.SIGNATURES and len(_lib.SIGNATURES[n][1]) == nargs, n
        assert any(fnmatch.fnmatchcase(n, p) for p in pats), n
    for name in ("set_adjust_hcorr", "adjust_hcorr", "last_hcorr", "adjust_hcorr_skipped"):
        assert callable(getattr(_lib.Context, name)), name
    from abcsmc_amd import device
    assert callable(device.adjust_hcorr)


def test_existing_structs_and_products_are_untouched():
    from abcsmc_amd import _lib
    assert [f[0] for f in _lib.AdjustOut._fields_] == ["theta", "weight", "coef", "rank", "status"]
    assert [f[0] for f in _lib.Path._fields_] == ["Ks", "T", "post_mean", "coef", "rank", "status", "h"]
    assert len(_lib.PRODUCTS) == 4


def test_facade_declares_the_correction():
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "ABC::Mat2D f() {\n"
           "  ABC::set_adjust_hcorr(true);\n"
           "  ABC::Mat2D h = ABC::last_hcorr();\n"
           "  ABC::set_adjust_hcorr(false);\n"
           "  return h; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_hcorr_is_accepted_wherever_transf_is():
    from abcsmc_amd import abcutil
    seen = 0
    for name, fn in inspect.getmembers(abcutil, inspect.isfunction):
        ps = inspect.signature(fn).parameters
        if "transf" in ps and "bounds" in ps and not name.startswith("_") and name not in ("transform_params", "untransform_params"):
            assert "hcorr" in ps and ps["hcorr"].default is False, name
            seen += 1
    assert seen >= 9


def test_hcorr_is_forwarded_only_when_given(monkeypatch):
    from abcsmc_amd import abcutil
    N, M, P, n = 100, 3, 2, 10
    rng = np.random.default_rng(1)
    X, Y = rng.standard_normal((N, M)), rng.standard_normal((N, P))
    seen = {}

    def fake(Xa, Ya, T, f, K, exclude=None, kernel="epanechnikov", max_comp=0, rule=0, theta=True, ctx=None, **kw):
        seen["kw"] = kw
        coef = np.zeros((len(exclude), 3, P))
        return dict(idx=np.zeros((len(exclude), K), np.uint64), coef=coef, post_mean=coef[:, 0] + 1.0, ncomp=1)

    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets_adjust", fake)
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear")
    assert seen["kw"] == {}
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear", hcorr=True)
    assert seen["kw"] == {"hcorr": True}

    def fake_path(Xa, Ya, T, f, Ks, kernel="epanechnikov", exclude=None, max_comp=0, rule=0, ctx=None, **kw):
        seen["path_kw"] = kw
        z = np.zeros((len(exclude), len(Ks), P))
        return dict(post_mean=z, alpha=z + 2.0, Ks=np.asarray(Ks), idx=np.zeros((len(exclude), Ks[-1]), np.uint64), ncomp=1)

    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets_path", fake_path)
    abcutil.cross_validate_pls_path(X, Y, n, (3, 7), seed=4, method="loclinear", hcorr=True)
    assert seen["path_kw"] == {"hcorr": True}


def usefulness_data(seed=0, N=4000, gamma=0.75):
    """two metrics (x and pure noise), two parameters: 2 x + exp(gamma x) eps (heteroscedastic) and x + eps"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N)
    X = np.stack([x, rng.standard_normal(N)], axis=1)
    Y = np.stack([2.0 * x + np.exp(gamma * x) * rng.standard_normal(N), x + rng.standard_normal(N)], axis=1)
    rows = np.sort(np.random.default_rng(seed + 100).choice(N, 100, replace=False)).astype(np.int64)
    return np.ascontiguousarray(X), np.ascontiguousarray(Y), rows


def weighted_sd(v, w):
    m = (w * v).sum() / w.sum()
    return np.sqrt((w * (v - m) ** 2).sum() / w.sum())


def usefulness_figures(X, rows, theta_on, theta_off, weight, gamma=0.75):
    """(90th percentile of |log(sd / true sd)| of parameter 0 with the correction, the same without, the median relative change
    of parameter 1's sd) over the targets; theta_* (B, K, P), weight (B, K)"""
    on, off, p1 = [], [], []
    for b, row in enumerate(rows):
        true = np.exp(gamma * X[row, 0])
        on.append(abs(np.log(weighted_sd(theta_on[b][:, 0], weight[b]) / true)))
        off.append(abs(np.log(weighted_sd(theta_off[b][:, 0], weight[b]) / true)))
        p1.append(weighted_sd(theta_on[b][:, 1], weight[b]) / weighted_sd(theta_off[b][:, 1], weight[b]))
    return np.percentile(on, 90), np.percentile(off, 90), abs(np.median(p1) - 1.0)


def test_the_correction_recovers_the_local_spread():
    """The usefulness check on the reference alone, through the oracle's PLS fit and ranking: 100 targets taken from the 4000
    rows and excluded from their own ranking, K = 2000, Epanechnikov weights.  The 90th percentile over targets of
    |log(weighted sd of the adjusted rows of parameter 0 / exp(0.75 x_target))| must be <= 0.1 with the correction and >= 0.3
    without; parameter 1 (homoscedastic) changes its sd by less than 10 % at the median.
    The reference gives 0.055 with, 0.500 without and 0.000 for parameter 1 (seeds 1 and 2: 0.067 / 0.769 and 0.066 / 0.646)."""
    from oracle import pyoracle as O
    X, Y, rows = usefulness_data()
    K = 2000
    on, off, wt = [], [], []
    for b in rows:
        r = O.particle_ranking_pls(X, Y, X[b], 0.5, max_comp=2, rule=0)
        nc = r["ncomp"]
        idx = r["idx"].astype(np.int64)
        idx = idx[idx != b][:K]
        S = R.scores(X[idx], r["mean"], r["sd"], r["R"], nc)
        o = R.scores(X[b], r["mean"], r["sd"], r["R"], nc)[0]
        d = np.sqrt(((S - o) ** 2).sum(axis=1))
        h = H.hcorr(d, S, o, Y[idx])
        assert not h["skipped"].any()
        on.append(h["theta"]); off.append(h["plain"]); wt.append(h["weight"])
    f_on, f_off, f_p1 = usefulness_figures(X, rows, on, off, wt)
    print("usefulness (reference): with %.3f without %.3f parameter 1 %.4f" % (f_on, f_off, f_p1))
    assert f_on <= 0.1 and f_off >= 0.3 and f_p1 < 0.1
