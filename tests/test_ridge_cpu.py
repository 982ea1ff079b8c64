"""CPU: the ridge adjustment with the penalty chosen by leave-one-out PRESS (include/abcsmc_hip.h, abc_ctx_set_adjust_ridge).
The NumPy reference (_ridge_ref) is the penalised weighted least-squares fit it claims to be, its PRESS is the brute-force
leave-one-out refit's, lambda = (0,) is the plain fit, an interpolating fit gives +inf and the last index, the new entries are
declared, exported and bound, the wrappers take ridge=, and the choice does what it is for on the reference alone (no GPU
call)."""
import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _loclinear_ref as R
import _ridge_ref as G
from test_loclinear_cpu import ROOT, _header_args

NEW = {"abc_ctx_set_adjust_ridge": 3, "abc_adjust_last_ridge": 8, "abc_adjust_ridge_unscored": 3}
LAMBDAS = (0.0, 1e-3, 1e-2, 1e-1, 1.0)


def _case(K, nc, P, seed, collinear=0.05):
    """K retained rows in ranking order: scores 0 and 1 nearly collinear, parameters linear in the scores plus unit noise"""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((K, nc))
    if nc > 1:
        S[:, 1] = S[:, 0] + collinear * rng.standard_normal(K)
    o = np.full(nc, 0.2)
    d = np.sqrt(((S - o) ** 2).sum(axis=1))
    order = np.argsort(d, kind="stable")
    S, d = S[order], d[order]
    theta = S @ rng.normal(0.0, 1.0, (nc, P)) + rng.standard_normal((K, P))
    return d, S, o, theta


def _penalised_lstsq(w, x, y, lam):
    """the weighted least-squares fit of y on [1, x] with the rows sqrt(lam C_kk) e_k' appended (C the weighted centred moments
    of x): the ridge fit with an unpenalised intercept.  Returns ((1 + nc, P) coefficients, the penalty rows)."""
    K, nc = x.shape
    xc = x - (w[:, None] * x).sum(axis=0) / w.sum()
    ckk = (w[:, None] * xc * xc).sum(axis=0)
    pen = np.hstack([np.zeros((nc, 1)), np.diag(np.sqrt(lam * ckk))])
    sw = np.sqrt(w)[:, None]
    D = np.vstack([np.hstack([np.ones((K, 1)), x]) * sw, pen])
    return np.linalg.lstsq(D, np.vstack([y * sw, np.zeros((nc, y.shape[1]))]), rcond=None)[0], pen


@pytest.mark.parametrize("K,nc,P,kernel", [(16, 4, 3, 0), (40, 12, 2, 0), (300, 8, 4, 1)])
def test_reference_equals_penalised_weighted_least_squares(K, nc, P, kernel):
    d, S, o, theta = _case(K, nc, P, seed=K + nc)
    m = G.moments(d, S, o, theta, kernel)
    for lam, (alpha, beta, _, kept) in zip(LAMBDAS, G.fits(m, LAMBDAS)):
        assert kept.all()
        cf, _ = _penalised_lstsq(m["w"], S - o, theta, lam)
        ref = np.vstack([alpha[None, :], beta]).astype(np.float64)
        assert np.all(np.abs(ref - cf) <= 1e-8 * (1.0 + np.abs(cf).max())), (lam, np.abs(ref - cf).max())


@pytest.mark.parametrize("K,nc", [(16, 4), (40, 12), (300, 8)])
def test_press_equals_the_brute_force_leave_one_out_refit(K, nc):
    """every row of positive weight left out in turn, the fit made again with the penalty matrix held fixed (lam C_kk of ALL
    rows), the left-out row predicted: within 1e-9 relative of the closed form r_e / (1 - h_e)"""
    P = 2
    d, S, o, theta = _case(K, nc, P, seed=7 * K + nc)
    r = G.ridge(d, S, o, theta, LAMBDAS)
    w, x = r["weight"], S - o
    sw = np.sqrt(w)[:, None]
    for l, lam in enumerate(LAMBDAS):
        _, pen = _penalised_lstsq(w, x, theta, lam)
        D = np.hstack([np.ones((K, 1)), x])
        press = np.zeros(P)
        for e in np.flatnonzero(w > 0):
            keep = np.arange(K) != e
            cf = np.linalg.lstsq(np.vstack([(D * sw)[keep], pen]), np.vstack([(theta * sw)[keep], np.zeros((nc, P))]), rcond=None)[0]
            press += w[e] * (theta[e] - D[e] @ cf) ** 2
        assert np.all(np.isfinite(r["press"][l]))
        assert np.all(np.abs(r["press"][l] - press) <= 1e-9 * press), (lam, r["press"][l], press)


@pytest.mark.parametrize("K,nc,P,kernel", [(16, 4, 3, 0), (300, 8, 4, 1), (60, 3, 2, 0)])
def test_lambda_zero_is_the_plain_fit(K, nc, P, kernel):
    d, S, o, theta = _case(K, nc, P, seed=K)
    r, p = G.ridge(d, S, o, theta, (0.0,), kernel=kernel), R.loclinear(d, S, o, theta, kernel=kernel)
    for k in ("coef", "theta", "weight"):
        assert np.array_equal(r[k], p[k]), k
    assert (r["rank"], r["status"]) == (p["rank"], p["status"])
    assert r["pick"].tolist() == [0] * P and r["press"].shape == (1, P) and np.all(np.isinf(r["gap"]))


def test_an_interpolating_fit_is_unscored():
    """K <= nc + 1: the unpenalised fit (1 + nc coefficients) interpolates the rows of positive weight, every leverage is 1, so
    penalty 0 has PRESS +inf; when it is the only penalty the pick is the last index, L - 1 = 0.  A positive penalty keeps every
    leverage below 1 by the definition itself (that is what the penalty is for), so its PRESS stays finite and is picked."""
    for kernel in (0, 1):
        for K, nc in ((9, 8), (8, 8), (5, 4), (4, 4)):
            d, S, o, theta = _case(K, nc, 2, seed=K, collinear=1.0)
            r = G.ridge(d, S, o, theta, (0.0,), kernel=kernel)
            assert np.all(np.isinf(r["press"])) and r["pick"].tolist() == [0, 0], (kernel, K, nc)
            r = G.ridge(d, S, o, theta, LAMBDAS, kernel=kernel)
            assert np.all(np.isinf(r["press"][0])) and np.all(np.isfinite(r["press"][1:])) and np.all(r["pick"] > 0)


def test_abi_entries_declared_exported_and_bound():
    from abcsmc_amd import _lib
    exports = open(os.path.join(ROOT, "abcsmc_amd", "csrc", "exports.map")).read()
    pats = [p.strip() for g in re.findall(r"global:\s*([^;]+);", exports) for p in g.split()]
    for n, nargs in NEW.items():
        assert len(_header_args(n)) == nargs, n
        assert n in _lib.SIGNATURES and len(_lib.SIGNATURES[n][1]) == nargs, n
        assert any(fnmatch.fnmatchcase(n, p) for p in pats), n
    for name in ("set_adjust_ridge", "adjust_ridge", "last_ridge", "adjust_ridge_unscored"):
        assert callable(getattr(_lib.Context, name)), name
    from abcsmc_amd import device
    assert callable(device.adjust_ridge)
    header = open(os.path.join(ROOT, "include", "abcsmc_hip.h")).read()
    assert re.search(r"enum\s*\{\s*ABC_RIDGE_MAXL\s*=\s*8\s*\}", header)


def test_existing_structs_and_products_are_untouched():
    from abcsmc_amd import _lib
    assert [f[0] for f in _lib.AdjustOut._fields_] == ["theta", "weight", "coef", "rank", "status"]
    assert [f[0] for f in _lib.Path._fields_] == ["Ks", "T", "post_mean", "coef", "rank", "status", "h"]
    assert len(_lib.PRODUCTS) == 4


def test_facade_declares_the_setting():
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "void f() {\n"
           "  ABC::set_adjust_ridge(std::vector<double>{0.0, 0.1});\n"
           "  ABC::set_adjust_ridge({});\n"
           "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_ridge_is_accepted_wherever_hcorr_is():
    from abcsmc_amd import abcutil
    seen = 0
    for name, fn in inspect.getmembers(abcutil, inspect.isfunction):
        ps = inspect.signature(fn).parameters
        if "hcorr" in ps and not name.startswith("_"):
            assert "ridge" in ps and ps["ridge"].default is None, name
            seen += 1
    assert seen >= 9
    assert abcutil._ridge_list(0.5) == [0.5] and abcutil._ridge_list((0, 1)) == [0.0, 1.0]


def test_ridge_is_forwarded_only_when_given(monkeypatch):
    from abcsmc_amd import abcutil
    N, M, P, n = 100, 3, 2, 10
    rng = np.random.default_rng(1)
    X, Y = rng.standard_normal((N, M)), rng.standard_normal((N, P))
    seen = {}

    def fake(Xa, Ya, T, f, K, exclude=None, kernel="epanechnikov", max_comp=0, rule=0, theta=True, ctx=None, **kw):
        seen["kw"] = kw
        coef = np.zeros((len(exclude), 3, P))
        return dict(idx=np.zeros((len(exclude), K), np.uint64), coef=coef, post_mean=coef[:, 0] + 1.0, ncomp=1)

    def fake_rej(Xa, Ya, T, f, K, **kw):
        seen["rej"] = kw
        return dict(idx=np.zeros((T.shape[0], K), np.uint64), post_mean=np.zeros((T.shape[0], P)), ncomp=1)

    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets_adjust", fake)
    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets", fake_rej)
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear")
    assert seen["kw"] == {}
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear", ridge=(0, 0.1))
    assert seen["kw"] == {"ridge": (0, 0.1)}
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="rejection", ridge=(0, 0.1))
    assert "ridge" not in seen["rej"]

    def fake_path(Xa, Ya, T, f, Ks, kernel="epanechnikov", exclude=None, max_comp=0, rule=0, ctx=None, **kw):
        seen["path_kw"] = kw
        z = np.zeros((len(exclude), len(Ks), P))
        return dict(post_mean=z, alpha=z + 2.0, Ks=np.asarray(Ks), idx=np.zeros((len(exclude), Ks[-1]), np.uint64), ncomp=1)

    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets_path", fake_path)
    abcutil.cross_validate_pls_path(X, Y, n, (3, 7), seed=4, method="loclinear", ridge=0.5)
    assert seen["path_kw"] == {"ridge": 0.5}


# ---- usefulness ---------------------------------------------------------------------------------------------------------------
USEFUL_K, USEFUL_COMP = 18, 12


def usefulness_data(seed=11, N=3000, M=12, P=12):
    """twelve metrics, two of them nearly collinear, twelve parameters linear in the metrics plus unit noise (so that the PLS fit
    keeps all twelve components); 100 targets.  Returns (X, Y, rows, surface): surface (N, P) the noise-free regression surface"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, M))
    X[:, 1] = X[:, 0] + 0.05 * rng.standard_normal(N)
    surface = X @ rng.normal(0.0, 1.0, (M, P))
    Y = surface + rng.standard_normal((N, P))
    rows = np.sort(np.random.default_rng(3).choice(N, size=100, replace=False)).astype(np.int64)
    return np.ascontiguousarray(X), np.ascontiguousarray(Y), rows, surface


def test_the_choice_beats_the_unpenalised_fit_where_rows_are_few():
    """The usefulness check on the reference alone, through the oracle's PLS fit (it keeps 12 components): each of 100 targets
    excluded from its own ranking, K = 18 nearest rows in score space (1 + 12 coefficients from 18 rows, 17 of positive
    weight).  The rms error of alpha against the noise-free regression surface at the target is smaller with
    ridge = (0, 1e-3, 1e-2, 1e-1, 1) than without, for every parameter.
    Measured: the ratio of the two rms errors is 0.52 to 0.78 over the twelve parameters (at K = 24: 0.77 to 1.01, the effect
    fades as rows are added); the ratio of the squared errors against the noisy truth, what pred_error compares, 0.39 to 0.64."""
    from oracle import pyoracle as O
    X, Y, rows, surface = usefulness_data()
    r = O.particle_ranking_pls(X, Y, X[0], 0.5, max_comp=USEFUL_COMP, rule=0)
    nc = r["ncomp"]
    assert nc == USEFUL_COMP
    S = R.scores(X, r["mean"], r["sd"], r["R"], nc)
    e_plain, e_ridge = [], []
    for b in rows:
        d = np.sqrt(((S - S[b]) ** 2).sum(axis=1))
        d[b] = np.inf
        idx = np.argsort(d, kind="stable")[:USEFUL_K]
        e_plain.append(R.loclinear(d[idx], S[idx], S[b], Y[idx])["coef"][0] - surface[b])
        e_ridge.append(G.ridge(d[idx], S[idx], S[b], Y[idx], LAMBDAS)["coef"][0] - surface[b])
    rms_plain, rms_ridge = np.sqrt((np.array(e_plain) ** 2).mean(axis=0)), np.sqrt((np.array(e_ridge) ** 2).mean(axis=0))
    print("usefulness (reference): rms of alpha with the choice / without", np.round(rms_ridge / rms_plain, 3))
    assert np.all(rms_ridge < rms_plain)
