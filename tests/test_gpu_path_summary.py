"""Summaries along a tolerance path (abc_rank_targets_path_summary_dev, abc_particle_ranking_pls_targets_path_summary): weighted
quantiles and the CDF at the truth at every tolerance of ONE ranking.  Rejection: bit for bit the summary call with K = K_t and the
NumPy reference of the header's definition, on both sort paths.  Loclinear: one tolerance is the summary call bit for bit; several
tolerances against host values made in long double from the call's own coefficients.  A (target, tolerance) result does not depend
on the list, the batch, the entry point or the outputs asked for; rows past a tolerance never reach it.
Shapes, targets and tolerance lists of test_gpu_path.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _loclinear_ref as LR
import _path_summary_ref as PS
import _summary_ref as R
from test_gpu_path import KS_A, KS_B, _fit, _np, _same, _targets, _with_nc, _wl, fit6, fit_p      # noqa: F401 (fixtures)
from test_gpu_path import _run as _run_path
from test_gpu_summary import _check_bounds, _check_exact, _truth_on_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 0.3, 0.5)
PATH_OUT = ("post_mean", "coef", "rank", "status", "h")


def _run(F, model, T, Ks, method=0, kernel=0, truth=None, exclude=None, probs=PROBS, Y=None, ctx=None, **kw):
    import torch
    from abcsmc_amd import device
    ex = torch.tensor(exclude, dtype=torch.int64) if exclude is not None else None
    tr = torch.tensor(truth, dtype=torch.float64) if truth is not None else None
    return _np(device.rank_targets_path_summary(F["Xd"], model, F["A"], device.colmajor(T, DEV), Ks, F["Yd"] if Y is None else Y,
                                                probs=probs, truth=tr, method=method, kernel=kernel, exclude=ex, ctx=ctx, **kw))


def _summ(F, model, T, K, method=0, kernel=0, truth=None, exclude=None, probs=PROBS, Y=None):
    import torch
    from abcsmc_amd import device
    ex = torch.tensor(exclude, dtype=torch.int64) if exclude is not None else None
    tr = torch.tensor(truth, dtype=torch.float64) if truth is not None else None
    return _np(device.rank_targets_summary(F["Xd"], model, F["A"], device.colmajor(T, DEV), K, F["Yd"] if Y is None else Y,
                                           probs=probs, truth=tr, method=method, kernel=kernel, exclude=ex))


def _truth(F, T, Ks, ex, model=None):
    """truths as test_gpu_summary.py's: a retained row's value for even b (entry 3 of the ranking: inside the tolerances above 3,
    where it counts at half weight, outside the others), another row's otherwise"""
    first = _run_path(F, F["model"] if model is None else model, T, Ks, exclude=ex)
    return _truth_on_rows(F["Y"], first["idx"], F["Y"][np.arange(T.shape[0]) * 11 + 2])


def _rejection_checks(F, T, ex, Ks, truth, g, ref_cols=None):
    """g: the path summary's outputs (method 0).  Every (b, t) against the summary call with K = K_t and against _summary_ref;
    idx, dist and the path's outputs against the plain path call"""
    P = F["Y"].shape[1]
    plain = _run_path(F, F["model"], T, Ks, exclude=ex)
    for k in ("idx", "dist") + PATH_OUT:
        assert _same(g[k], plain[k]), k
    vals = F["Y"][g["idx"].astype(np.int64)]                                   # (B, K_max, P)
    cols = range(P) if ref_cols is None else ref_cols
    for t, K in enumerate(Ks):
        one = _summ(F, F["model"], T, K, truth=truth, exclude=ex)
        assert _same(g["quant"][:, t], one["quant"]) and _same(g["cdf"][:, t], one["cdf"]), K
        _check_exact(vals[:, :K][:, :, cols], None, g["quant"][:, t][:, :, cols], g["cdf"][:, t][:, cols], truth[:, cols])


def test_rejection_bit_exact(fit_p):
    F = fit_p
    T, ex = _targets(F["wl"], F["X"], seed=2)
    for Ks in (KS_A, KS_B):
        truth = _truth(F, T, Ks, ex)
        g = _run(F, F["model"], T, Ks, truth=truth, exclude=ex)
        assert g["quant"].shape == (5, len(Ks), len(PROBS), F["Y"].shape[1]) and g["cdf"].shape == (5, len(Ks), F["Y"].shape[1])
        _rejection_checks(F, T, ex, Ks, truth, g)
        assert 17 not in g["idx"][2] and 5 not in g["idx"][4]


def test_rejection_bit_exact_discrete(gpu_ctx):
    """many ties that straddle the tolerances, and a column of signed zeros (test_gpu_summary.py's rounding)"""
    wl, X, Y = _wl(24, 6, 6001, seed=31)
    Y = np.round(Y * 2.0) / 2.0 - np.round(np.mean(Y, axis=0) * 2.0) / 2.0
    Y[::3, 0] = -0.0
    Y[1::3, 0] = 0.0
    F = _fit(gpu_ctx, X, Y, 8)
    T, ex = _targets(wl, X, seed=9)
    for Ks in (KS_A, KS_B):
        truth = _truth(F, T, Ks, ex)
        truth[1, 0], truth[3, 0] = 0.0, -0.0
        g = _run(F, F["model"], T, Ks, truth=truth, exclude=ex)
        _rejection_checks(F, T, ex, Ks, truth, g)
        vals = Y[g["idx"].astype(np.int64)]
        assert all(np.any(vals[0, K:, 1] == vals[0, K - 1, 1]) for K in Ks[1:-1])      # ties across the cuts


def _loclinear_checks(F, T, g, b, t, K, nc, kernel, truth, cols, probs, tag):
    """(b, t) of a loclinear path summary against host values: theta*_e in long double from the call's own coef[b][t] and the
    reference scores (_loclinear_ref.scores, the reference of test_gpu_adjust.py, which grants theta 1e-9 of the column's range
    against it), weights formed from dist.
    nc = 0: the values are the Y rows themselves: equal weights bit for bit (_check_exact), Epanechnikov by _check_bounds.
    nc > 0: d = 1e-9 x range.  Equal weights: |Q - Q_ref| <= d (order statistics and their interpolation are 1-Lipschitz in the
    values).  Epanechnikov: R.quantile_bound's tolerance + d + the reference's own change under a value perturbation of size d.
    CDF: 4 K_t 2^-53 + the weight share of the entries within d of tau (each may change sides)."""
    X, Y = F["X"], F["Y"]
    idx = g["idx"][b, :K].astype(np.int64)
    dist = g["dist"][b, :K]
    rect = kernel == 1 or bool(g["status"][b, t] & 2)
    if rect:
        w = np.ones(K)
    else:
        tt = dist / dist[K - 1]
        w = 1.0 - tt * tt
    q, c = g["quant"][b, t][None][:, :, cols], g["cdf"][b, t][None][:, cols]
    if nc == 0:
        vals = Y[idx][None][:, :, cols]
        (_check_exact if rect else _check_bounds)(vals, w[None], q, c, truth[b:b + 1][:, cols], probs)
        return
    S = LR.scores(X[idx], F["mean"], F["sd"], F["R"], nc)
    o = LR.scores(T[b], F["mean"], F["sd"], F["R"], nc)[0]
    beta = g["coef"][b, t][1:1 + nc].astype(LR.LD)
    th = (Y[idx].astype(LR.LD) - (S - o).astype(LR.LD) @ beta).astype(np.float64)
    rng_ = Y.max(axis=0) - Y.min(axis=0)
    sign = np.where(np.random.default_rng(b * 100 + t).integers(0, 2, K) == 0, -1.0, 1.0)
    for jj, j in enumerate(cols):
        d = 1e-9 * rng_[j]
        v = th[:, j]
        for qi, lev in enumerate(probs):
            if rect:
                q0, tol = R.summary(v, None, (lev,))[0][0], d
            else:
                q0, tol = R.quantile_bound(v, w, lev, K)
                q1, _ = R.quantile_bound(v + d * sign, w, lev, K)
                tol += d + abs(q1 - q0)
            assert abs(q[0, qi, jj] - q0) <= tol, (tag, b, K, j, lev, q[0, qi, jj], q0, tol)
        u, om = R.sorted_segment(v, w)
        _, W = R.knots(om, R.LD)
        tau = truth[b, j]
        c0 = R.cdf_sorted(u, om, W, tau, R.LD)
        share = float(om[np.abs(u - tau) <= d].sum() / om.sum())
        assert abs(c[0, jj] - c0) <= 4 * K * 2.0 ** -53 + share, (tag, b, K, j, c[0, jj], c0, share)


def test_global_path(gpu_ctx):
    """K_max = 16385 > 8192: chunks, merges and k_smp_eval_global; the tolerances sit on and just past a tile"""
    wl, X, Y = _wl(8, 2, 20000, seed=5)
    F = _fit(gpu_ctx, X, Y, 2)
    F["wl"] = wl
    T = np.ascontiguousarray(np.concatenate([X[[11, 15000]], wl.rows_by_index((1 << 41) + np.arange(1))[0]]))
    ex = [11, 15000, -1]
    Ks = (1, 8192, 8193, 16385)
    truth = _truth(F, T, Ks, ex)
    g = _run(F, F["model"], T, Ks, truth=truth, exclude=ex)
    _rejection_checks(F, T, ex, Ks, truth, g)
    nc = F["ncomp"]
    probs = (0.025, 0.5, 0.975, 1.0)
    for kernel in (0, 1):
        g1 = _run(F, F["model"], T, Ks, method=1, kernel=kernel, truth=truth, exclude=ex, probs=probs)
        plain = _run_path(F, F["model"], T, Ks, exclude=ex, kernel=kernel)
        for k in ("idx", "dist") + PATH_OUT:
            assert _same(g1[k], plain[k]), k
        for b in range(3):
            for t, K in enumerate(Ks):
                _loclinear_checks(F, T, g1, b, t, K, nc, kernel, truth, [0, 1], probs, ("global", kernel))
        one = _summ(F, F["model"], T, Ks[-1], method=1, kernel=kernel, truth=truth, exclude=ex, probs=probs)
        lone = _run(F, F["model"], T, Ks[-1:], method=1, kernel=kernel, truth=truth, exclude=ex, probs=probs)
        assert _same(lone["quant"][:, 0], one["quant"]) and _same(lone["cdf"][:, 0], one["cdf"])


def test_forced_paths_agree(tmp_path):
    """ABC_SUMMARY_PATH=lds / global (ABC_DIAG=1) at K_max = 4097, each in a fresh process: the same bits on both paths, and the
    reference's bits under rejection"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for path in ("lds", "global"):
        out = str(tmp_path / (path + ".npz"))
        p = subprocess.run([sys.executable, os.path.join(root, "tests", "_path_summary_worker.py"), out], capture_output=True,
                           text=True, timeout=600, env=dict(os.environ, ABC_DIAG="1", ABC_SUMMARY_PATH=path), cwd=root)
        assert p.returncode == 0, p.stderr[-3000:]
        res[path] = dict(np.load(out))
    for k in res["lds"]:
        assert _same(res["lds"][k], res["global"][k]), k
    r = res["global"]
    vals = r["Y"][r["idx"].astype(np.int64)]
    Ks = [int(k) for k in r["Ks"]]
    for b in range(vals.shape[0]):
        for j in range(vals.shape[2]):
            q, c = PS.path_summary(vals[b, :, j], Ks, tuple(r["probs"]), r["truth"][b, j])
            assert np.array_equal(r["rej_quant"][b, :, :, j], q) and np.array_equal(r["rej_cdf"][b, :, j], c), (b, j)


@pytest.mark.parametrize("nc", [8, 32])
def test_one_tolerance_is_the_summary_call(fit_p, nc):
    F = fit_p
    T, ex = _targets(F["wl"], F["X"], seed=3)
    model = _with_nc(F, nc)
    truth = F["Y"][np.arange(5) * 7 + 1]
    for K in (1, 7, 1000):
        for kernel in (0, 1):
            g = _run(F, model, T, (K,), method=1, kernel=kernel, truth=truth, exclude=ex)
            one = _summ(F, model, T, K, method=1, kernel=kernel, truth=truth, exclude=ex)
            assert _same(g["idx"], one["idx"]), (nc, K, kernel)
            assert _same(g["quant"][:, 0], one["quant"]) and _same(g["cdf"][:, 0], one["cdf"]), (nc, K, kernel)


@pytest.mark.parametrize("nc", [0, 2, 8])
def test_loclinear_several_tolerances(fit_p, nc):
    F = fit_p
    P = F["Y"].shape[1]
    T, ex = _targets(F["wl"], F["X"], seed=nc)
    model = _with_nc(F, nc)
    cols = sorted({0, P // 2, P - 1})
    probs = (0.025, 0.5, 0.975, 0.3)
    for Ks in (KS_A, KS_B):
        truth = _truth(F, T, Ks, ex, model)
        for kernel in (0, 1):
            g = _run(F, model, T, Ks, method=1, kernel=kernel, truth=truth, exclude=ex, probs=probs)
            plain = _run_path(F, model, T, Ks, exclude=ex, kernel=kernel)
            for k in ("idx", "dist") + PATH_OUT:
                assert _same(g[k], plain[k]), k
            for b in ((0, 3) if Ks[-1] >= 1000 else range(5)):
                for t, K in enumerate(Ks):
                    _loclinear_checks(F, T, g, b, t, K, nc, kernel, truth, cols, probs, (P, nc, Ks[-1], kernel))
            if Ks[0] == 1 and kernel == 0:
                assert np.all(g["status"][:, 0] & 2)                       # K_t = 1: the rectangular fallback, so exact above


def test_invariance(fit6, gpu_ctx):
    """(b, t) does not depend on the other tolerances (given K_max), the batch, the entry point, the outputs asked for, or on
    being the context's first call"""
    from abcsmc_amd import _lib, abcutil
    F = fit6
    fresh_rows, _ = F["wl"].rows_by_index((1 << 42) + np.arange(40))
    T = np.ascontiguousarray(fresh_rows)
    T[5] = F["X"][100]
    truth = F["Y"][np.arange(40) * 3]
    OUT = ("quant", "cdf")
    for method in (0, 1):
        kw = dict(method=method, truth=truth)
        two = _run(F, F["model"], T, (100, 1000), **kw)
        five = _run(F, F["model"], T, (50, 100, 400, 700, 1000), **kw)
        for k in OUT:
            assert _same(five[k][:, 1], two[k][:, 0]) and _same(five[k][:, 4], two[k][:, 1]), (method, k)
        three = _run(F, F["model"], T, (100, 500, 1000), **kw)
        for k in OUT:
            assert _same(three[k][:, 0], two[k][:, 0]) and _same(three[k][:, 2], two[k][:, 1]), (method, k)
        for b in (0, 5, 39):
            one = _run(F, F["model"], np.ascontiguousarray(T[b:b + 1]), (100, 500, 1000), method=method, truth=truth[b:b + 1])
            for k in OUT + ("idx", "dist") + PATH_OUT:
                assert _same(one[k][0], three[k][b]), (method, k, b)
        h = abcutil.particle_ranking_PLS_targets_path_summary(F["X"], F["Y"], T, 0.5, (100, 500, 1000), probs=PROBS, truth=truth,
                                                              method=("rejection", "loclinear")[method], max_comp=8, rule=0,
                                                              ctx=gpu_ctx)
        assert h["ncomp"] == F["ncomp"] and h["quant"].shape == three["quant"].shape
        for k in OUT + ("dist",) + PATH_OUT:
            assert _same(h[k], three[k]), (method, k)
        assert np.array_equal(h["idx"].astype(np.int64), three["idx"])
        bare = dict(post_mean=False, coef=False, fit=False, idx=False, dist=False)
        for extra in ({}, bare):
            qonly = _run(F, F["model"], T, (100, 500, 1000), method=method, **extra)
            conly = _run(F, F["model"], T, (100, 500, 1000), quant=False, **kw, **extra)
            both = _run(F, F["model"], T, (100, 500, 1000), **kw, **extra)
            assert qonly["cdf"] is None and conly["quant"] is None
            assert _same(qonly["quant"], three["quant"]) and _same(conly["cdf"], three["cdf"]), (method, bool(extra))
            assert _same(both["quant"], three["quant"]) and _same(both["cdf"], three["cdf"]), (method, bool(extra))
        fresh = _lib.Context(0)
        try:
            first = _run(F, F["model"], T, (100, 500, 1000), ctx=fresh, **kw)
        finally:
            fresh.close()
        for k in OUT + ("idx", "dist") + PATH_OUT:
            assert _same(first[k], three[k]), (method, k)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_farther_rows_stay_out(fit_p, method, value):
    """a non-finite parameter in the row ranked 300th (between K_0 = 256 and K_1 = 1000) reaches exactly the tolerances past it,
    and only its own column"""
    F = fit_p
    P = F["Y"].shape[1]
    T, ex = _targets(F["wl"], F["X"], seed=4)
    model = _with_nc(F, 8)
    Ks = (256, 1000)
    truth = F["Y"][np.arange(5) * 13 + 4]
    clean = _run(F, model, T, Ks, method=method, truth=truth, exclude=ex)
    r = int(clean["idx"][3, 300])
    Yb = F["Yd"].clone()
    Yb[0, r] = value
    g = _run(F, model, T, Ks, method=method, truth=truth, exclude=ex, Y=Yb)
    assert _same(g["idx"], clean["idx"]) and _same(g["dist"], clean["dist"])
    touched = 0
    for b in range(5):
        at = np.flatnonzero(clean["idx"][b] == r)
        for t, K in enumerate(Ks):
            hit = at.size > 0 and at[0] < K
            touched += hit
            for key in ("quant", "cdf"):
                if not hit:
                    assert _same(g[key][b, t], clean[key][b, t]) and np.all(np.isfinite(g[key][b, t])), (b, K, key)
                else:
                    assert np.all(np.isnan(g[key][b, t][..., 0])), (b, K, key)
                    assert _same(g[key][b, t][..., 1:], clean[key][b, t][..., 1:]), (b, K, key)
                    assert np.all(np.isfinite(g[key][b, t][..., 1:]))
    assert np.flatnonzero(clean["idx"][3] == r)[0] == 300 and touched >= 1
    assert np.all(np.isfinite(g["quant"][3, 0])) and np.all(np.isnan(g["quant"][3, 1][:, 0]))


def test_cross_validate_pls_path_median_and_coverage(gpu_ctx):
    """every tolerance of cross_validate_pls_path(statistic="median", coverage=True) against cross_validate_pls(K = K_t, ...).
    Rejection: post_median, truth_cdf and ci95 bit for bit.  Loclinear: the path's fit (moment chunks of K_max) and the
    adjustment's (chunks of K_t) are each held to 1e-9 of a parameter's range by their references, so with d = 2e-9 x range the
    medians may differ by d plus twice R.quantile_bound's tolerance, truth_cdf by 8 K_t 2^-53 plus the weight share of adjusted
    rows within d of the truth, and ci95 only through truths within d (plus the quantiles' tolerance) of an interval end: their
    count is taken here from the long-double reference on the adjustment's rows, and it is 0 for this seed."""
    from abcsmc_amd import abcutil
    _, X, Y = _wl(8, 4, 20000, seed=1)
    Ks = (100, 400, 1600)
    n = 100
    rng_ = Y.max(axis=0) - Y.min(axis=0)
    base = abcutil.cross_validate_pls_path(X, Y, n, Ks, seed=1, ctx=gpu_ctx)
    assert sorted(base) == sorted(["rows", "theta", "Ks", "post_mean", "pred_error", "best", "idx", "ncomp"])
    for method in ("rejection", "loclinear"):
        plain = abcutil.cross_validate_pls_path(X, Y, n, Ks, seed=1, method=method, ctx=gpu_ctx)
        p = abcutil.cross_validate_pls_path(X, Y, n, Ks, seed=1, method=method, statistic="median", coverage=True, ctx=gpu_ctx)
        assert np.array_equal(p["rows"], plain["rows"]) and np.array_equal(p["idx"], plain["idx"]) and "post_mean" not in p
        assert p["post_median"].shape == (n, 3, 4) and p["truth_cdf"].shape == (n, 3, 4)
        assert p["ci95"].shape == (3, 4) and p["coverage_ks"].shape == (3, 4) and p["best_calibrated"].shape == (4,)
        assert np.array_equal(p["coverage_ks"], abcutil.coverage_ks(p["truth_cdf"]))
        assert np.array_equal(p["best_calibrated"], np.argmin(p["coverage_ks"], axis=0))
        assert np.array_equal(p["best"], np.argmin(p["pred_error"], axis=0))
        var = p["theta"].var(axis=0, ddof=1)
        assert np.allclose(p["pred_error"], ((p["post_median"] - p["theta"][:, None]) ** 2).sum(axis=0) / (n * var), rtol=1e-12)
        for t, K in enumerate(Ks):
            one = abcutil.cross_validate_pls(X, Y, n, K, seed=1, method=method, statistic="median", coverage=True, ctx=gpu_ctx)
            assert np.array_equal(one["rows"], p["rows"]) and np.array_equal(one["idx"], p["idx"][:, :K])
            if method == "rejection":
                assert _same(p["post_median"][:, t], one["post_median"]) and _same(p["truth_cdf"][:, t], one["truth_cdf"])
                assert _same(p["ci95"][t], one["ci95"])
                continue
            a = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[p["rows"]], 0.5, K, exclude=p["rows"], ctx=gpu_ctx)
            d = 2e-9 * rng_
            near = 0
            for b in range(n):
                for j in range(4):
                    v, w, tau = a["theta"][b, :, j], a["weight"][b], p["theta"][b, j]
                    _, tol = R.quantile_bound(v, w, 0.5, K)
                    assert abs(p["post_median"][b, t, j] - one["post_median"][b, j]) <= d[j] + 2 * tol, (K, b, j)
                    share = float(w[np.abs(v - tau) <= d[j]].sum() / w.sum())
                    assert abs(p["truth_cdf"][b, t, j] - one["truth_cdf"][b, j]) <= 8 * K * 2.0 ** -53 + share, (K, b, j)
                    for lev in (0.025, 0.975):
                        q0, tq = R.quantile_bound(v, w, lev, K)
                        near += abs(tau - q0) <= d[j] + tq
            print("loclinear K", K, "truths near an interval end:", near)
            assert near == 0                                                     # (this seed: no truth is that close to an end)
            assert _same(p["ci95"][t], one["ci95"])


def test_bad_arguments(fit6, gpu_ctx):
    """the new refusals (NULL sum; quant and cdf both NULL) and the inherited ones carry the new entries' names"""
    import torch
    from abcsmc_amd import _lib, device
    L = _lib.lib()
    F = fit6
    X, Y = np.asfortranarray(F["X"]), np.asfortranarray(F["Y"])
    N, M = X.shape
    P, B = Y.shape[1], 4
    T = np.asfortranarray(X[:B])
    ks = np.array((10, 20), dtype=np.uint64)
    pr = np.array((0.5, 0.9))
    hq, hc, ht = np.empty(B * 2 * 2 * P), np.empty(B * 2 * P), np.zeros(B * P)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    Xd, Yd, Td, model = F["Xd"], F["Yd"], device.colmajor(T, DEV), F["model"]
    dq, dc, dt = (torch.zeros(v.size, dtype=torch.float64, device=DEV) for v in (hq, hc, ht))
    path = _lib.Path(ks.ctypes.data, 2, None, None, None, None, None)

    def host(sm, pt=path, method=0, kernel=0, mc=3):
        return L.abc_particle_ranking_pls_targets_path_summary(gpu_ctx.handle, p(X), p(Y), N, M, P, p(T), B, 0.5, mc, 0, None, method,
                                                               kernel, None, None, C.byref(pt) if pt is not None else None,
                                                               C.byref(sm) if sm is not None else None, None)

    def dev(sm, pt=path, method=0, kernel=0, mc=8):
        return L.abc_rank_targets_path_summary_dev(gpu_ctx.handle, Xd.data_ptr(), N, Yd.data_ptr(), N, N, M, P, model.data_ptr(), mc,
                                                   Td.data_ptr(), B, B, None, method, kernel, None, None,
                                                   C.byref(pt) if pt is not None else None, C.byref(sm) if sm is not None else None)

    def refused(rc, code, name):
        assert rc == code, (rc, name)
        msg = L.abc_last_error(gpu_ctx.handle)
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert name in msg, msg

    for call, name, q, c, tr in ((host, "abc_particle_ranking_pls_targets_path_summary", p(hq), p(hc), p(ht)),
                                 (dev, "abc_rank_targets_path_summary_dev", dq.data_ptr(), dc.data_ptr(), dt.data_ptr())):
        S = lambda quant=q, cdf=None, truth=None, nq=2, probs=pr: _lib.Summary(probs.ctypes.data, nq, truth, quant, cdf)
        refused(call(None), INVALID, name)                                       # NULL sum
        refused(call(S(quant=None)), INVALID, name)                              # quant and cdf both NULL
        refused(call(S(quant=None, truth=tr)), INVALID, name)                    # ... also with a truth
        refused(call(S(cdf=c)), INVALID, name)                                   # cdf without truth
        refused(call(S(nq=0)), INVALID, name)
        refused(call(S(nq=65)), INVALID, name)
        refused(call(S(probs=np.array((0.5, 1.5)))), INVALID, name)
        refused(call(S(), pt=None), INVALID, name)                               # the path's own
        refused(call(S(), pt=_lib.Path(ks.ctypes.data, 0, None, None, None, None, None)), INVALID, name)
        refused(call(S(), method=2), INVALID, name)
        refused(call(S(), kernel=2), INVALID, name)
        refused(call(S(), mc=65), -4, name)
        gpu_ctx.check(call(S(quant=None, cdf=c, truth=tr)))                      # the CDF alone is a request
        gpu_ctx.check(call(S(cdf=c, truth=tr), method=1))                        # and the context stays usable
    torch.cuda.synchronize()
