"""Weighted posterior quantiles and CDF of the batched ranking (abc_rank_targets_summary_dev,
abc_particle_ranking_pls_targets_summary, abc_weighted_summary*): the device against the NumPy reference of the header's
definition (tests/_summary_ref.py) built on the device's own rows, adjusted values and weights; bit for bit wherever the weights
are equal, within the accuracy contract otherwise; the ranking and adjustment outputs unchanged; batch, entry-point and path
invariance; argument errors; cross-validation with the median and the coverage diagnostic."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _summary_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 0.3, 0.5)


def _wl(M, P, N, seed):
    from abcsmc_amd import synthetic
    wl = synthetic.Workload(M, P, seed)
    X, Y = wl.rows(0, N)
    return np.asarray(X), np.asarray(Y)


def _fit(ctx, X, Y, A, f=0.5):
    import torch
    from abcsmc_amd import _lib, device
    L = _lib.lib()
    N, M = X.shape
    P = Y.shape[1]
    Xd, Yd = device.colmajor(X, DEV), device.colmajor(Y, DEV)
    stats = torch.empty(L.abc_stats_len(M, P), dtype=torch.float64, device=DEV)
    model = torch.empty(L.abc_model_len(M, P, A), dtype=torch.float64, device=DEV)
    obs = torch.zeros(M, dtype=torch.float64, device=DEV)
    ntr = int(np.floor(f * N + 0.5))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(L.abc_stats_shift_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, stats.data_ptr()))
    ctx.check(L.abc_stats_accumulate_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, 0, ntr, stats.data_ptr()))
    ctx.check(L.abc_pls_model_dev(ctx.handle, stats.data_ptr(), obs.data_ptr(), M, P, A, 0, model.data_ptr()))
    torch.cuda.synchronize()
    return dict(Xd=Xd, Yd=Yd, model=model, A=A)


def _np(t):
    return t.cpu().numpy()


def _summ(F, T, K, method=0, kernel=0, truth=None, exclude=None, probs=PROBS, adjust=(), dist=False, Yd=None):
    import torch
    from abcsmc_amd import device
    Td = device.colmajor(T, DEV)
    ex = torch.tensor(exclude, dtype=torch.int64) if exclude is not None else None
    tr = torch.tensor(truth, dtype=torch.float64) if truth is not None else None
    r = device.rank_targets_summary(F["Xd"], F["model"], F["A"], Td, K, F["Yd"] if Yd is None else Yd, probs=probs, truth=tr,
                                    method=method, kernel=kernel, exclude=ex, dist=dist, adjust=adjust)
    torch.cuda.synchronize()
    return {k: (_np(v) if v is not None else None) for k, v in r.items()}


def _check_exact(vals, wts, quant, cdf, truth, probs=PROBS):
    """vals (B, K, P), wts (B, K) or None: every segment's quantiles and CDF bit for bit"""
    B, _, P = vals.shape
    for b in range(B):
        for j in range(P):
            q, c = R.summary(vals[b, :, j], None if wts is None else wts[b], probs, None if truth is None else truth[b, j])
            assert np.array_equal(quant[b, :, j], q, equal_nan=True), (b, j, quant[b, :, j], q)
            if truth is not None:
                assert np.array_equal(cdf[b, j], c, equal_nan=True), (b, j, cdf[b, j], c)


def _check_bounds(vals, wts, quant, cdf, truth, probs=PROBS):
    """unequal weights: quantiles within R.quantile_bound of the long-double reference, CDF within 4 K 2^-53"""
    B, K, P = vals.shape
    for b in range(B):
        for j in range(P):
            v = vals[b, :, j]
            for qi, q in enumerate(probs):
                q0, tol = R.quantile_bound(v, wts[b], q, K)
                assert abs(quant[b, qi, j] - q0) <= tol, (b, j, q, quant[b, qi, j], q0, tol)
            if truth is not None:
                u, om = R.sorted_segment(v, wts[b])
                _, W = R.knots(om, R.LD)
                c0 = R.cdf_sorted(u, om, W, truth[b, j], R.LD)
                assert abs(cdf[b, j] - c0) <= 4 * K * 2.0 ** -53, (b, j, cdf[b, j], c0)


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def _truth_on_rows(Y, idx, T_rows):
    """truth per (b, j): a retained row's value for even b (counts at half weight), a held-out row's otherwise"""
    B = idx.shape[0]
    tr = np.asarray(T_rows, dtype=np.float64).copy()
    for b in range(0, B, 2):
        tr[b] = Y[int(idx[b, min(3, idx.shape[1] - 1)])]
    return tr


@pytest.mark.parametrize("N,M,P,K,B,nq,excl,discrete", [
    (500, 6, 3, 1, 5, 3, False, False),
    (400, 5, 4, 399, 7, 7, True, False),
    (3000, 8, 5, 1000, 20, 7, True, False),
    (2000, 6, 3, 700, 9, 7, False, True),
    (1200, 4, 2, 64, 300, 2, True, False),
])
def test_rejection_bit_exact(ctx, N, M, P, K, B, nq, excl, discrete):
    X, Y = _wl(M, P, N, N + K)
    if discrete:                               # many ties, and signed zeros
        Y = np.round(Y * 2.0) / 2.0 - np.round(np.mean(Y, axis=0) * 2.0) / 2.0
        Y[::3, 0] = -0.0
        Y[1::3, 0] = 0.0
    F = _fit(ctx, X, Y, min(M, P))
    rows = np.arange(B) * 3 % N
    ex = rows if excl else None
    probs = PROBS[:nq]
    first = _summ(F, X[rows], K, exclude=ex, probs=probs)
    truth = _truth_on_rows(Y, first["idx"], Y[rows])
    r = _summ(F, X[rows], K, truth=truth, exclude=ex, probs=probs, dist=True)
    assert np.array_equal(r["idx"], first["idx"])
    from abcsmc_amd import device
    import torch
    Td = device.colmajor(X[rows], DEV)
    exd = torch.tensor(ex, dtype=torch.int64) if ex is not None else None
    idx, dist, _ = device.rank_targets(F["Xd"], F["model"], F["A"], Td, K, Y=F["Yd"], exclude=exd)
    assert np.array_equal(r["idx"], _np(idx)) and np.array_equal(r["dist"], _np(dist))
    vals = Y[r["idx"].astype(np.int64)]                  # (B, K, P)
    _check_exact(vals, None, r["quant"], r["cdf"], truth, probs)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,M,P,K,B", [(2000, 6, 3, 500, 12), (800, 5, 4, 1, 4), (5000, 8, 6, 4097, 3)])
def test_loclinear_against_adjusted_rows(ctx, kernel, N, M, P, K, B):
    from abcsmc_amd import device
    import torch
    X, Y = _wl(M, P, N, 7 * N + K)
    F = _fit(ctx, X, Y, min(M, P))
    rows = np.arange(B) * 5
    Td = device.colmajor(X[rows], DEV)
    a = device.rank_targets_adjust(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], exclude=torch.tensor(rows), kernel=kernel)
    torch.cuda.synchronize()
    a = {k: (_np(v) if v is not None else None) for k, v in a.items()}
    truth = Y[rows].copy()
    truth[0] = a["theta"][0, min(2, K - 1)]                 # a retained adjusted value: counts at half weight
    r = _summ(F, X[rows], K, method=1, kernel=kernel, truth=truth, exclude=rows, dist=True,
              adjust=("theta", "weight", "coef", "rank", "status"))
    for k in ("idx", "dist", "theta", "weight", "coef", "rank", "status"):
        assert np.array_equal(r[k], a[k]), k
    rect = kernel == 1
    for b in range(B):
        wts = a["weight"][b:b + 1]
        rect_b = rect or bool(a["status"][b] & 2)
        if rect_b:
            _check_exact(a["theta"][b:b + 1], wts, r["quant"][b:b + 1], r["cdf"][b:b + 1], truth[b:b + 1])
        else:
            _check_bounds(a["theta"][b:b + 1], wts, r["quant"][b:b + 1], r["cdf"][b:b + 1], truth[b:b + 1])


def test_batch_and_entry_point_invariance(ctx):
    from abcsmc_amd import abcutil
    X, Y = _wl(6, 3, 4000, 21)
    B = 300
    rows = np.arange(B) * 13
    for method in ("rejection", "loclinear"):
        full = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[rows], 0.5, 600, truth=Y[rows], method=method, exclude=rows,
                                                            ctx=ctx)
        for b in (0, 137, 299):
            one = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[rows[b:b + 1]], 0.5, 600, truth=Y[rows[b:b + 1]],
                                                               method=method, exclude=rows[b:b + 1], ctx=ctx)
            assert np.array_equal(one["quant"][0], full["quant"][b]) and np.array_equal(one["cdf"][0], full["cdf"][b])
        again = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[rows], 0.5, 600, truth=Y[rows], method=method, exclude=rows,
                                                             ctx=ctx)
        assert np.array_equal(again["quant"], full["quant"]) and np.array_equal(again["cdf"], full["cdf"])
    # device entry with the host entry's fit: the same bits
    import torch
    from abcsmc_amd import _lib
    L = _lib.lib()
    F = _fit(ctx, X, Y, 3)
    dev = _summ(F, X[rows], 600, method=1, truth=Y[rows], exclude=rows)
    host = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[rows], 0.5, 600, truth=Y[rows], method="loclinear", exclude=rows,
                                                        probs=PROBS, ctx=ctx)
    assert np.array_equal(dev["idx"], host["idx"].astype(np.int64))
    assert np.array_equal(dev["quant"], host["quant"]) and np.array_equal(dev["cdf"], host["cdf"])
    # the generic entry: device and host
    rng = np.random.default_rng(2)
    V = rng.normal(size=(3000, 4))
    w = rng.uniform(0, 1, size=3000)
    h = abcutil.weighted_summary(V, w, probs=PROBS, truth=V[5], ctx=ctx)
    from abcsmc_amd import device
    d = device.weighted_summary(torch.tensor(V.T.copy(), device=DEV), torch.tensor(w), probs=PROBS, truth=torch.tensor(V[5]))
    assert np.array_equal(_np(d["quant"]), h["quant"]) and np.array_equal(_np(d["cdf"]), h["cdf"])
    _check_bounds(V[None], w[None], h["quant"][None], h["cdf"][None], V[5][None])


def test_global_path_large_K(ctx):
    """N = 6e4, K = 5e4: beyond the LDS path; both methods against the reference"""
    from abcsmc_amd import abcutil
    X, Y = _wl(8, 3, 60000, 5)
    rows = np.array([11, 40000])
    r0 = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[rows], 0.5, 50000, truth=Y[rows], exclude=rows, probs=PROBS, ctx=ctx)
    _check_exact(Y[r0["idx"].astype(np.int64)], None, r0["quant"], r0["cdf"], Y[rows])
    a = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[rows], 0.5, 50000, exclude=rows, ctx=ctx)
    r1 = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[rows], 0.5, 50000, truth=Y[rows], exclude=rows, probs=PROBS,
                                                      method="loclinear", ctx=ctx)
    assert np.array_equal(r1["idx"], a["idx"])
    _check_bounds(a["theta"], a["weight"], r1["quant"], r1["cdf"], Y[rows])
    V = np.round(np.random.default_rng(9).normal(size=(20000, 2)), 2)
    g = abcutil.weighted_summary(V, probs=PROBS, truth=V[3], ctx=ctx)
    _check_exact(V[None], None, g["quant"][None], g["cdf"][None], V[3][None])


def test_forced_paths_agree(tmp_path):
    """ABC_SUMMARY_PATH=lds / global (ABC_DIAG=1) at K = 2500 and 4000: the same bits on both paths (the sums' order depends on
    the tile only), and the reference's bits for the equal-weight segments"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for path in ("lds", "global"):
        out = str(tmp_path / (path + ".npz"))
        p = subprocess.run([sys.executable, os.path.join(root, "tests", "_summary_worker.py"), out], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, ABC_DIAG="1", ABC_SUMMARY_PATH=path), cwd=root)
        assert p.returncode == 0, p.stderr[-3000:]
        res[path] = dict(np.load(out))
    for k in res["lds"]:
        assert np.array_equal(res["lds"][k], res["global"][k]), k
    V = np.round(np.random.default_rng(5).normal(size=(4000, 2)), 1)
    probs = (0.025, 0.5, 0.975, 0.1, 0.0, 1.0)
    _check_exact(V[None], None, res["global"]["gen_eq_quant"][None], res["global"]["gen_eq_cdf"][None], V[17][None], probs)


def test_nan_in_one_column(ctx):
    X, Y = _wl(5, 3, 1500, 3)
    Y = Y.copy()
    Y[::50, 1] = np.nan
    F = _fit(ctx, X, Y, 3)
    rows = np.arange(6) * 9
    r = _summ(F, X[rows], 200, truth=Y[rows] * 0 + 1.0, exclude=rows)
    vals = Y[r["idx"].astype(np.int64)]
    for b in range(6):
        has = np.isnan(vals[b, :, 1]).any()
        assert np.isnan(r["quant"][b, :, 1]).all() == has and np.isnan(r["cdf"][b, 1]) == has
        assert np.isfinite(r["quant"][b, :, [0, 2]]).all() and np.isfinite(r["cdf"][b, [0, 2]]).all()
    assert any(np.isnan(vals[b, :, 1]).any() for b in range(6))
    _check_exact(vals, None, r["quant"], r["cdf"], Y[rows] * 0 + 1.0)


def test_argument_errors(ctx):
    import torch
    from abcsmc_amd import _lib, abcutil, device
    X, Y = _wl(5, 3, 800, 4)
    F = _fit(ctx, X, Y, 3)
    T = X[:4]
    with pytest.raises(RuntimeError):
        _summ(F, T, 50, method=2)
    with pytest.raises(RuntimeError):
        _summ(F, T, 50, kernel=3)
    for probs in ((), tuple(np.linspace(0, 1, 65)), (0.5, np.nan), (1.5,), (-0.1,)):
        with pytest.raises(RuntimeError):
            _summ(F, T, 50, probs=probs)
    with pytest.raises(RuntimeError):
        _summ(F, T, 900)                                    # K > N
    L = _lib.lib()
    pr = np.array([0.5])
    q = torch.empty(4 * 3, dtype=torch.float64, device=DEV)
    cdf = torch.empty(4 * 3, dtype=torch.float64, device=DEV)
    s = _lib.Summary(pr.ctypes.data, 1, None, q.data_ptr(), cdf.data_ptr())             # cdf without truth
    Td = device.colmajor(T, DEV)
    rc = L.abc_rank_targets_summary_dev(ctx.handle, F["Xd"].data_ptr(), 800, F["Yd"].data_ptr(), 800, 800, 5, 3,
                                        F["model"].data_ptr(), 3, Td.data_ptr(), 4, 4, None, 50, 0, 0, None, None, None, C.byref(s))
    assert rc == -1                                          # ABC_ERR_INVALID
    s = _lib.Summary(pr.ctypes.data, 1, None, q.data_ptr(), None)
    rc = L.abc_rank_targets_summary_dev(ctx.handle, F["Xd"].data_ptr(), 800, None, 800, 800, 5, 3,
                                        F["model"].data_ptr(), 3, Td.data_ptr(), 4, 4, None, 50, 0, 0, None, None, None, C.byref(s))
    assert rc != 0                                           # Y NULL
    rc = L.abc_rank_targets_summary_dev(ctx.handle, F["Xd"].data_ptr(), 800, F["Yd"].data_ptr(), 800, 800, 5, 3,
                                        F["model"].data_ptr(), 3, Td.data_ptr(), 4, 4, None, 50, 0, 0, None, None, None, None)
    assert rc != 0                                           # sum NULL
    # every refusal of the ranking, the adjustment and the summaries, on the device and the host entry
    INVALID, UNSUPPORTED = -1, -4
    N, M, P = 800, 5, 3
    Xf, Yf, Tf = np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(T)
    Yw = np.asfortranarray(np.random.default_rng(0).standard_normal((N, 1025)))
    Tn, Ti = np.array(T), np.array(T)
    Tn[2, 1], Ti[0, 0] = np.nan, np.inf
    hq, hcdf = np.empty(4 * 65 * 3), np.empty(4 * 3)
    hp = lambda v: v.ctypes.data_as(C.c_void_p) if v is not None else None
    dp = lambda t: t.data_ptr() if t is not None else None
    q65 = torch.empty(4 * 65 * 3, dtype=torch.float64, device=DEV)
    levels, l_high, l_low, l_nan = np.full(65, 0.5), np.array([0.5, 1.5]), np.array([-0.1]), np.array([0.5, np.nan])

    def summary(quant, probs=levels, nq=1, cdf=None):
        return _lib.Summary(probs.ctypes.data if probs is not None else None, nq, None, quant, cdf)

    def host(B=4, K=50, ex=None, Xm=Xf, Ym=Yf, Pm=P, Tm=Tf, mc=3, method=0, kernel=0, sm=summary(hp(hq))):
        return L.abc_particle_ranking_pls_targets_summary(ctx.handle, hp(Xm), hp(Ym), N, M, Pm, hp(Tm), B, 0.5, mc, 0, hp(ex), K,
                                                          method, kernel, None, None, None, C.byref(sm) if sm is not None else None,
                                                          None)

    def dev(B=4, K=50, ex=None, Xm=F["Xd"], Ym=F["Yd"], Pm=P, tg=Td, md=F["model"], A=3, ldx=N, ldy=N, ldt=4, method=0, kernel=0,
            sm=summary(q65.data_ptr())):
        return L.abc_rank_targets_summary_dev(ctx.handle, dp(Xm), ldx, dp(Ym), ldy, N, M, Pm, dp(md), A, dp(tg), ldt, B, dp(ex), K,
                                              method, kernel, None, None, None, C.byref(sm) if sm is not None else None)

    def refused(rc, code):
        assert rc == code, rc
        assert L.abc_last_error(ctx.handle)

    U = lambda v: np.array(v, dtype=np.int64).astype(np.uint64)
    exd = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
    for call, buf, cdfbuf, ex, arr in ((host, hp(hq), hp(hcdf), U, np.asfortranarray),
                                       (dev, q65.data_ptr(), cdf.data_ptr(), exd, lambda t: device.colmajor(t, DEV))):
        for bad in (dict(B=0), dict(K=0), dict(K=N + 1), dict(K=N, ex=ex([3, -1, -1, -1])), dict(ex=ex([N, -1, -1, -1])),
                    dict(Xm=None), dict(Ym=None), dict(method=2), dict(method=-1), dict(kernel=2), dict(kernel=-1), dict(sm=None),
                    dict(sm=summary(buf, nq=0)), dict(sm=summary(buf, nq=65)), dict(sm=summary(buf, probs=None)),
                    dict(sm=summary(buf, probs=l_high, nq=2)), dict(sm=summary(buf, probs=l_low)),
                    dict(sm=summary(buf, probs=l_nan, nq=2)), dict(sm=summary(buf, cdf=cdfbuf))):
            refused(call(**bad), INVALID)
        refused(call(**{"Tm" if call is host else "tg": None}), INVALID)
        refused(call(**{"Tm" if call is host else "tg": arr(Tn)}), INVALID)
        refused(call(**{"Tm" if call is host else "tg": arr(Ti)}), INVALID)
        refused(call(**{"mc" if call is host else "A": 65}), UNSUPPORTED)
    refused(host(Ym=Yw, Pm=1025), UNSUPPORTED)
    refused(dev(Ym=device.colmajor(Yw, DEV), Pm=1025), UNSUPPORTED)
    for bad in (dict(ldx=N - 1), dict(ldy=N - 1), dict(ldt=3), dict(md=None), dict(A=0)):
        refused(dev(**bad), INVALID)
    V = np.random.default_rng(0).normal(size=(100, 2))
    for bad_w in (-np.ones(100), np.zeros(100), np.where(np.arange(100) == 7, np.nan, 1.0), np.where(np.arange(100) == 7, np.inf, 1.0)):
        with pytest.raises(RuntimeError):
            abcutil.weighted_summary(V, bad_w, ctx=ctx)
        with pytest.raises(RuntimeError):
            device.weighted_summary(torch.tensor(V.T.copy(), device=DEV), torch.tensor(bad_w))
    Vd = torch.tensor(V.T.copy(), device=DEV)
    s = _lib.Summary(pr.ctypes.data, 1, None, q.data_ptr(), None)
    for args in ((Vd.data_ptr(), 100, 0, 2), (Vd.data_ptr(), 100, 100, 0), (Vd.data_ptr(), 99, 100, 2), (None, 100, 100, 2)):
        assert L.abc_weighted_summary_dev(ctx.handle, *args, None, C.byref(s)) != 0, args
    with pytest.raises(RuntimeError):
        abcutil.particle_ranking_PLS_targets_summary(X, Y, T, 0.5, 50, method="loclinear", probs=(2.0,), ctx=ctx)
    torch.cuda.synchronize()
    # the context still works after the errors
    r = abcutil.weighted_summary(V, probs=(0.5,), ctx=ctx)
    assert np.array_equal(r["quant"][0], np.array([R.summary(V[:, j], probs=(0.5,))[0][0] for j in range(2)]))


def test_cross_validate_median_and_coverage(ctx):
    """synthetic.Workload(8, 4, 17), N = 20000, 300 left-out rows, K = 400, seed 3.  Observed on an MI355X (the rejection
    medians equal the reference's bits, checked below):
        rejection  ci95 0.990 0.983 0.993 0.993   mean truth_cdf 0.502 0.505 0.484 0.488
        loclinear  ci95 0.937 0.947 0.943 0.960   mean truth_cdf 0.490 0.507 0.468 0.501
    The rejection posterior is wide (it ignores the slope of the parameters in the scores), so it over-covers; the adjusted one is
    close to 0.95.  Bounds: ci95 in [0.90, 1] and the mean truth_cdf within 0.06 of 0.5 (about twice the largest deviation seen;
    its standard error over 300 uniform values is 0.017)."""
    from abcsmc_amd import abcutil
    X, Y = _wl(8, 4, 20000, 17)
    base = abcutil.cross_validate_pls(X, Y, 300, 400, seed=3, ctx=ctx)
    mean = abcutil.cross_validate_pls(X, Y, 300, 400, seed=3, ctx=ctx, statistic="mean")
    assert sorted(base) == sorted(mean)
    for k in base:
        assert np.array_equal(base[k], mean[k], equal_nan=True), k
    for method in ("rejection", "loclinear"):
        med = abcutil.cross_validate_pls(X, Y, 300, 400, seed=3, ctx=ctx, method=method, statistic="median", coverage=True)
        assert np.array_equal(med["rows"], base["rows"])
        if method == "rejection":
            vals = Y[med["idx"].astype(np.int64)]
            ref = np.array([[R.summary(vals[b, :, j], probs=(0.5,))[0][0] for j in range(4)] for b in range(300)])
            assert np.array_equal(med["post_median"], ref)
        var = med["theta"].var(axis=0, ddof=1)
        assert np.allclose(med["pred_error"], ((med["post_median"] - med["theta"]) ** 2).sum(axis=0) / (300 * var), rtol=1e-12)
        print(method, "ci95", med["ci95"], "mean truth_cdf", med["truth_cdf"].mean(axis=0))
        assert med["truth_cdf"].shape == (300, 4) and np.all((0 <= med["truth_cdf"]) & (med["truth_cdf"] <= 1))
        assert np.all((0.90 <= med["ci95"]) & (med["ci95"] <= 1.0)), med["ci95"]
        assert np.all(np.abs(med["truth_cdf"].mean(axis=0) - 0.5) <= 0.06), med["truth_cdf"].mean(axis=0)
    ll = abcutil.cross_validate_pls(X, Y, 300, 400, seed=3, ctx=ctx, method="loclinear", coverage=True)
    assert np.all(np.abs(ll["ci95"] - 0.95) <= 0.04), ll["ci95"]                     # the adjusted posterior is calibrated
