"""Local-linear regression adjustment of the batched PLS ranking (abc_rank_targets_adjust_dev,
abc_particle_ranking_pls_targets_adjust): the ranking is unchanged bit for bit, the regression matches the NumPy reference of
the header's definition, every target's result is the same alone and in a batch, and the adjustment improves the estimate."""
import ctypes as C

import numpy as np
import pytest

import _loclinear_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _wl(M, P, N, seed):
    from abcsmc_amd import synthetic
    wl = synthetic.Workload(M, P, seed)
    X, Y = wl.rows(0, N)
    return wl, np.asarray(X), np.asarray(Y)


def _fit(ctx, X, Y, A, rule=0, f=0.5):
    """the fit on the device from the stage entry points; returns the model record and its host parts (mean, sd, R)"""
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
    ctx.check(L.abc_pls_model_dev(ctx.handle, stats.data_ptr(), obs.data_ptr(), M, P, A, rule, model.data_ptr()))
    torch.cuda.synchronize()
    m = model.cpu().numpy()
    off_mean = 4
    off_sd = off_mean + M + P
    off_R = off_sd + M + P + M + A
    return dict(X=X, Y=Y, Xd=Xd, Yd=Yd, model=model, A=A, mean=m[off_mean:off_mean + M], sd=m[off_sd:off_sd + M],
                R=m[off_R:off_R + M * A].reshape(A, M).T.copy(), ncomp=int(m[0]))


def _with_nc(F, nc):
    m = F["model"].clone()
    m[0] = float(nc)
    return m


def _run(F, model, T, K, exclude=None, kernel=0, X=None, Y=None):
    import torch
    from abcsmc_amd import device
    Td = device.colmajor(T, DEV)
    ex = torch.tensor(exclude, dtype=torch.int64) if exclude is not None else None
    r = device.rank_targets_adjust(F["Xd"] if X is None else X, model, F["A"], Td, K, F["Yd"] if Y is None else Y,
                                   exclude=ex, kernel=kernel)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in r.items()}


def _check_ref(F, T, g, b, nc, kernel, tag):
    """coef and theta within 1e-9 of each parameter column's range; where the fit itself is ill-conditioned (fewer rows with
    weight than components: an exact interpolation) the bound is widened to 100x what a relative 1e-15 perturbation of the
    scores changes in the reference.  rank, status and the weights exact."""
    X, Y = F["X"], F["Y"]
    idx = g["idx"][b].astype(np.int64)
    S = R.scores(X[idx], F["mean"], F["sd"], F["R"], nc)
    o = R.scores(T[b], F["mean"], F["sd"], F["R"], nc)[0]
    ref = R.loclinear(g["dist"][b], S, o, Y[idx], kernel=kernel, A=F["A"])
    pert = R.loclinear(g["dist"][b], S * (1.0 + 1e-15 * np.random.default_rng(b).standard_normal(S.shape)), o, Y[idx],
                       kernel=kernel, A=F["A"])
    rng_ = Y.max(axis=0) - Y.min(axis=0)
    assert g["rank"][b] == ref["rank"] and g["status"][b] == ref["status"], (tag, b, g["rank"][b], ref["rank"], g["status"][b])
    assert np.array_equal(g["weight"][b], ref["weight"]), (tag, b)
    for key in ("coef", "theta"):
        sens = np.abs(pert[key] - ref[key]).max(axis=0) if pert["rank"] == ref["rank"] else 0.0
        tol = 1e-9 * rng_ + 100.0 * sens
        err = np.abs(g[key][b] - ref[key])
        assert np.all(err <= tol), (tag, b, key, (err / rng_).max(), (sens / rng_).max())
    assert np.all(g["coef"][b][1 + nc:] == 0.0)


def _targets(wl, X, seed):
    """fresh draws, a row of the set, a copy of that row (then excluded), far outside the cloud, a duplicate of the first"""
    N, M = X.shape
    fresh, _ = wl.rows_by_index((1 << 40) + seed * 1000 + np.arange(5))
    T = np.array(fresh)
    T[1] = X[N // 3]
    T[2] = X[17]
    T[3] = X.mean(axis=0) + 50.0 * X.std(axis=0)
    T[4] = T[0]
    return np.ascontiguousarray(T), [-1, -1, 17, -1, 5]


@pytest.fixture(scope="module", params=[1, 2, 16, 33])
def fit_p(request, gpu_ctx):
    P = request.param
    wl, X, Y = _wl(40, P, 6000, seed=100 + P)
    F = _fit(gpu_ctx, X, Y, 32)
    F["wl"] = wl
    return F


GRID_K = [1, 2, 3, 7, 256, 1000, 4097]


@pytest.mark.parametrize("nc", [0, 1, 2, 8, 16, 32])
def test_against_reference(fit_p, nc):
    F = fit_p
    T, ex = _targets(F["wl"], F["X"], seed=nc)
    model = _with_nc(F, nc)
    for K in GRID_K:
        big = K >= 1000
        if big and nc not in (0, 8, 32):
            continue
        kernel = 1 if K == 256 and nc == 2 else 0
        g = _run(F, model, T, K, exclude=ex, kernel=kernel)
        for b in ((0, 3) if big else range(5)):
            _check_ref(F, T, g, b, nc, kernel, (F["Y"].shape[1], nc, K))
        if K == 1:
            assert np.all(g["status"] & 2) and np.all(g["rank"] == 0)
        if nc == 0:                                     # no components: alpha is the weighted mean, rows unchanged
            assert np.array_equal(g["theta"][0], F["Y"][g["idx"][0].astype(np.int64)])


def test_reference_at_300_targets(gpu_ctx):
    wl, X, Y = _wl(32, 16, 8000, seed=9)
    F = _fit(gpu_ctx, X, Y, 8)
    fresh, _ = wl.rows_by_index((1 << 41) + np.arange(300))
    T = np.ascontiguousarray(fresh)
    ex = [-1] * 300
    ex[7] = 3
    g = _run(F, _with_nc(F, 8), T, 256, exclude=ex)
    assert 3 not in g["idx"][7]
    for b in (0, 7, 150, 299):
        _check_ref(F, T, g, b, 8, 0, "B300")


def test_duplicated_rows_give_h_zero(gpu_ctx):
    wl, X, Y = _wl(12, 3, 3000, seed=4)
    X = np.array(X)
    X[1:60] = X[0]                                     # 60 identical rows, different parameters
    F = _fit(gpu_ctx, np.ascontiguousarray(X), Y, 4)
    T = np.ascontiguousarray(X[[0, 0, 100]])
    for K in (1, 7, 60):
        g = _run(F, _with_nc(F, 4), T, K)
        for b in range(3):
            _check_ref(F, T, g, b, 4, 0, ("dup", K))
        for b in range(2):
            assert set(g["idx"][b].tolist()) <= set(range(60))
            assert g["status"][b] & 2 and g["rank"][b] == 0
            assert np.allclose(g["coef"][b][0], Y[g["idx"][b].astype(np.int64)].mean(axis=0), rtol=1e-13)


def test_ranking_unchanged(gpu_ctx):
    """idx / dist of both new entry points equal the plain batched ranking's, bit for bit, with and without exclusion"""
    import torch
    from abcsmc_amd import abcutil, device
    wl, X, Y = _wl(24, 6, 6001, seed=31)
    T, ex = _targets(wl, X, seed=2)
    for e in (None, ex):
        h = abcutil.particle_ranking_PLS_targets(X, Y, T, 0.5, 40, exclude=e, max_comp=8, rule=0, details=True, ctx=gpu_ctx)
        a = abcutil.particle_ranking_PLS_targets_adjust(X, Y, T, 0.5, 40, exclude=e, max_comp=8, rule=0, ctx=gpu_ctx)
        assert np.array_equal(a["idx"], h["idx"])
        assert np.array_equal(a["dist"].view(np.uint64), h["dist"].view(np.uint64))
        assert a["ncomp"] == h["ncomp"]
    F = _fit(gpu_ctx, X, Y, 8)
    Td = device.colmajor(T, DEV)
    for e in (None, ex):
        et = torch.tensor(e, dtype=torch.int64) if e is not None else None
        idx, d, _ = device.rank_targets(F["Xd"], F["model"], 8, Td, 40, Y=F["Yd"], exclude=et)
        r = device.rank_targets_adjust(F["Xd"], F["model"], 8, Td, 40, F["Yd"], exclude=et)
        torch.cuda.synchronize()
        assert torch.equal(idx, r["idx"]) and torch.equal(d.view(torch.int64), r["dist"].view(torch.int64))


def test_batch_invariance_and_entry_points(gpu_ctx):
    """target b's coef / theta bits: alone (B = 1, rows gathered straight from the scores), inside a batch of 300 (through the
    row-major table), and through the host drop-in"""
    from abcsmc_amd import abcutil
    wl, X, Y = _wl(24, 6, 6001, seed=31)
    F = _fit(gpu_ctx, X, Y, 8, rule=0)
    fresh, _ = wl.rows_by_index((1 << 42) + np.arange(300))
    T = np.ascontiguousarray(fresh)
    T[5] = X[100]
    K = 200
    g = _run(F, F["model"], T, K)
    h = abcutil.particle_ranking_PLS_targets_adjust(X, Y, T, 0.5, K, max_comp=8, rule=0, ctx=gpu_ctx)
    assert h["ncomp"] == F["ncomp"]
    for key in ("idx", "coef", "theta", "weight", "rank", "status"):
        assert np.array_equal(np.asarray(h[key]).view(np.uint8), np.asarray(g[key]).view(np.uint8)), key
    for b in (0, 5, 123, 299):
        one = _run(F, F["model"], np.ascontiguousarray(T[b:b + 1]), K)
        for key in ("idx", "coef", "theta", "weight"):
            assert np.array_equal(one[key][0].view(np.uint8), g[key][b].view(np.uint8)), (key, b)


def test_strided_and_offset_views(gpu_ctx):
    import torch
    wl, X, Y = _wl(24, 6, 6001, seed=31)
    F = _fit(gpu_ctx, X, Y, 8)
    N, M, P = 6001, 24, 6
    T, ex = _targets(wl, X, seed=3)
    ref = _run(F, F["model"], T, 33, exclude=ex)
    big = torch.full((M, N + 7), float("nan"), dtype=torch.float64, device=DEV)
    big[:, 1:N + 1] = F["Xd"]
    ybig = torch.full((P, N + 3), float("nan"), dtype=torch.float64, device=DEV)
    ybig[:, 2:N + 2] = F["Yd"]
    g = _run(F, F["model"], T, 33, exclude=ex, X=big[:, 1:N + 1], Y=ybig[:, 2:N + 2])
    for key in ("idx", "dist", "coef", "theta", "weight", "rank", "status"):
        assert np.array_equal(g[key].view(np.uint8), ref[key].view(np.uint8)), key


def test_loclinear_beats_rejection(gpu_ctx):
    """a linear latent-factor model: the regression adjustment lowers cv4abc's prediction error of every parameter"""
    from abcsmc_amd import abcutil
    _, X, Y = _wl(8, 4, 20000, seed=1)
    rej = abcutil.cross_validate_pls(X, Y, 300, 400, seed=1, ctx=gpu_ctx)
    ll = abcutil.cross_validate_pls(X, Y, 300, 400, seed=1, method="loclinear", ctx=gpu_ctx)
    assert np.array_equal(rej["rows"], ll["rows"])
    assert np.all(ll["pred_error"] < rej["pred_error"]), (ll["pred_error"], rej["pred_error"])
    # the default method keeps the plain batched ranking's posterior means
    raw = abcutil.particle_ranking_PLS_targets(X, Y, X[rej["rows"]], 0.5, 400, exclude=rej["rows"], details=True, ctx=gpu_ctx)
    assert np.array_equal(rej["post_mean"], raw["post_mean"])


def test_bad_arguments(gpu_ctx):
    import torch
    from abcsmc_amd import _lib, device
    L = _lib.lib()
    N, M, P = 500, 6, 3
    _, X, Y = _wl(M, P, N, seed=1)
    X, Y = np.asfortranarray(X), np.asfortranarray(Y)
    T = np.asfortranarray(X[:4])
    idx = np.empty(4 * N, dtype=np.uint64)
    coef = np.empty(4 * 70 * 1100)
    out = _lib.AdjustOut(None, None, coef.ctypes.data, None, None)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def host(B=4, K=10, kernel=0, Ym=Y, o=out, mc=3, Pm=P):
        return L.abc_particle_ranking_pls_targets_adjust(gpu_ctx.handle, p(X), p(Ym), N, M, Pm, p(T), B, 0.5, mc, 0, None, K,
                                                         kernel, p(idx), None, C.byref(o) if o is not None else None, None)

    def refused(rc, code):
        assert rc == code, rc
        assert L.abc_last_error(gpu_ctx.handle)

    INVALID, UNSUPPORTED = -1, -4
    refused(host(kernel=2), INVALID)
    refused(host(kernel=-1), INVALID)
    refused(host(Ym=None), INVALID)
    refused(host(o=None), INVALID)
    refused(host(B=0), INVALID)
    refused(host(K=0), INVALID)
    refused(host(K=N + 1), INVALID)
    refused(host(mc=65), UNSUPPORTED)
    Yw = np.asfortranarray(np.random.default_rng(0).standard_normal((N, 1025)))
    refused(host(Ym=Yw, Pm=1025), UNSUPPORTED)
    Xd, Yd, Td = device.colmajor(X, DEV), device.colmajor(Y, DEV), device.colmajor(T, DEV)
    model = torch.zeros(L.abc_model_len(M, P, 3), dtype=torch.float64, device=DEV)
    ib = torch.empty(4 * 10, dtype=torch.int64, device=DEV)
    dout = _lib.AdjustOut(None, None, None, None, None)

    def dev(ldy=N, Ym=Yd, kernel=0, A=3, o=dout, ldx=N):
        return L.abc_rank_targets_adjust_dev(gpu_ctx.handle, Xd.data_ptr(), ldx, Ym.data_ptr() if Ym is not None else None, ldy,
                                             N, M, P, model.data_ptr(), A, Td.data_ptr(), 4, 4, None, 10, kernel, ib.data_ptr(),
                                             None, C.byref(o) if o is not None else None)

    refused(dev(ldy=N - 1), INVALID)
    refused(dev(Ym=None), INVALID)
    refused(dev(kernel=3), INVALID)
    refused(dev(o=None), INVALID)
    refused(dev(ldx=N - 1), INVALID)
    refused(dev(A=65), UNSUPPORTED)
    refused(dev(kernel=-1), INVALID)
    # what the plain batched ranking refuses (test_gpu_targets.py), on both entries
    U = lambda v: np.array(v, dtype=np.int64).astype(np.uint64)
    Tn, Ti = np.array(T), np.array(T)
    Tn[2, 1], Ti[0, 0] = np.nan, np.inf
    Tn, Ti = np.asfortranarray(Tn), np.asfortranarray(Ti)

    def host2(K=10, ex=None, Xm=X, Tm=T, idx_=idx):
        return L.abc_particle_ranking_pls_targets_adjust(gpu_ctx.handle, p(Xm), p(Y), N, M, P, p(Tm), 4, 0.5, 3, 0, p(ex), K, 0,
                                                         p(idx_), None, C.byref(out), None)

    refused(host2(K=N, ex=U([3, -1, -1, -1])), INVALID)
    refused(host2(ex=U([N, -1, -1, -1])), INVALID)
    refused(host2(Xm=None), INVALID)
    refused(host2(Tm=None), INVALID)
    refused(host2(idx_=None), INVALID)
    refused(host2(Tm=Tn), INVALID)
    refused(host2(Tm=Ti), INVALID)
    dp = lambda t: t.data_ptr() if t is not None else None
    exd = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
    Ywd = device.colmajor(Yw, DEV)

    def dev2(B=4, K=10, ex=None, Xm=Xd, Ym=Yd, Pm=P, tg=Td, idx_=ib, md=model, A=3, ldt=4):
        return L.abc_rank_targets_adjust_dev(gpu_ctx.handle, dp(Xm), N, dp(Ym), N, N, M, Pm, dp(md), A, dp(tg), ldt, B, dp(ex), K, 0,
                                             dp(idx_), None, C.byref(dout))

    refused(dev2(B=0), INVALID)
    refused(dev2(K=0), INVALID)
    refused(dev2(K=N + 1), INVALID)
    refused(dev2(K=N, ex=exd([3, -1, -1, -1])), INVALID)
    refused(dev2(ex=exd([N, -1, -1, -1])), INVALID)
    refused(dev2(Xm=None), INVALID)
    refused(dev2(tg=None), INVALID)
    refused(dev2(idx_=None), INVALID)
    refused(dev2(md=None), INVALID)
    refused(dev2(ldt=3), INVALID)
    refused(dev2(A=0), INVALID)
    refused(dev2(Ym=Ywd, Pm=1025), UNSUPPORTED)
    refused(dev2(tg=device.colmajor(Tn, DEV)), INVALID)
    refused(dev2(tg=device.colmajor(Ti, DEV)), INVALID)
    # the context stays usable
    from abcsmc_amd import abcutil
    a = abcutil.particle_ranking_PLS_targets_adjust(X, Y, T, 0.5, 10, max_comp=3, rule=0, ctx=gpu_ctx)
    h = abcutil.particle_ranking_PLS_targets(X, Y, T, 0.5, 10, max_comp=3, rule=0, ctx=gpu_ctx)
    assert np.array_equal(a["idx"], h)
