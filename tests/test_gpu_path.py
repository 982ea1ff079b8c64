"""Tolerance path of the batched PLS ranking (abc_rank_targets_path_dev, abc_particle_ranking_pls_targets_path): one ranking at
K_max, then the rejection mean and the local-linear fit at every tolerance of an ascending list.  Against the long-double reference
of the header's definition (_path_ref.py); the ranking and every prefix of it are the plain ranking's bits; one tolerance is the
adjustment bit for bit; a (target, tolerance) result does not depend on the batch, the entry point or the other tolerances; rows
past a tolerance never reach it.  Sizes of test_gpu_adjust.py: N = 6000, M = 40, its five kinds of target.
This file has not run on a card yet: no MI355X could be had when it was written."""
import ctypes as C

import numpy as np
import pytest

import _loclinear_ref as R
import _path_ref as PR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID, UNSUPPORTED = -1, -4
KS_A = (1, 2, 7, 256, 257, 1000, 4097)      # K_t = 1 (fallback), a chunk edge (256 | 257), 17 chunks at K_max (chunks of 241)
KS_B = (3, 241, 242, 482)                   # cuts on and just past the chunk size of K_max = 482 (two chunks of 241)


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


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in r.items()}


def _run(F, model, T, Ks, exclude=None, kernel=0, Y=None, ctx=None):
    import torch
    from abcsmc_amd import device
    ex = torch.tensor(exclude, dtype=torch.int64) if exclude is not None else None
    return _np(device.rank_targets_path(F["Xd"], model, F["A"], device.colmajor(T, DEV), Ks, F["Yd"] if Y is None else Y,
                                        exclude=ex, kernel=kernel, ctx=ctx))


def _run_adjust(F, model, T, K, exclude=None, kernel=0):
    import torch
    from abcsmc_amd import device
    ex = torch.tensor(exclude, dtype=torch.int64) if exclude is not None else None
    return _np(device.rank_targets_adjust(F["Xd"], model, F["A"], device.colmajor(T, DEV), K, F["Yd"], exclude=ex, kernel=kernel,
                                          theta=False, weight=False))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _check_ref(F, T, g, b, nc, kernel, Ks, tag):
    """rank, status and h exact.  coef by the rule of test_gpu_adjust.py's _check_ref: within 1e-9 of each parameter column's
    range, widened where the fit itself is ill-conditioned (fewer rows with weight than components) to 100x what a relative 1e-15
    perturbation of the scores changes in the reference.  post_mean within 4 K_t 2^-53 max |Y_j| of the long-double mean: the
    bound of two fixed-order fp64 sums of K_t terms (each within K_t 2^-53 sum |y| <= K_t^2 2^-53 max |Y_j|, divided by K_t)."""
    X, Y = F["X"], F["Y"]
    idx = g["idx"][b].astype(np.int64)
    S = R.scores(X[idx], F["mean"], F["sd"], F["R"], nc)
    o = R.scores(T[b], F["mean"], F["sd"], F["R"], nc)[0]
    ref = PR.path(g["dist"][b], S, o, Y[idx], Ks, kernel=kernel, A=F["A"])
    pert = PR.path(g["dist"][b], S * (1.0 + 1e-15 * np.random.default_rng(b).standard_normal(S.shape)), o, Y[idx], Ks,
                   kernel=kernel, A=F["A"])
    rng_ = Y.max(axis=0) - Y.min(axis=0)
    ymax = np.abs(Y).max(axis=0)
    for t, K in enumerate(Ks):
        assert g["rank"][b, t] == ref["rank"][t] and g["status"][b, t] == ref["status"][t], \
            (tag, b, K, g["rank"][b, t], ref["rank"][t], g["status"][b, t], ref["status"][t])
        assert _same(g["h"][b, t], g["dist"][b, K - 1]) and g["h"][b, t] == ref["h"][t], (tag, b, K)
        sens = np.abs(pert["coef"][t] - ref["coef"][t]).max(axis=0) if pert["rank"][t] == ref["rank"][t] else 0.0
        tol = 1e-9 * rng_ + 100.0 * sens
        err = np.abs(g["coef"][b, t] - ref["coef"][t])
        assert np.all(err <= tol), (tag, b, K, "coef", (err / rng_).max(), (np.asarray(sens) / rng_).max())
        assert np.all(g["coef"][b, t][1 + nc:] == 0.0)
        perr = np.abs(g["post_mean"][b, t].astype(np.longdouble) - ref["post_mean"][t]).astype(np.float64)
        assert np.all(perr <= 4.0 * K * 2.0 ** -53 * ymax), (tag, b, K, "post_mean", (perr / ymax).max())


@pytest.fixture(scope="module", params=[1, 16, 33])
def fit_p(request, gpu_ctx):
    P = request.param
    wl, X, Y = _wl(40, P, 6000, seed=100 + P)
    F = _fit(gpu_ctx, X, Y, 32)
    F["wl"] = wl
    return F


@pytest.fixture(scope="module")
def fit6(gpu_ctx):
    """the shapes of test_gpu_adjust.py's batch test: N = 6001, M = 24, P = 6, A = 8, rule 0"""
    wl, X, Y = _wl(24, 6, 6001, seed=31)
    F = _fit(gpu_ctx, X, Y, 8, rule=0)
    F["wl"] = wl
    return F


@pytest.mark.parametrize("nc", [0, 2, 8, 32])
def test_against_reference(fit_p, nc):
    """(nc = 32, every P) are blocks of more than 256 entry groups: k_adj_moments once per tolerance; the others take
    k_adj_moments_path (7 tolerances: passes of 4 and 3 lanes; 4 tolerances: one pass)"""
    F = fit_p
    T, ex = _targets(F["wl"], F["X"], seed=nc)
    model = _with_nc(F, nc)
    for Ks in (KS_A, KS_B):
        for kernel in (0, 1):
            g = _run(F, model, T, Ks, exclude=ex, kernel=kernel)
            for b in ((0, 3) if Ks[-1] >= 1000 else range(5)):
                _check_ref(F, T, g, b, nc, kernel, Ks, (F["Y"].shape[1], nc, Ks[-1], kernel))
            if Ks[0] == 1 and kernel == 0:
                assert np.all(g["status"][:, 0] & 2) and np.all(g["rank"][:, 0] == 0)
            assert 17 not in g["idx"][2] and 5 not in g["idx"][4]


def test_ranking_and_prefixes_are_the_plain_ranking(fit_p):
    import torch
    from abcsmc_amd import device
    F = fit_p
    T, ex = _targets(F["wl"], F["X"], seed=7)
    Td = device.colmajor(T, DEV)
    for e in (None, ex):
        et = torch.tensor(e, dtype=torch.int64) if e is not None else None
        g = _run(F, F["model"], T, KS_A, exclude=e)
        for K in KS_A:
            idx, d, _ = device.rank_targets(F["Xd"], F["model"], F["A"], Td, K, Y=F["Yd"], exclude=et)
            torch.cuda.synchronize()
            assert np.array_equal(g["idx"][:, :K], idx.cpu().numpy()), K
            if K == KS_A[-1]:
                assert _same(g["dist"], d.cpu().numpy())


@pytest.mark.parametrize("nc", [8, 32])
def test_one_tolerance_is_the_adjustment(fit_p, nc):
    F = fit_p
    T, ex = _targets(F["wl"], F["X"], seed=3)
    model = _with_nc(F, nc)
    for K in (1, 7, 1000):
        for kernel in (0, 1):
            g = _run(F, model, T, (K,), exclude=ex, kernel=kernel)
            a = _run_adjust(F, model, T, K, exclude=ex, kernel=kernel)
            assert _same(g["idx"], a["idx"]) and _same(g["dist"], a["dist"])
            assert _same(g["coef"][:, 0], a["coef"]), (nc, K, kernel)
            assert np.array_equal(g["rank"][:, 0], a["rank"]) and np.array_equal(g["status"][:, 0], a["status"])


OUT = ("post_mean", "coef", "rank", "status", "h")


def test_independence_of_list_batch_and_entry(fit6, gpu_ctx):
    from abcsmc_amd import abcutil
    F = fit6
    fresh, _ = F["wl"].rows_by_index((1 << 42) + np.arange(40))
    T = np.ascontiguousarray(fresh)
    T[5] = F["X"][100]
    two = _run(F, F["model"], T, (100, 1000))
    three = _run(F, F["model"], T, (100, 500, 1000))
    for k in OUT:
        assert _same(two[k][:, 0], three[k][:, 0]) and _same(two[k][:, 1], three[k][:, 2]), k
    five = _run(F, F["model"], T, (50, 100, 400, 700, 1000))          # passes of 4 lanes and 1 lane
    for k in OUT:
        assert _same(five[k][:, 1], two[k][:, 0]) and _same(five[k][:, 4], two[k][:, 1]), k
    for b in (0, 5, 39):                                              # alone: rows gathered straight from the scores
        one = _run(F, F["model"], np.ascontiguousarray(T[b:b + 1]), (100, 500, 1000))
        for k in OUT + ("idx", "dist"):
            assert _same(one[k][0], three[k][b]), (k, b)
    h = abcutil.particle_ranking_PLS_targets_path(F["X"], F["Y"], T, 0.5, (100, 500, 1000), max_comp=8, rule=0, ctx=gpu_ctx)
    assert h["ncomp"] == F["ncomp"] and list(h["Ks"]) == [100, 500, 1000]
    for k in OUT + ("idx", "dist"):
        assert _same(h[k], three[k]), k
    assert _same(h["alpha"], three["coef"][:, :, 0])


def test_farther_rows_stay_out(fit_p):
    """a NaN parameter in the row ranked 300th reaches tolerance K_t exactly where 300 < K_t, and only its own column"""
    import torch
    F = fit_p
    P = F["Y"].shape[1]
    T, ex = _targets(F["wl"], F["X"], seed=4)
    model = _with_nc(F, 8)
    Ks = (256, 1000)
    clean = _run(F, model, T, Ks, exclude=ex)
    r = int(clean["idx"][3, 300])
    Yb = F["Yd"].clone()
    Yb[0, r] = float("nan")
    g = _run(F, model, T, Ks, exclude=ex, Y=Yb)
    assert _same(g["idx"], clean["idx"]) and _same(g["dist"], clean["dist"])
    assert np.array_equal(g["rank"], clean["rank"]) and np.array_equal(g["status"], clean["status"]) and _same(g["h"], clean["h"])
    touched = 0
    for b in range(5):
        at = np.flatnonzero(clean["idx"][b] == r)
        for t, K in enumerate(Ks):
            hit = at.size > 0 and at[0] < K
            touched += hit
            for key in ("post_mean", "coef"):
                if not hit:
                    assert _same(g[key][b, t], clean[key][b, t]), (b, K, key)
                    assert np.all(np.isfinite(g[key][b, t]))
                else:
                    col0 = g[key][b, t][:9, 0] if key == "coef" else g[key][b, t][0]      # alpha and the 8 components' beta
                    assert np.all(np.isnan(col0)), (b, K, key)
                    assert _same(g[key][b, t][..., 1:], clean[key][b, t][..., 1:]), (b, K, key)
    assert np.flatnonzero(clean["idx"][3] == r)[0] == 300 and touched >= 1
    assert np.all(np.isfinite(g["coef"][3, 0])) and np.isnan(g["coef"][3, 1, 0, 0])
    if P > 1:
        assert np.all(np.isfinite(g["coef"][3, 1][:, 1:]))


def _host_call(ctx, X, Y, T, Ks, names, kernel=0, mc=8):
    """the host entry through ctypes with only the named output members; returns (rc, outputs)"""
    from abcsmc_amd import _lib
    L = _lib.lib()
    N, M = X.shape
    P, B, nt, A = Y.shape[1], T.shape[0], len(Ks), mc
    Xf, Yf, Tf = np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(T)
    ks = np.array(Ks, dtype=np.uint64)
    shapes = dict(post_mean=((B, nt, P), np.float64), coef=((B, nt, A + 1, P), np.float64), rank=((B, nt), np.int32),
                  status=((B, nt), np.int32), h=((B, nt), np.float64))
    o = {k: np.full(shapes[k][0], -77, dtype=shapes[k][1]) for k in names}
    idx = np.empty((B, int(ks[-1])), dtype=np.uint64)
    path = _lib.Path(ks.ctypes.data, nt, *(o[k].ctypes.data if k in o else None for k in OUT))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.abc_particle_ranking_pls_targets_path(ctx.handle, p(Xf), p(Yf), N, M, P, p(Tf), B, 0.5, mc, 0, None, kernel, p(idx), None,
                                                 C.byref(path), None)
    o["idx"] = idx
    return rc, o


def _dev_call(ctx, F, T, Ks, names, kernel=0):
    import torch
    from abcsmc_amd import _lib, device
    L = _lib.lib()
    M, N = F["Xd"].shape
    P, B, nt, A = F["Yd"].shape[0], T.shape[0], len(Ks), F["A"]
    Td = device.colmajor(T, DEV)
    ks = np.array(Ks, dtype=np.uint64)
    shapes = dict(post_mean=((B, nt, P), torch.float64), coef=((B, nt, A + 1, P), torch.float64), rank=((B, nt), torch.int32),
                  status=((B, nt), torch.int32), h=((B, nt), torch.float64))
    o = {k: torch.full(shapes[k][0], -77, dtype=shapes[k][1], device=DEV) for k in names}
    idx = torch.empty((B, int(ks[-1])), dtype=torch.int64, device=DEV)
    path = _lib.Path(ks.ctypes.data, nt, *(o[k].data_ptr() if k in o else None for k in OUT))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    rc = L.abc_rank_targets_path_dev(ctx.handle, F["Xd"].data_ptr(), N, F["Yd"].data_ptr(), N, N, M, P, F["model"].data_ptr(), A,
                                     Td.data_ptr(), B, B, None, kernel, idx.data_ptr(), None, C.byref(path))
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in o.items()}
    o["idx"] = idx.cpu().numpy()
    return rc, o


def test_each_member_alone_and_first_use(fit6, gpu_ctx):
    """every output member alone (the others NULL, dist NULL) gives the bytes it has in the full request, through both entries;
    the first call on a fresh context has reserved enough on its own"""
    from abcsmc_amd import _lib
    F = fit6
    T, _ = _targets(F["wl"], F["X"], seed=6)
    Ks = (5, 300, 700)
    for call in (lambda c, names: _host_call(c, F["X"], F["Y"], T, Ks, names), lambda c, names: _dev_call(c, F, T, Ks, names)):
        rc, full = call(gpu_ctx, OUT)
        gpu_ctx.check(rc)
        for k in OUT:
            assert not np.any(full[k] == -77), k
            rc, one = call(gpu_ctx, (k,))
            gpu_ctx.check(rc)
            assert _same(one[k], full[k]) and _same(one["idx"], full["idx"]), k
        rc, none = call(gpu_ctx, ())
        gpu_ctx.check(rc)
        assert _same(none["idx"], full["idx"])
        fresh = _lib.Context(0)
        try:
            rc, first = call(fresh, OUT)
            fresh.check(rc)
        finally:
            fresh.close()
        for k in OUT + ("idx",):
            assert _same(first[k], full[k]), k


def test_cross_validate_pls_path(gpu_ctx):
    """pred_error[t] against cross_validate_pls(K = Ks[t]).  Rejection: both means are fixed-order fp64 sums of K_t terms, each
    within K_t 2^-53 max |Y_j| of the exact mean, so they differ by at most d = 2 K_t 2^-53 max |Y_j|.  Loclinear: alpha of the
    path (chunks of K_max) and of the adjustment (chunks of K_t) are held to the reference rule's first term, 1e-9 of the
    parameter's range (K_t >= 100 rows on at most 4 components: the sensitivity term is not needed).  Through the formula,
    |error' - error| <= sum_b (2 |pm - theta| d + d^2) / (n Var), plus the rounding of the n-term sum itself."""
    from abcsmc_amd import abcutil
    _, X, Y = _wl(8, 4, 20000, seed=1)
    Ks = (100, 400, 1600)
    n = 100
    ymax = np.abs(Y).max(axis=0)
    rng_ = Y.max(axis=0) - Y.min(axis=0)
    for method in ("rejection", "loclinear"):
        p = abcutil.cross_validate_pls_path(X, Y, n, Ks, seed=1, method=method, ctx=gpu_ctx)
        assert p["post_mean"].shape == (n, 3, 4) and p["pred_error"].shape == (3, 4) and p["best"].shape == (4,)
        assert np.array_equal(p["best"], np.argmin(p["pred_error"], axis=0))
        var = p["theta"].var(axis=0, ddof=1)
        for t, K in enumerate(Ks):
            one = abcutil.cross_validate_pls(X, Y, n, K, seed=1, method=method, ctx=gpu_ctx)
            assert np.array_equal(one["rows"], p["rows"]) and np.array_equal(one["theta"], p["theta"])
            assert np.array_equal(one["idx"], p["idx"][:, :K])
            d = 2.0 * K * 2.0 ** -53 * ymax if method == "rejection" else 1e-9 * rng_
            diff = np.abs(p["post_mean"][:, t] - one["post_mean"])
            print(method, K, "post_mean diff / bound", (diff / d).max())
            assert np.all(diff <= d), (method, K, (diff / d).max())
            bound = ((2.0 * np.abs(one["post_mean"] - p["theta"]) * d + d * d).sum(axis=0) / (n * var)
                     + 8.0 * n * 2.0 ** -53 * one["pred_error"])
            assert np.all(np.abs(p["pred_error"][t] - one["pred_error"]) <= bound), (method, K)


def test_bad_arguments(fit6, gpu_ctx):
    import torch
    from abcsmc_amd import _lib, device
    L = _lib.lib()
    F = fit6
    X, Y = np.asfortranarray(F["X"]), np.asfortranarray(F["Y"])
    N, M = X.shape
    P, B = Y.shape[1], 4
    T = np.asfortranarray(X[:B])
    idx = np.empty(B * N, dtype=np.uint64)
    coef = np.empty(B * 16 * 70 * P)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    U = lambda v: np.array(v, dtype=np.uint64)

    def desc(Ks, T_=None, null_ks=False):
        ks = U(Ks)
        d = _lib.Path(None if null_ks else ks.ctypes.data, len(Ks) if T_ is None else T_, None, coef.ctypes.data, None, None, None)
        d._keep = ks
        return d

    def host(d, mc=3, ex=None, kernel=0):
        return L.abc_particle_ranking_pls_targets_path(gpu_ctx.handle, p(X), p(Y), N, M, P, p(T), B, 0.5, mc, 0, p(ex), kernel,
                                                       p(idx), None, C.byref(d) if d is not None else None, None)

    Xd, Yd, Td, model = F["Xd"], F["Yd"], device.colmajor(T, DEV), F["model"]
    ib = torch.empty(B * N, dtype=torch.int64, device=DEV)
    cd = torch.empty(B * 16 * 70 * P, dtype=torch.float64, device=DEV)

    def dev(d, A=8, kernel=0):
        if d is not None:
            d = _lib.Path(d.Ks, d.T, None, cd.data_ptr(), None, None, None)
        return L.abc_rank_targets_path_dev(gpu_ctx.handle, Xd.data_ptr(), N, Yd.data_ptr(), N, N, M, P, model.data_ptr(), A,
                                           Td.data_ptr(), B, B, None, kernel, ib.data_ptr(), None,
                                           C.byref(d) if d is not None else None)

    def refused(rc, code, name):
        assert rc == code, (rc, name)
        msg = L.abc_last_error(gpu_ctx.handle)
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert name in msg, msg

    for call, name in ((host, "abc_particle_ranking_pls_targets_path"), (dev, "abc_rank_targets_path_dev")):
        refused(call(None), INVALID, name)
        refused(call(desc((10, 20), null_ks=True)), INVALID, name)
        refused(call(desc((10,), T_=0)), INVALID, name)
        refused(call(desc(tuple(range(1, 18)))), INVALID, name)
        refused(call(desc((10, 10))), INVALID, name)
        refused(call(desc((10, 20, 15))), INVALID, name)
        refused(call(desc((0, 5))), INVALID, name)
        refused(call(desc((10, N + 1))), INVALID, name)
        refused(call(desc((10, 20)), kernel=2), INVALID, name)
    refused(host(desc((10, N)), ex=U([3, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1])), INVALID, "abc_particle_ranking_pls_targets_path")
    refused(host(desc((10, 20)), mc=65), UNSUPPORTED, "abc_particle_ranking_pls_targets_path")
    refused(dev(desc((10, 20)), A=65), UNSUPPORTED, "abc_rank_targets_path_dev")
    # sixteen tolerances are accepted, and the context stays usable
    gpu_ctx.check(host(desc(tuple(range(1, 17)))))
    gpu_ctx.check(dev(desc(tuple(range(5, 21)))))
