"""Weighted posterior densities and modes of the batched ranking (abc_rank_targets_density_dev,
abc_particle_ranking_pls_targets_density, abc_weighted_density*): the device against the NumPy reference of the header's definition
(tests/_density_ref.py) built on the device's own rows, adjusted values and weights.  Every case checks the bandwidth within
bw_bound, the grid exactly from the device's bandwidth, the density at the device's bandwidth and grid within the accuracy
contract, and the mode as the first largest value of the device's own density.  Then batch, entry-point, repeat and dens-or-not
invariance, the ranking and adjustment outputs unchanged, argument errors and cross-validation with the mode.

DN_TILE = 1024 entries is the density kernel's LDS tile and DN_GC = 512 grid points its work-group's chunk (density.hip);
8192 is the largest K of the summaries' LDS path."""
import ctypes as C

import numpy as np
import pytest

import _density_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {"rel": 0.0}                       # largest |f_dev - f_ref| / f_ref seen where f_ref >= 1e-280 max f_ref


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


def _dens(F, T, K, exclude=None, **kw):
    import torch
    from abcsmc_amd import device
    Td = device.colmajor(T, DEV)
    ex = torch.tensor(exclude, dtype=torch.int64) if exclude is not None else None
    r = device.rank_targets_density(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], exclude=ex, **kw)
    torch.cuda.synchronize()
    return {k: (_np(v) if v is not None else None) for k, v in r.items()}


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def _check_segment(v, w, out, seg, G, cut=3.0, bw_scale=1.0, bw=None):
    """one segment of the device's outputs (out[name][seg]) against the reference"""
    v = np.asarray(v, dtype=np.float64)
    h, lo_x, step = out["bw"][seg], out["grid"][seg][0], out["grid"][seg][1]
    dens, mode, md = out["dens"][seg], out["mode"][seg], out["mode_dens"][seg]
    if not np.all(np.isfinite(v)):
        assert np.isnan(h) and np.isnan(lo_x) and np.isnan(step) and np.isnan(mode) and np.isnan(md) and np.isnan(dens).all(), seg
        return
    if bw is not None:
        assert h == bw, (seg, h, bw)
    else:
        h_ref, tol = D.bw_bound(v, w, bw_scale)
        assert abs(h - h_ref) <= tol, (seg, h, h_ref, tol)
    u, _ = D.positive(v, w)
    assert (lo_x, step) == D.grid(u.min(), u.max(), h, cut, G), (seg, lo_x, step)
    x = D.grid_points(lo_x, step, G)
    f_ref = D.density_at(v, w, x, h)
    err = np.abs(dens.astype(D.LD) - f_ref)
    big = f_ref >= 1e-280 * f_ref.max()
    WORST["rel"] = max(WORST["rel"], float((err[big] / f_ref[big]).max()))
    assert np.all(err <= D.density_bound(f_ref)), (seg, float((err[big] / f_ref[big]).max()))
    g = int(np.argmax(dens))                                   # the first on ties
    assert mode == x[g] and md == dens[g], (seg, mode, x[g], md, dens[g])
    assert D.density_at(v, w, x[g:g + 1], h)[0] >= (1 - 2e-6) * f_ref.max(), seg


def _check_all(vals, wts, out, G, **kw):
    """vals (B, K, P), wts (B, K) or None, out: the device's arrays shaped (B, P, ...)"""
    B, _, P = vals.shape
    bw = kw.pop("bw", None)
    for b in range(B):
        for j in range(P):
            _check_segment(vals[b, :, j], None if wts is None else wts[b], out, (b, j), G,
                           bw=None if bw is None else np.broadcast_to(bw, (B, P))[b, j], **kw)


@pytest.mark.parametrize("N,M,P,K,B,G,excl", [
    (500, 6, 3, 1, 5, 64, False),
    (400, 5, 1, 2, 4, 2, True),
    (600, 5, 3, 63, 3, 63, True),
    (900, 6, 17, 257, 1, 65, False),
    (3000, 8, 3, 1000, 20, 65, True),
    (3000, 8, 3, 1000, 2, 512, False),
    (3000, 5, 2, 1025, 2, 4096, False),                         # one entry past the LDS tile; eight grid chunks
    (9000, 6, 2, 8193, 2, 64, True),                            # past the summaries' LDS path
])
def test_rejection(ctx, N, M, P, K, B, G, excl):
    import torch
    from abcsmc_amd import device
    X, Y = _wl(M, P, N, N + K)
    F = _fit(ctx, X, Y, min(M, P))
    rows = np.arange(B) * 3 % N
    ex = rows if excl else None
    r = _dens(F, X[rows], K, exclude=ex, G=G, dist=True)
    Td = torch.empty((M, B), dtype=torch.float64, device=DEV)          # (unit stride also with one target)
    Td.copy_(torch.tensor(X[rows]).T)
    exd = torch.tensor(ex, dtype=torch.int64) if ex is not None else None
    idx, dist, _ = device.rank_targets(F["Xd"], F["model"], F["A"], Td, K, Y=F["Yd"], exclude=exd)
    assert np.array_equal(r["idx"], _np(idx)) and np.array_equal(r["dist"], _np(dist))
    _check_all(Y[r["idx"]], None, r, G)
    print("worst relative density error so far", WORST["rel"])


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,M,P,K,B,G", [(2000, 6, 3, 500, 12, 512), (800, 5, 4, 1, 4, 65), (9000, 6, 2, 8193, 2, 63)])
def test_loclinear_against_adjusted_rows(ctx, kernel, N, M, P, K, B, G):
    """Epanechnikov: unequal weights and the weight-0 last row; rectangular; K = 1: the rectangular fallback"""
    import torch
    from abcsmc_amd import device
    X, Y = _wl(M, P, N, 7 * N + K)
    F = _fit(ctx, X, Y, min(M, P))
    rows = np.arange(B) * 5
    Td = device.colmajor(X[rows], DEV)
    a = device.rank_targets_adjust(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], exclude=torch.tensor(rows), kernel=kernel)
    torch.cuda.synchronize()
    a = {k: (_np(v) if v is not None else None) for k, v in a.items()}
    r = _dens(F, X[rows], K, exclude=rows, G=G, method=1, kernel=kernel, dist=True,
              adjust=("theta", "weight", "coef", "rank", "status"))
    for k in ("idx", "dist", "theta", "weight", "coef", "rank", "status"):
        assert np.array_equal(r[k], a[k]), k
    if kernel == 0 and K > 1:
        assert np.all(a["weight"][:, -1] == 0) and np.all(a["weight"][:, 0] > 0)
    _check_all(a["theta"], a["weight"], r, G)
    print("worst relative density error so far", WORST["rel"])


def _generic(ctx, V, w=None, **kw):
    from abcsmc_amd import abcutil
    return abcutil.weighted_density(V, w, ctx=ctx, **kw)


def test_generic_weights_with_zeros_and_options(ctx):
    rng = np.random.default_rng(11)
    K, P, G = 700, 3, 65
    V = rng.normal(size=(K, P)) * np.array([1.0, 30.0, 1e-3]) + np.array([0.0, -200.0, 5.0])
    w = rng.uniform(0, 1, size=K)
    w[::7] = 0.0
    w[0] = 0.0                                                  # the first positive weight is not entry 0
    r = _generic(ctx, V, w, G=G)
    _check_all(V[None], w[None], {k: v[None] for k, v in r.items()}, G)
    r = _generic(ctx, V, w, G=G, bw_scale=0.37, cut=0.0)
    _check_all(V[None], w[None], {k: v[None] for k, v in r.items()}, G, bw_scale=0.37, cut=0.0)
    assert np.array_equal(r["grid"][:, 0], np.array([V[w > 0, j].min() for j in range(P)]))
    bw = np.array([0.5, 11.0, 2e-4])
    r = _generic(ctx, V, w, G=G, bw=bw, bw_scale=5.0)            # given bandwidths: bw_scale is not applied
    _check_all(V[None], w[None], {k: v[None] for k, v in r.items()}, G, bw=bw[None])
    # zero-weight entries change nothing
    keep = w > 0
    r0 = _generic(ctx, V, w, G=G)
    r1 = _generic(ctx, V[keep], w[keep], G=G)
    for k in ("bw", "grid"):
        assert np.allclose(r0[k], r1[k], rtol=1e-12), k


def test_discrete_equal_and_offset_values(ctx):
    rng = np.random.default_rng(12)
    K, G = 600, 512
    disc = rng.integers(0, 4, size=K).astype(np.float64)       # four atoms
    two = np.where(np.arange(K) % 2 == 0, -1.0, 1.0)            # two equal peaks
    const = np.full(K, -2.5)                                    # all equal: s = 0 and IQR = 0, h from |v|
    zeros = np.zeros(K)                                         # ... and from 1
    offset = 1e6 + rng.normal(size=K)                           # a one-pass variance would lose the spread
    V = np.stack([disc, two, const, zeros, offset], axis=1)
    r = _generic(ctx, V, G=G)
    _check_all(V[None], None, {k: v[None] for k, v in r.items()}, G)
    assert r["bw"][2] == pytest.approx(0.9 * 2.5 * K ** -0.2, rel=1e-14) and r["bw"][3] == pytest.approx(0.9 * K ** -0.2, rel=1e-14)
    assert r["bw"][4] == pytest.approx(D.bandwidth(offset)[0], rel=1e-9) and 0.15 < r["bw"][4] < 0.35
    # cut = 0 with all values equal: every grid point is the same point, so every density is the same bits and the
    # mode is the first, in one chunk (G = 65) and across chunks (G = 4096)
    for g in (2, 65, 4096):
        t = _generic(ctx, V[:, 2:4], G=g, cut=0.0)
        assert np.all(t["grid"][:, 1] == 0) and np.all(t["dens"] == t["dens"][:, :1])
        assert np.array_equal(t["mode"], t["grid"][:, 0]) and np.array_equal(t["mode_dens"], t["dens"][:, 0])
    # K = 1 through the generic entry
    one = _generic(ctx, np.array([[3.0, 0.0]]), G=63)
    _check_all(np.array([[[3.0, 0.0]]]), None, {k: v[None] for k, v in one.items()}, 63)
    assert one["bw"][0] == pytest.approx(2.7, rel=1e-14) and one["bw"][1] == pytest.approx(0.9, rel=1e-14)


def test_nan_and_inf_segments(ctx):
    X, Y = _wl(5, 3, 1500, 3)
    Y = Y.copy()
    Y[::50, 1] = np.nan
    Y[7::90, 2] = np.inf
    F = _fit(ctx, X, np.nan_to_num(Y, nan=0.0, posinf=0.0), 3)
    import torch
    from abcsmc_amd import device
    F["Yd"] = device.colmajor(Y, DEV)
    rows = np.arange(6) * 9
    r = _dens(F, X[rows], 200, exclude=rows, G=65)
    vals = Y[r["idx"]]
    bad = ~np.isfinite(vals).all(axis=1)                        # (B, P)
    assert bad[:, 1].any() and bad[:, 2].any() and not bad[:, 0].any() and not bad.all()
    assert np.array_equal(np.isnan(r["mode"]), bad) and np.array_equal(np.isnan(r["dens"]).all(axis=2), bad)
    _check_all(vals, None, r, 65)
    torch.cuda.synchronize()


def test_invariance(ctx):
    import torch
    from abcsmc_amd import abcutil, device
    X, Y = _wl(6, 3, 4000, 21)
    B, K, G = 40, 600, 512
    rows = np.arange(B) * 13
    names = ("dens", "grid", "bw", "mode", "mode_dens")
    for method in ("rejection", "loclinear"):
        kw = dict(method=method, exclude=rows, G=G, ctx=ctx)
        full = abcutil.particle_ranking_PLS_targets_density(X, Y, X[rows], 0.5, K, **kw)
        for b in (0, 17, 39):                                   # alone and inside the batch
            kw1 = dict(kw, exclude=rows[b:b + 1])
            one = abcutil.particle_ranking_PLS_targets_density(X, Y, X[rows[b:b + 1]], 0.5, K, **kw1)
            for k in names:
                assert np.array_equal(one[k][0], full[k][b]), (method, b, k)
        again = abcutil.particle_ranking_PLS_targets_density(X, Y, X[rows], 0.5, K, **kw)
        for k in names + ("idx", "dist"):
            assert np.array_equal(again[k], full[k]), (method, k)
        nod = abcutil.particle_ranking_PLS_targets_density(X, Y, X[rows], 0.5, K, dens=False, **kw)
        assert nod["dens"] is None
        for k in ("mode", "mode_dens", "bw", "grid"):          # the mode does not depend on dens being written
            assert np.array_equal(nod[k], full[k]), (method, k)
        assert np.allclose(full["x"][..., 0], full["grid"][..., 0]) and full["x"].shape == (B, 3, G)
        # the device entry with the same fit: the same bits
        F = _fit(ctx, X, Y, 3)
        dev = _dens(F, X[rows], K, exclude=rows, G=G, method=0 if method == "rejection" else 1)
        assert np.array_equal(dev["idx"], full["idx"].astype(np.int64))
        for k in names:
            assert np.array_equal(dev[k], full[k]), (method, k)
        nod = _dens(F, X[rows], K, exclude=rows, G=G, method=0 if method == "rejection" else 1, dens=False)
        assert np.array_equal(nod["mode"], full["mode"]) and np.array_equal(nod["mode_dens"], full["mode_dens"])
    # more than one grid chunk: the mode with and without dens
    a = abcutil.particle_ranking_PLS_targets_density(X, Y, X[rows[:3]], 0.5, K, G=1500, ctx=ctx)
    b = abcutil.particle_ranking_PLS_targets_density(X, Y, X[rows[:3]], 0.5, K, G=1500, dens=False, ctx=ctx)
    assert np.array_equal(a["mode"], b["mode"]) and np.array_equal(a["mode_dens"], b["mode_dens"])
    g = np.argmax(a["dens"], axis=2)
    assert np.array_equal(a["mode_dens"], np.take_along_axis(a["dens"], g[..., None], axis=2)[..., 0])
    # the generic entry: device and host
    rng = np.random.default_rng(2)
    V = rng.normal(size=(3000, 4))
    w = rng.uniform(0, 1, size=3000)
    h = abcutil.weighted_density(V, w, G=65, ctx=ctx)
    d = device.weighted_density(torch.tensor(V.T.copy(), device=DEV), torch.tensor(w), G=65)
    for k in names:
        assert np.array_equal(_np(d[k]), h[k]), k
    _check_all(V[None], w[None], {k: v[None] for k, v in h.items()}, 65)
    print("worst relative density error so far", WORST["rel"])


def test_argument_errors(ctx):
    import torch
    from abcsmc_amd import _lib, abcutil, device
    X, Y = _wl(5, 3, 800, 4)
    F = _fit(ctx, X, Y, 3)
    T = X[:4]
    L = _lib.lib()
    INVALID, UNSUPPORTED = -1, -4
    N, M, P, G = 800, 5, 3, 16
    Xf, Yf, Tf = np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(T)
    Yw = np.asfortranarray(np.random.default_rng(0).standard_normal((N, 1025)))
    hp = lambda v: v.ctypes.data_as(C.c_void_p) if v is not None else None
    dp = lambda t: t.data_ptr() if t is not None else None
    Td = device.colmajor(T, DEV)
    hmode, dmode = np.empty(4 * 1025), torch.empty(4 * 1025, dtype=torch.float64, device=DEV)
    hbw, dbw = np.ones(4 * P), torch.ones(4 * P, dtype=torch.float64, device=DEV)

    def den(mode, G=G, cut=3.0, bw_scale=1.0, bw=None):
        return _lib.Density(G, cut, bw_scale, bw, None, None, None, mode, None)

    def host(B=4, K=50, ex=None, Xm=Xf, Ym=Yf, Pm=P, Tm=Tf, mc=3, method=0, kernel=0, dn=den(hp(hmode))):
        return L.abc_particle_ranking_pls_targets_density(ctx.handle, hp(Xm), hp(Ym), N, M, Pm, hp(Tm), B, 0.5, mc, 0, hp(ex), K,
                                                          method, kernel, None, None, None, C.byref(dn) if dn is not None else None,
                                                          None)

    def dev(B=4, K=50, ex=None, Xm=F["Xd"], Ym=F["Yd"], Pm=P, tg=Td, md=F["model"], A=3, ldx=N, ldy=N, ldt=4, method=0, kernel=0,
            dn=den(dmode.data_ptr())):
        return L.abc_rank_targets_density_dev(ctx.handle, dp(Xm), ldx, dp(Ym), ldy, N, M, Pm, dp(md), A, dp(tg), ldt, B, dp(ex), K,
                                              method, kernel, None, None, None, C.byref(dn) if dn is not None else None)

    def refused(rc, code):
        assert rc == code, rc
        assert L.abc_last_error(ctx.handle)

    U = lambda v: np.array(v, dtype=np.int64).astype(np.uint64)
    exd = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
    for call, buf, ex, bwbuf, mk in ((host, hp(hmode), U, hbw, lambda a: hp(a)),
                                     (dev, dmode.data_ptr(), exd, dbw, lambda t: t.data_ptr())):
        for bad in (dict(dn=None), dict(dn=den(buf, G=1)), dict(dn=den(buf, G=0)), dict(dn=den(buf, G=4097)),
                    dict(dn=den(buf, cut=-1.0)), dict(dn=den(buf, cut=np.nan)), dict(dn=den(buf, cut=np.inf)),
                    dict(dn=den(buf, bw_scale=0.0)), dict(dn=den(buf, bw_scale=-2.0)), dict(dn=den(buf, bw_scale=np.nan)),
                    dict(dn=den(buf, bw_scale=np.inf)), dict(dn=den(None)),
                    dict(B=0), dict(K=0), dict(K=N + 1), dict(K=N, ex=ex([3, -1, -1, -1])), dict(ex=ex([N, -1, -1, -1])),
                    dict(Xm=None), dict(Ym=None), dict(method=2), dict(method=-1), dict(kernel=2), dict(kernel=-1)):
            refused(call(**bad), INVALID)
        refused(call(**{"Tm" if call is host else "tg": None}), INVALID)
        refused(call(**{"mc" if call is host else "A": 65}), UNSUPPORTED)
        for v in (0.0, -1.0, np.nan, np.inf):                   # a given bandwidth, checked on the device
            bwbuf[5] = v
            refused(call(dn=den(buf, bw=mk(bwbuf))), INVALID)
        bwbuf[5] = 1.0
        assert call(dn=den(buf, bw=mk(bwbuf))) == 0
        assert call(dn=den(buf, G=2)) == 0 and call(dn=den(buf, cut=0.0)) == 0
    refused(host(Ym=Yw, Pm=1025), UNSUPPORTED)
    refused(dev(Ym=device.colmajor(Yw, DEV), Pm=1025), UNSUPPORTED)
    for bad in (dict(ldx=N - 1), dict(ldy=N - 1), dict(ldt=3), dict(md=None), dict(A=0)):
        refused(dev(**bad), INVALID)
    # the generic entries: the summaries' checks of V, ldv, K, P and the weights
    V = np.random.default_rng(0).normal(size=(100, 2))
    Vd = torch.tensor(V.T.copy(), device=DEV)
    for bad_w in (-np.ones(100), np.zeros(100), np.where(np.arange(100) == 7, np.nan, 1.0), np.where(np.arange(100) == 7, np.inf, 1.0)):
        with pytest.raises(RuntimeError):
            abcutil.weighted_density(V, bad_w, ctx=ctx)
        with pytest.raises(RuntimeError):
            device.weighted_density(Vd, torch.tensor(bad_w))
    dn = den(dmode.data_ptr())
    for args in ((Vd.data_ptr(), 100, 0, 2), (Vd.data_ptr(), 100, 100, 0), (Vd.data_ptr(), 99, 100, 2), (None, 100, 100, 2)):
        refused(L.abc_weighted_density_dev(ctx.handle, *args, None, C.byref(dn)), INVALID)
    refused(L.abc_weighted_density_dev(ctx.handle, Vd.data_ptr(), 100, 100, 2, None, None), INVALID)
    refused(L.abc_weighted_density_dev(ctx.handle, Vd.data_ptr(), 100, 100, 2, None, C.byref(den(dmode.data_ptr(), G=1))), INVALID)
    refused(L.abc_weighted_density(ctx.handle, hp(np.asfortranarray(V)), 100, 2, None, C.byref(den(None))), INVALID)
    for kw in (dict(bw=-1.0), dict(bw=[1.0, np.nan]), dict(G=5000), dict(cut=-0.5), dict(bw_scale=0.0)):
        with pytest.raises(RuntimeError):
            abcutil.weighted_density(V, ctx=ctx, **kw)
    with pytest.raises(ValueError):
        abcutil.cross_validate_pls(X, Y, 4, 50, seed=1, ctx=ctx, statistic="max")
    torch.cuda.synchronize()
    # the context still works after the errors
    r = abcutil.weighted_density(V, G=63, ctx=ctx)
    _check_all(V[None], None, {k: v[None] for k, v in r.items()}, 63)


def test_cross_validate_mode(ctx):
    from abcsmc_amd import abcutil
    X, Y = _wl(8, 4, 3000, 17)
    base = abcutil.cross_validate_pls(X, Y, 40, 300, seed=3, ctx=ctx)
    assert sorted(base) == ["idx", "ncomp", "post_mean", "pred_error", "rows", "theta"]
    plain = abcutil.particle_ranking_PLS_targets(X, Y, X[base["rows"]], 0.5, 300, exclude=base["rows"], details=True, ctx=ctx)
    assert np.array_equal(base["post_mean"], plain["post_mean"]) and np.array_equal(base["idx"], plain["idx"])
    for method in ("rejection", "loclinear"):
        cv = abcutil.cross_validate_pls(X, Y, 40, 300, seed=3, ctx=ctx, method=method, statistic="mode")
        assert np.array_equal(cv["rows"], base["rows"]) and "post_mean" not in cv
        direct = abcutil.particle_ranking_PLS_targets_density(X, Y, X[cv["rows"]], 0.5, 300, method=method, exclude=cv["rows"],
                                                              ctx=ctx)
        assert np.array_equal(cv["post_mode"], direct["mode"]) and np.array_equal(cv["idx"], direct["idx"])
        assert cv["pred_error"].shape == (4,) and np.all(np.isfinite(cv["pred_error"]))
        var = cv["theta"].var(axis=0, ddof=1)
        assert np.allclose(cv["pred_error"], ((cv["post_mode"] - cv["theta"]) ** 2).sum(axis=0) / (40 * var), rtol=1e-12)
